#pragma once
/* Stand-in for boost::archive::text_iarchive: reading a serialized graph is file input and ends the process. */
#include <iostream>
#include <fstream>
#include <sstream>
#include "../../standin_fail.h"
namespace boost { namespace archive {
struct text_iarchive { explicit text_iarchive(std::istream&) {} template<class T> text_iarchive& operator>>(T&) { standin::unavailable("boost::archive::text_iarchive"); } };
} }
