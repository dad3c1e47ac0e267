#pragma once
#include <sstream>
#include <string>
#include <stdexcept>
namespace boost { struct bad_lexical_cast : std::runtime_error { bad_lexical_cast() : std::runtime_error("bad_lexical_cast") {} };
template<class T, class S> T lexical_cast(const S& s) { std::stringstream ss; ss << s; T t; ss >> t; if(ss.fail()) throw bad_lexical_cast(); return t; }
template<> inline std::string lexical_cast<std::string, std::string>(const std::string& s) { return s; } }
