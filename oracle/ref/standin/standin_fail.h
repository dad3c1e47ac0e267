#pragma once
/* Stand-in members that would read or decode a BAM file end the process with their name: the reference build of
 * oracle/ref/ runs no I/O of BamTools or Boost, and a call that reaches one is a mistake of the driver. */
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
namespace standin { [[noreturn]] inline void unavailable(const char* what) { std::fprintf(stderr, "oracle/ref stand-in: %s is not available (no BAM or archive I/O in the reference build)\n", what); std::abort(); }
/* Members that read no file but depend on BamTools' own decoding or arithmetic (the reference calls them when it prints a record before a failing assert) throw:
 * the driver turns the exception into the failure of its call. */
[[noreturn]] inline void undefined(const char* what) { throw std::logic_error(std::string("oracle/ref stand-in: ") + what + " is not defined by the stand-in"); } }
