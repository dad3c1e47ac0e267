/* Symbols that the reference objects of libhlala_ref.so name but that no pinned path reaches, and whose own source does not compile
 * against the stand-ins (simulator/readSimulator.cpp draws from Boost's random number library).  The library is opened with RTLD_NOW,
 * so they have to exist; each one reports its name and ends the process.  None returns. */
#include "simulator/readSimulator.h"

#include <cstdio>
#include <cstdlib>

namespace {
[[noreturn]] void not_linked(const char* name)
{
    std::fprintf(stderr, "oracle/ref: %s is not part of the reference build (ref_stubs.cpp)\n", name);
    std::abort();
}
}

namespace simulator {
readSimulator::readSimulator(std::string, unsigned int, bool, char, char) { not_linked("simulator::readSimulator::readSimulator"); }
std::pair<double, double> readSimulator::averageErrorRate_R1_R2() { not_linked("simulator::readSimulator::averageErrorRate_R1_R2"); }
std::vector<oneReadPair> readSimulator::simulate_paired_reads_from_string(std::string, double, double, double, bool, std::string) { not_linked("simulator::readSimulator::simulate_paired_reads_from_string"); }
}
