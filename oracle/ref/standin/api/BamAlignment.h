#pragma once
#include <string>
#include <vector>
#include <cstdint>
namespace BamTools { struct CigarOp { char Type; uint32_t Length; }; struct BamAlignment { std::string Name, QueryBases, AlignedBases, Qualities; int32_t RefID=0, Position=0; std::vector<CigarOp> CigarData; }; }
