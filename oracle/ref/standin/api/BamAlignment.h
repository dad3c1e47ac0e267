#pragma once
/* Stand-in for BamTools' api/BamAlignment.h, written from the interface as the reference's mapper uses it.  A record is plain data
 * that the driver (../ref_driver.cpp) fills in; the flag queries read AlignmentFlag with the bits of the SAM specification.  Members
 * that decode a record or depend on BamTools' own arithmetic (BuildCharData, GetTag, HasTag, GetTagType, GetEndPosition) throw an exception that carries their name. */
#include <string>
#include <vector>
#include <cstdint>
#include "BamAux.h"
#include "../standin_fail.h"
namespace BamTools {
struct CigarOp { char Type; uint32_t Length; CigarOp(char type = '\0', uint32_t length = 0) : Type(type), Length(length) {} };
struct BamAlignment {
    std::string Name, QueryBases, AlignedBases, Qualities, TagData, Filename;
    int32_t Length = 0, RefID = -1, Position = -1, MateRefID = -1, MatePosition = -1, InsertSize = 0;
    uint16_t Bin = 0, MapQuality = 0;
    uint32_t AlignmentFlag = 0;
    std::vector<CigarOp> CigarData;
    bool IsPaired() const { return AlignmentFlag & 0x1; }
    bool IsProperPair() const { return AlignmentFlag & 0x2; }
    bool IsMapped() const { return !(AlignmentFlag & 0x4); }
    bool IsMateMapped() const { return !(AlignmentFlag & 0x8); }
    bool IsReverseStrand() const { return AlignmentFlag & 0x10; }
    bool IsMateReverseStrand() const { return AlignmentFlag & 0x20; }
    bool IsFirstMate() const { return AlignmentFlag & 0x40; }
    bool IsSecondMate() const { return AlignmentFlag & 0x80; }
    bool IsPrimaryAlignment() const { return !(AlignmentFlag & 0x100); }
    bool IsFailedQC() const { return AlignmentFlag & 0x200; }
    bool IsDuplicate() const { return AlignmentFlag & 0x400; }
    void SetIsReverseStrand(bool ok) { if(ok) AlignmentFlag |= 0x10; else AlignmentFlag &= ~0x10u; }
    bool BuildCharData() { standin::undefined("BamAlignment::BuildCharData"); }
    int GetEndPosition(bool usePadded = false, bool closedInterval = false) const { (void)usePadded; (void)closedInterval; standin::undefined("BamAlignment::GetEndPosition"); }
    bool HasTag(const std::string& tag) const { (void)tag; standin::undefined("BamAlignment::HasTag"); }
    bool GetTagType(const std::string& tag, char& type) const { (void)tag; (void)type; standin::undefined("BamAlignment::GetTagType"); }
    template<class T> bool GetTag(const std::string& tag, T& destination) const { (void)tag; (void)destination; standin::undefined("BamAlignment::GetTag"); }
};
}
