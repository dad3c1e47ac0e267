#pragma once
/* Stand-in for BamTools' api/BamAux.h, written from the interface as mapper/processBAM.cpp uses it: reference sequence entries and a region. */
#include <string>
#include <cstdint>
namespace BamTools {
namespace Constants {   /* tag type codes of the SAM/BAM specification */
const char BAM_TAG_TYPE_ASCII = 'A', BAM_TAG_TYPE_INT8 = 'c', BAM_TAG_TYPE_UINT8 = 'C', BAM_TAG_TYPE_INT16 = 's', BAM_TAG_TYPE_UINT16 = 'S',
           BAM_TAG_TYPE_INT32 = 'i', BAM_TAG_TYPE_UINT32 = 'I', BAM_TAG_TYPE_FLOAT = 'f', BAM_TAG_TYPE_STRING = 'Z', BAM_TAG_TYPE_HEX = 'H', BAM_TAG_TYPE_ARRAY = 'B';
}
struct RefData { std::string RefName; int32_t RefLength; RefData(const std::string& name = "", int32_t length = 0) : RefName(name), RefLength(length) {} };
struct BamRegion { int LeftRefID, LeftPosition, RightRefID, RightPosition; BamRegion(int leftID = -1, int leftPos = -1, int rightID = -1, int rightPos = -1) : LeftRefID(leftID), LeftPosition(leftPos), RightRefID(rightID), RightPosition(rightPos) {} };
}
