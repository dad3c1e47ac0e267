#pragma once
/* Stand-in for BamTools' api/BamReader.h: the member functions the reference's mapper names.  None of them works: the reference build
 * of oracle/ref/ reads no BAM file, and every member ends the process with its name. */
#include "BamAlignment.h"
namespace BamTools {
typedef std::vector<RefData> RefVector;
struct BamReader {
    bool Open(const std::string&) { standin::unavailable("BamReader::Open"); }
    bool Close() { standin::unavailable("BamReader::Close"); }
    bool IsOpen() const { standin::unavailable("BamReader::IsOpen"); }
    bool Rewind() { standin::unavailable("BamReader::Rewind"); }
    bool Jump(int, int = 0) { standin::unavailable("BamReader::Jump"); }
    bool SetRegion(const BamRegion&) { standin::unavailable("BamReader::SetRegion"); }
    bool SetRegion(int, int, int, int) { standin::unavailable("BamReader::SetRegion"); }
    bool GetNextAlignment(BamAlignment&) { standin::unavailable("BamReader::GetNextAlignment"); }
    bool GetNextAlignmentCore(BamAlignment&) { standin::unavailable("BamReader::GetNextAlignmentCore"); }
    bool LocateIndex() { standin::unavailable("BamReader::LocateIndex"); }
    bool HasIndex() const { standin::unavailable("BamReader::HasIndex"); }
    bool OpenIndex(const std::string&) { standin::unavailable("BamReader::OpenIndex"); }
    int GetReferenceCount() const { standin::unavailable("BamReader::GetReferenceCount"); }
    int GetReferenceID(const std::string&) const { standin::unavailable("BamReader::GetReferenceID"); }
    const RefVector& GetReferenceData() const { standin::unavailable("BamReader::GetReferenceData"); }
    std::string GetHeaderText() const { standin::unavailable("BamReader::GetHeaderText"); }
    std::string GetErrorString() const { standin::unavailable("BamReader::GetErrorString"); }
};
}
