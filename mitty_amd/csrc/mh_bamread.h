// mh_bamread.h — the structural check every BAM record passes on the host before it is handed out by the reader
// (mh_bamread.cpp) or uploaded to a record session (mh_recs.hip).  Plain C++ (no HIP).
#pragma once

#include <cstdint>
#include <string>

namespace mh {

constexpr int64_t BAM_REC_MAX = (int64_t)1 << 28;   // a record's block_size bound (bytes)

// rec: the record with its 4-byte block_size; size: the bytes it occupies (4 + block_size).  True when the fixed
// fields, the NUL-terminated read name, the CIGAR, the packed sequence and the qualities fit inside block_size:
//   l_read_name >= 1, name[l_read_name - 1] == 0, 32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq <= block_size
bool bam_record_ok(const uint8_t *rec, int64_t size, std::string *why);

}  // namespace mh
