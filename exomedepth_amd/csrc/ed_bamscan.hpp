// ed_bamscan.hpp -- walk the records of an inflated BAM stream and copy out the four fields the read counter needs.  Host only: no HIP
// include, nothing of the library's; edcore.hip wraps it as ed_bam_scan_records, and tools/bamscan_check.cpp compiles the same body into a
// stand-alone program that runs it under the host sanitizers.
//
// A BAM alignment record (SAM specification, section 4.2) is  block_size:int32  followed by block_size bytes, the first 32 of which are
//   refID:int32  pos:int32  l_read_name:uint8  mapq:uint8  bin:uint16  n_cigar_op:uint16  flag:uint16  l_seq:uint32
//   next_refID:int32  next_pos:int32  tlen:int32
// all little-endian and unaligned.  Everything after them (read name, CIGAR, bases, qualities, tags) is skipped by block_size alone.
#pragma once

#include <cstdint>

namespace edbam {

constexpr int32_t kFixed = 32;              // bytes of a record that every record has (after the block_size word)
constexpr int32_t kMaxBlock = 1 << 28;      // a record longer than this is taken for a corrupt stream, not for a read

enum : int { kScanOk = 0, kScanBadBlock = 1 };

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// Records of buf[0, n_bytes), at most cap of them, into the four arrays.  Stops before the first record that is not wholly inside the buffer
// (or at cap); *bytes_consumed is then the offset of that record -- always a record boundary -- and the caller carries the rest into its next
// buffer.  A block_size below kFixed or above kMaxBlock (a negative one included) ends the scan with kScanBadBlock: *bad_offset is where the
// word lies and *bad_value what it holds; the records before it have been written and counted.  No byte outside [buf, buf + n_bytes) is read.
inline int scan_records(const uint8_t* buf, int64_t n_bytes, int64_t cap, int32_t* refid, int32_t* pos, int32_t* tlen, uint32_t* flag_mapq,
                        int64_t* n_records, int64_t* bytes_consumed, int64_t* bad_offset, int32_t* bad_value)
{
  int64_t off = 0, n = 0;
  int rc = kScanOk;
  while (n < cap && n_bytes - off >= 4) {
    const int32_t bs = (int32_t)le32(buf + off);
    if (bs < kFixed || bs > kMaxBlock) {
      *bad_offset = off; *bad_value = bs;
      rc = kScanBadBlock;
      break;
    }
    if (n_bytes - off - 4 < (int64_t)bs) break;     // the record's tail is in the next buffer
    const uint8_t* r = buf + off + 4;
    refid[n] = (int32_t)le32(r);
    pos[n] = (int32_t)le32(r + 4);
    tlen[n] = (int32_t)le32(r + 28);
    flag_mapq[n] = le16(r + 14) | ((uint32_t)r[9] << 16);
    ++n;
    off += 4 + (int64_t)bs;
  }
  *n_records = n;
  *bytes_consumed = off;
  return rc;
}

}  // namespace edbam
