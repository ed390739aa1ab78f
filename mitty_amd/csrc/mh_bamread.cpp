// mh_bamread.cpp — host BAM reader for the alignment scorers (the reference reads its BAMs through
// pysam.AlignmentFile / fetch, mitty/benchmarking/mq.py:21,61-62, derr.py:20,65-66).  Plain C++ with zlib, no HIP.
//
//   file (mapped) -> BGZF block headers walked in order (BSIZE from the 'BC' extra field, ISIZE from the trailer, so
//                    every block's place in the uncompressed stream is known before it is inflated)
//                 -> raw inflate of a batch of blocks on `threads` threads, CRC32 and ISIZE checked per block (or, for a
//                    handle of mh_bamfile_open_gpu, the batch inflated and checked in one launch: mh_inflate.hip)
//                 -> the BAM header (text, n_ref, names, lengths), then the record stream handed out in chunks cut at
//                    record boundaries, with each chunk's record offsets; the chunk after the one handed out is
//                    inflated and cut by a thread of the handle meanwhile (read-ahead, a second buffer)
//
// The file is untrusted: every length is checked against the bytes at hand before it is used, and every record passes
// bam_record_ok before it is handed out.  No index is needed and the records may be in any order.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mitty_hip.h"
#include "mh_bamread.h"
#define MH_INFLATE_OPTIONAL   // (this file links without mh_inflate.hip too: see mh_inflate.h)
#include "mh_inflate.h"

namespace mh {

static inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
static inline uint32_t le32(const uint8_t *p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

bool bam_record_ok(const uint8_t *rec, int64_t size, std::string *why) {
  auto bad = [&](const char *m) {
    if (why) *why = m;
    return false;
  };
  if (size < 36) return bad("record shorter than its fixed fields");
  const int64_t bs = (int64_t)le32(rec);
  if (bs + 4 != size) return bad("block_size does not match the record's bytes");
  const int64_t lrn = rec[12], ncig = le16(rec + 16), lseq = (int64_t)(int32_t)le32(rec + 20);
  if (lrn < 1) return bad("l_read_name is 0");
  if (lseq < 0) return bad("negative l_seq");
  if (32 + lrn + 4 * ncig + (lseq + 1) / 2 + lseq > bs) return bad("name, CIGAR, sequence and qualities exceed block_size");
  if (rec[36 + lrn - 1] != 0) return bad("read name is not NUL-terminated");
  return true;
}

}  // namespace mh

using mh::le16;
using mh::le32;

struct mh_bamfile {
  std::string err;
  int fd = -1;
  const uint8_t *map = nullptr;
  int64_t fsize = 0, fpos = 0;   // the mapped file and the next BGZF block's offset
  int threads = 1;
  mh::Inflater *gpu = nullptr;   // mh_bamfile_open_gpu: fill() hands its batch to the device instead of the threads
  // Uncompressed bytes not handed out yet, [head, buf.size()), and the chunk cut from them.  Two sides: while the caller
  // works on the chunk of one, a thread of the handle inflates and cuts the next chunk in the other (read-ahead).
  struct Side {
    std::vector<uint8_t> buf;
    int64_t head = 0;
    std::vector<int64_t> roff;   // the chunk's record offsets (from head)
    int64_t len = 0;             // its bytes
    int32_t rc = MH_OK;
    bool ready = false;          // holds a chunk cut ahead
  };
  Side side[2];
  int cur = 0;
  std::thread ahead;
  std::string text, names;       // header text; reference names, NUL-separated
  std::vector<int64_t> lens;
  bool failed = false;
  bool opened = false;            // the header was read (never written after mh_bamfile_open)
};

namespace {

int32_t fail(mh_bamfile *f, const std::string &m) {
  f->err = m;
  f->failed = true;
  return MH_E_ARG;
}

struct Blk {
  int64_t cpos, clen;   // the deflate payload in the file
  int64_t dst;          // its place in buf
  uint32_t crc, isize;
};

// The BGZF block header at file offset o (p: its bytes, left: the bytes from there to the end): the payload's place,
// CRC32 and ISIZE into b, the block's size into *bsize.  False with the message in *why.
bool walk_block(const uint8_t *p, int64_t o, int64_t left, Blk *b, int64_t *bsize_out, std::string *why) {
  auto bad = [&](const char *m) {
    *why = m + std::to_string(o);
    return false;
  };
  if (left < 18) return bad("truncated BGZF block header at offset ");
  if (p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) return bad("not a BGZF block at offset ");
  const int64_t xlen = le16(p + 10);
  if (12 + xlen > left) return bad("truncated BGZF extra field at offset ");
  int64_t bsize = -1;
  for (int64_t x = 12; x + 4 <= 12 + xlen;) {
    const int64_t slen = le16(p + x + 2);
    if (x + 4 + slen > 12 + xlen) break;
    if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2) bsize = (int64_t)le16(p + x + 4) + 1;
    x += 4 + slen;
  }
  if (bsize < 0) return bad("BGZF block without a BC field at offset ");
  if (bsize < 12 + xlen + 8) return bad("BGZF block size too small at offset ");
  if (bsize > left) return bad("truncated BGZF block at offset ");
  b->cpos = o + 12 + xlen;
  b->clen = bsize - 12 - xlen - 8;
  b->crc = le32(p + bsize - 8);
  b->isize = le32(p + bsize - 4);
  if (b->isize > 65536) return bad("BGZF block ISIZE over 64 KiB at offset ");
  *bsize_out = bsize;
  return true;
}

std::string inflate_message(int64_t cpos) {
  return "BGZF block fails to inflate or its CRC32 / ISIZE differs (payload at offset " + std::to_string(cpos) + ")";
}

// blks inflated on the device into out (each at its dst - dst0).  *bad: the lowest failing payload offset, or -1.
int32_t inflate_gpu(mh::Inflater *g, const uint8_t *map, const std::vector<Blk> &blks, int64_t dst0, uint8_t *out,
                    int64_t out_bytes, int threads, int64_t *bad, std::string *err) {
  std::vector<mh::InflateMember> m(blks.size());
  for (size_t k = 0; k < blks.size(); k++)
    m[k] = mh::InflateMember{blks[k].cpos, blks[k].dst - dst0, (uint32_t)blks[k].clen, blks[k].isize, blks[k].crc, 0};
  *bad = -1;
  const int32_t rc = mh::inflater_run(g, map, m.data(), m.size(), out, out_bytes, threads, err);
  if (rc != MH_OK) return rc;
  for (size_t k = 0; k < m.size(); k++)
    if (m[k].status != 0 && (*bad < 0 || blks[k].cpos < *bad)) *bad = blks[k].cpos;
  return MH_OK;
}

// Inflates BGZF blocks from fpos until at least `want` more bytes are in buf or the file ends.
int32_t fill(mh_bamfile *f, mh_bamfile::Side &s, int64_t want) {
  std::vector<Blk> blks;
  if (s.head > 0) {   // keep only what has not been handed out
    s.buf.erase(s.buf.begin(), s.buf.begin() + s.head);
    s.head = 0;
  }
  const int64_t dst0 = (int64_t)s.buf.size();
  int64_t dst = dst0, got = 0;
  while (got < want && f->fpos < f->fsize) {
    const int64_t o = f->fpos;
    Blk b;
    int64_t bsize = 0;
    std::string why;
    if (!walk_block(f->map + o, o, f->fsize - o, &b, &bsize, &why)) return fail(f, why);
    b.dst = dst;
    dst += b.isize;
    got += b.isize;
    blks.push_back(b);
    f->fpos += bsize;
  }
  if (blks.empty()) return MH_OK;
  s.buf.resize((size_t)dst);
  if (f->gpu) {
    int64_t bad = -1;
    std::string err;
    const int32_t rc =
        inflate_gpu(f->gpu, f->map, blks, dst0, s.buf.data() + dst0, dst - dst0, f->threads, &bad, &err);
    if (rc != MH_OK) {
      f->err = err;
      f->failed = true;
      return rc;
    }
    if (bad >= 0) return fail(f, inflate_message(bad));
    return MH_OK;
  }
  std::atomic<size_t> next{0};
  std::atomic<int64_t> bad{-1};
  auto work = [&]() {
    z_stream z;
    uint8_t none = 0;   // where an empty block (ISIZE 0: the end-of-file marker) inflates to: zlib refuses a null output
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= blks.size()) return;
      const Blk &b = blks[k];
      memset(&z, 0, sizeof z);
      bool ok = inflateInit2(&z, -15) == Z_OK;
      if (ok) {
        z.next_in = const_cast<Bytef *>(f->map + b.cpos);
        z.avail_in = (uInt)b.clen;
        z.next_out = b.isize ? s.buf.data() + b.dst : &none;
        z.avail_out = b.isize;
        const int rc = inflate(&z, Z_FINISH);
        ok = rc == Z_STREAM_END && z.total_out == b.isize;
        inflateEnd(&z);
      }
      if (ok) ok = (uint32_t)crc32(crc32(0L, Z_NULL, 0), b.isize ? s.buf.data() + b.dst : &none, b.isize) == b.crc;
      if (!ok) {
        int64_t exp = -1;
        bad.compare_exchange_strong(exp, b.cpos);
      }
    }
  };
  const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)f->threads, blks.size()));
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; t++) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
  if (bad.load() >= 0) return fail(f, inflate_message(bad.load()));
  return MH_OK;
}

// Makes at least n bytes available from head; false when the file ends first (no error set).
int32_t need(mh_bamfile *f, int64_t n, bool *have) {
  mh_bamfile::Side &s = f->side[0];
  while ((int64_t)s.buf.size() - s.head < n && f->fpos < f->fsize) {
    const int32_t rc = fill(f, s, std::max<int64_t>(n - ((int64_t)s.buf.size() - s.head), 1 << 20));
    if (rc != MH_OK) return rc;
  }
  *have = (int64_t)s.buf.size() - s.head >= n;
  return MH_OK;
}

int32_t read_header(mh_bamfile *f) {
  bool have = false;
  int32_t rc = need(f, 12, &have);
  if (rc != MH_OK) return rc;
  if (!have) return fail(f, "truncated BAM header");
  if (memcmp(f->side[0].buf.data() + f->side[0].head, "BAM\1", 4) != 0) return fail(f, "bad BAM magic");
  const int64_t l_text = (int64_t)(int32_t)le32(f->side[0].buf.data() + f->side[0].head + 4);
  if (l_text < 0) return fail(f, "negative l_text in the BAM header");
  rc = need(f, 12 + l_text, &have);
  if (rc != MH_OK) return rc;
  if (!have) return fail(f, "truncated BAM header text");
  f->text.assign((const char *)f->side[0].buf.data() + f->side[0].head + 8, (size_t)l_text);
  const int64_t n_ref = (int64_t)(int32_t)le32(f->side[0].buf.data() + f->side[0].head + 8 + l_text);
  if (n_ref < 0) return fail(f, "negative n_ref in the BAM header");
  f->side[0].head += 12 + l_text;
  for (int64_t r = 0; r < n_ref; r++) {
    rc = need(f, 4, &have);
    if (rc != MH_OK) return rc;
    if (!have) return fail(f, "truncated BAM reference list");
    const int64_t l_name = (int64_t)(int32_t)le32(f->side[0].buf.data() + f->side[0].head);
    if (l_name < 1) return fail(f, "reference name of length < 1 in the BAM header");
    rc = need(f, 4 + l_name + 4, &have);
    if (rc != MH_OK) return rc;
    if (!have) return fail(f, "truncated BAM reference list");
    const uint8_t *p = f->side[0].buf.data() + f->side[0].head + 4;
    if (p[l_name - 1] != 0) return fail(f, "reference name is not NUL-terminated");
    f->names.append((const char *)p, strlen((const char *)p));
    f->names.push_back('\0');
    f->lens.push_back((int64_t)(int32_t)le32(p + l_name));
    f->side[0].head += 4 + l_name + 4;
  }
  return MH_OK;
}

// The next chunk of side s: whole records from s.head, about max_bytes bytes of them (at least one record), inflating
// more blocks as needed; s.roff / s.len describe it.  No record at the end of the file.
int32_t cut_chunk(mh_bamfile *f, mh_bamfile::Side &s, int64_t max_bytes) {
  s.roff.clear();
  s.roff.push_back(0);
  s.len = 0;
  int64_t o = 0;   // bytes of whole records found from head
  for (;;) {
    const int64_t avail = (int64_t)s.buf.size() - s.head;
    const uint8_t *p = s.buf.data() + s.head;
    bool more = false;   // the data at hand ends before the chunk is full
    while (o < max_bytes) {
      if (o + 4 > avail) { more = true; break; }
      const int64_t bs = (int64_t)le32(p + o);
      if (bs < 32 || bs > mh::BAM_REC_MAX) return fail(f, "BAM record with block_size " + std::to_string(bs));
      if (o + 4 + bs > avail) { more = true; break; }
      std::string why;
      if (!mh::bam_record_ok(p + o, 4 + bs, &why)) return fail(f, "malformed BAM record: " + why);
      o += 4 + bs;
      s.roff.push_back(o);
    }
    if (!more) break;
    if (f->fpos >= f->fsize) {
      if (o != avail) return fail(f, "BAM record cut by the end of the file");
      break;
    }
    // (fill drops the bytes before head, so the offsets found so far stay valid from the new head = 0)
    const int32_t rc = fill(f, s, std::max<int64_t>(max_bytes - avail + 4, 1));
    if (rc != MH_OK) return rc;
  }
  s.len = o;
  return MH_OK;
}

}  // namespace

extern "C" {

static int32_t bamfile_open(const char *path, int32_t device, int32_t threads, mh_bamfile **out) {
  if (!path || !out) return MH_E_ARG;
  *out = nullptr;
  mh_bamfile *f = new mh_bamfile();
  *out = f;
  f->threads = std::max(1, std::min(threads, 256));
  if (device >= 0) {
    if (!mh::inflater_create) return fail(f, "this build of the reader has no device inflater");
    const int32_t rc = mh::inflater_create(device, &f->gpu, &f->err);
    if (rc != MH_OK) {
      f->failed = true;
      return rc;
    }
  }
  f->fd = open(path, O_RDONLY);
  if (f->fd < 0) return fail(f, std::string("cannot open ") + path);
  struct stat st;
  if (fstat(f->fd, &st) != 0 || !S_ISREG(st.st_mode)) return fail(f, std::string("not a regular file: ") + path);
  f->fsize = (int64_t)st.st_size;
  if (f->fsize == 0) return fail(f, "empty file (no BGZF block)");
  void *m = mmap(nullptr, (size_t)f->fsize, PROT_READ, MAP_PRIVATE, f->fd, 0);
  if (m == MAP_FAILED) return fail(f, std::string("cannot map ") + path);
  f->map = (const uint8_t *)m;
  const int32_t rc = read_header(f);
  f->opened = rc == MH_OK;
  return rc;
}

int32_t mh_bamfile_open(const char *path, int32_t threads, mh_bamfile **out) {
  return bamfile_open(path, -1, threads, out);
}

int32_t mh_bamfile_open_gpu(const char *path, int32_t device, int32_t threads, mh_bamfile **out) {
  if (device < 0) return MH_E_ARG;
  return bamfile_open(path, device, threads, out);
}

int32_t mh_bgzf_inflate_gpu(int32_t device, const char *in, int64_t len, char *out, int64_t cap, int64_t *used,
                            int64_t *bad_offset) {
  if (used) *used = 0;
  if (bad_offset) *bad_offset = -1;
  if (device < 0 || len < 0 || cap < 0 || (len > 0 && !in) || (cap > 0 && !out) || !used) return MH_E_ARG;
  const uint8_t *p = (const uint8_t *)in;
  std::vector<Blk> blks;
  std::vector<int64_t> at;   // the blocks' offsets
  int64_t dst = 0;
  for (int64_t o = 0; o < len;) {
    Blk b;
    int64_t bsize = 0;
    std::string why;
    if (!walk_block(p + o, o, len - o, &b, &bsize, &why)) {
      if (bad_offset) *bad_offset = o;
      return MH_E_ARG;
    }
    b.dst = dst;
    dst += b.isize;
    blks.push_back(b);
    at.push_back(o);
    o += bsize;
  }
  *used = dst;
  if (dst > cap) return MH_E_CAPACITY;
  if (blks.empty()) return MH_OK;
  mh::Inflater *g = nullptr;
  std::string err;
  if (!mh::inflater_create) return MH_E_STATE;
  int32_t rc = mh::inflater_create(device, &g, &err);
  if (rc != MH_OK) return rc;
  uint8_t none = 0;
  int64_t bad = -1;
  rc = inflate_gpu(g, p, blks, 0, cap > 0 ? (uint8_t *)out : &none, dst, 4, &bad, &err);
  mh::inflater_destroy(g);
  if (rc != MH_OK) return rc;
  if (bad >= 0) {
    int64_t o = 0;   // the block whose payload starts at `bad`
    for (size_t k = 0; k < blks.size(); k++)
      if (blks[k].cpos == bad) o = at[k];
    if (bad_offset) *bad_offset = o;
    return MH_E_ARG;
  }
  return MH_OK;
}

const char *mh_bamfile_error(const mh_bamfile *f) { return f ? f->err.c_str() : "null handle"; }

int32_t mh_bamfile_header(const mh_bamfile *f, const char **text, int64_t *text_len, int32_t *n_ref,
                          const char **names, const int64_t **lengths) {
  if (!f || !f->opened) return MH_E_ARG;   // (only fields the read-ahead thread never touches)
  if (text) *text = f->text.data();
  if (text_len) *text_len = (int64_t)f->text.size();
  if (n_ref) *n_ref = (int32_t)f->lens.size();
  if (names) *names = f->names.data();
  if (lengths) *lengths = f->lens.data();
  return MH_OK;
}

int32_t mh_bamfile_next(mh_bamfile *f, int64_t max_bytes, const uint8_t **recs, int64_t *len, const int64_t **roff,
                        int64_t *n) {
  if (!f || !recs || !len || !roff || !n) return MH_E_ARG;
  *recs = nullptr;
  *roff = nullptr;
  *len = *n = 0;
  if (f->ahead.joinable()) f->ahead.join();
  if (f->failed) return MH_E_ARG;
  if (max_bytes < 1) max_bytes = 1;
  mh_bamfile::Side &c = f->side[f->cur];
  if (!c.ready) c.rc = cut_chunk(f, c, max_bytes);   // (the first call, and calls after the end of the file)
  c.ready = false;
  if (c.rc != MH_OK) return c.rc;
  *n = (int64_t)c.roff.size() - 1;
  *len = c.len;
  *recs = c.buf.data() + c.head;
  *roff = c.roff.data();
  if (*n > 0) {
    // read-ahead: the bytes after this chunk move to the other side, where a thread of the handle inflates and cuts
    // the next chunk (of the same max_bytes) while the caller works on this one; this side is not touched meanwhile
    mh_bamfile::Side &o = f->side[f->cur ^ 1];
    o.buf.assign(c.buf.begin() + c.head + c.len, c.buf.end());
    o.head = 0;
    f->cur ^= 1;
    f->ahead = std::thread([f, &o, max_bytes]() {
      o.rc = cut_chunk(f, o, max_bytes);
      o.ready = true;
    });
  }
  return MH_OK;
}

int32_t mh_bamfile_close(mh_bamfile *f) {
  if (!f) return MH_OK;
  if (f->ahead.joinable()) f->ahead.join();
  if (f->map) munmap(const_cast<uint8_t *>(f->map), (size_t)f->fsize);
  if (f->fd >= 0) close(f->fd);
  if (f->gpu) mh::inflater_destroy(f->gpu);
  delete f;
  return MH_OK;
}

}  // extern "C"
