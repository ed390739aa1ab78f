// mh_inflate.h — the single-thread parts of the device BGZF inflater (mh_inflate.hip): the bit reader, the code-length
// code, canonical Huffman tables for code lengths up to 15, deflate's length / distance tables (RFC 1951 §3.2.5), the
// stored, fixed and dynamic block loops and the CRC-32 pieces.  __host__ __device__ under hipcc and plain C++ under a
// host compiler, so tests/inflate_host.cpp runs exactly this code on the CPU (under the sanitizers, against zlib) and
// mh_bamread.cpp reaches the inflater through the interface at the end without any HIP header.
//
// The input is untrusted.  Every input read is bounded by the payload length (BitReader::refill), every output write
// by the member's ISIZE (checked before Out::lit / copy / store are called), every distance by the bytes already
// written to this member, every table build is checked for over-subscription and incompleteness, and every loop
// consumes at least one input bit or produces one output byte per turn.  A bad stream ends with a status.
//
// Accept rule: zlib's.  A member is good exactly when inflate(Z_FINISH) with -15 window bits returns Z_STREAM_END with
// total_out == ISIZE and the CRC-32 matches: an incomplete code-length set is an error, an incomplete literal/length
// or distance set is allowed only as a single code of length 1, a missing end-of-block code is an error, HLIT > 286
// and HDIST > 30 are errors, symbols 286 / 287 and distance codes 30 / 31 are errors when used, repeat code 16 needs a
// previous length, LEN must equal ~NLEN, bytes after the final block are ignored.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MH_INF_HD __host__ __device__
#else
#define MH_INF_HD
#endif

namespace mh {
namespace inf {

enum : int32_t { ST_OK = 0, ST_BAD_STREAM = 1, ST_LENGTH = 2, ST_CRC = 3 };

constexpr int MAX_ISIZE = 65536;
constexpr int FAST_L = 10, FAST_D = 8, FAST_C = 7;   // bits of the first-level tables; longer codes walk the counts
constexpr int NLIT = 288, NDIST = 32, NCL = 19;      // alphabet sizes with the reserved symbols of the fixed codes

MH_INF_HD inline int len_base(int c) {   // c = symbol - 257, 0..28
  if (c < 8) return c + 3;
  if (c == 28) return 258;
  return 3 + ((4 + (c & 3)) << (c / 4 - 1));
}
MH_INF_HD inline int len_extra(int c) { return (c < 8 || c == 28) ? 0 : c / 4 - 1; }
MH_INF_HD inline int dist_base(int c) {   // 0..29
  if (c < 4) return c + 1;
  return 1 + ((2 + (c & 1)) << (c / 2 - 1));
}
MH_INF_HD inline int dist_extra(int c) { return c < 4 ? 0 : c / 2 - 1; }

MH_INF_HD inline int cl_order(int i) {   // §3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
  if (i < 3) return 16 + i;
  if (i == 3) return 0;
  const int k = i - 4;   // 8 7 9 6 10 5 ...
  return (k & 1) ? 7 - (k >> 1) : 8 + (k >> 1);
}

// Where the bit reader gets the payload's bytes from: the host reads the payload in place; the device stages it
// through LDS (mh_inflate.hip DevSource).  load64(pos) needs pos + 8 <= n, byte(pos) needs pos < n.
struct HostSource {
  const uint8_t *in;
  MH_INF_HD uint64_t load64(int64_t pos) const {
    uint64_t w;
    __builtin_memcpy(&w, in + pos, 8);   // little-endian hosts
    return w;
  }
  MH_INF_HD uint32_t byte(int64_t pos) const { return in[pos]; }
};

// LSB-first bit reader over the n bytes of a source.  buf holds at least cnt valid bits (bits above cnt, when set,
// are the stream's own next bits: refill ORs whole words in).  After refill cnt >= 48 unless the input is exhausted: a
// length / distance pair takes at most 15 + 5 + 15 + 13 bits, and a refill that finds 48 already there costs no load.
template <class S>
struct BitReader {
  S &src;
  int64_t n, pos;
  uint64_t buf;
  int cnt;
  MH_INF_HD void refill() {
    if (cnt >= 48) return;
    if (n - pos >= 8) {
      buf |= src.load64(pos) << cnt;
      const int adv = (63 - cnt) >> 3;
      pos += adv;
      cnt += adv * 8;
    } else {
      while (cnt < 56 && pos < n) {
        buf |= (uint64_t)src.byte(pos++) << cnt;
        cnt += 8;
      }
    }
  }
  MH_INF_HD uint32_t peek(int k) const { return (uint32_t)buf & ((1u << k) - 1u); }
  MH_INF_HD void drop(int k) {
    buf >>= k;
    cnt -= k;
  }
  MH_INF_HD uint32_t take(int k) {   // k <= 16, cnt >= k checked by the caller
    const uint32_t v = peek(k);
    drop(k);
    return v;
  }
};

// Decode tables of one deflate block (LDS on the device).  A first-level entry is symbol | length << 9, 0 for a code
// longer than the table's bits (or no code): those are found by walking count[] / sym[] a bit at a time.
struct Tables {
  uint16_t lfast[1 << FAST_L], dfast[1 << FAST_D], cfast[1 << FAST_C];
  uint16_t lcount[16], dcount[16], ccount[16], offs[48];   // offs: build_table's scratch
  uint16_t lsym[NLIT], dsym[NDIST], csym[NCL + 1];
  uint8_t lens[NLIT + NDIST];
};

// What the core needs from its surroundings besides the output: the host runs it on one thread; the device runs it
// on every lane of a wave with the same values (uni() tells the compiler so), shares the table fills among the lanes
// and orders them with sync().
struct HostPolicy {
  MH_INF_HD int lane() const { return 0; }
  MH_INF_HD int lanes() const { return 1; }
  MH_INF_HD uint32_t uni(uint32_t v) const { return v; }
  MH_INF_HD void sync() const {}
};

// Output of the host: a plain buffer of ISIZE bytes.
struct HostOut {
  uint8_t *out;
  MH_INF_HD void lit(uint32_t pos, uint8_t b) { out[pos] = b; }
  MH_INF_HD void copy(uint32_t pos, uint32_t dist, uint32_t len) {   // byte-serial: dist < len repeats the pattern
    for (uint32_t i = 0; i < len; i++) out[pos + i] = out[pos - dist + i];
  }
  MH_INF_HD void store(uint32_t pos, const uint8_t *src, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) out[pos + i] = src[i];
  }
};

MH_INF_HD inline uint32_t bit_reverse(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; i++) {
    r = (r << 1) | (code & 1u);
    code >>= 1;
  }
  return r;
}

// Canonical Huffman decode tables from n code lengths (0..15).  Returns -1 when the lengths are over-subscribed, else
// the unused code space in units of 2^-15 (0: complete); *max_len is the longest length (0: no code at all).
template <class P>
MH_INF_HD inline int build_table(const uint8_t *lens, int n, uint16_t *count, uint16_t *sym, uint16_t *offs,
                                 uint16_t *fast, int fbits, int *max_len, P &pol) {
  pol.sync();   // (the lanes' reads of the previous block's tables are done)
  for (int l = 0; l < 16; l++) count[l] = 0;
  for (int s = 0; s < n; s++) {
    const uint32_t l = pol.uni(lens[s]) & 15u;
    count[l] = (uint16_t)(count[l] + 1);
  }
  int mx = 0, left = 1;
  for (int l = 1; l < 16; l++) {
    const int c = (int)pol.uni(count[l]);
    if (c) mx = l;
    left = (left << 1) - c;
    if (left < 0) return -1;
  }
  *max_len = mx;
  // start[l]: where the symbols of length l begin in sym (sorted by length, then symbol); first[l]: their first code
  uint16_t *start = offs + 16, *first = offs + 32;
  uint32_t code = 0, idx = 0;
  for (int l = 1; l < 16; l++) {
    const uint32_t c = pol.uni(count[l]);
    offs[l] = start[l] = (uint16_t)idx;
    first[l] = (uint16_t)code;
    idx += c;
    code = (code + c) << 1;   // (< 2^16: the lengths are not over-subscribed)
  }
  for (int s = 0; s < n; s++) {
    const uint32_t l = pol.uni(lens[s]) & 15u;
    if (l) {
      const uint32_t o = pol.uni(offs[l]);   // < n: the counts sum to at most n
      sym[o] = (uint16_t)s;
      offs[l] = (uint16_t)(o + 1);
    }
  }
  const int fsize = 1 << fbits;
  for (int j = pol.lane(); j < fsize; j += pol.lanes()) fast[j] = 0;
  pol.sync();
  // first-level entries of the codes that fit, a symbol per lane at a time
  const int top = mx < fbits ? mx : fbits;
  const int nfast = top ? (int)pol.uni(start[top]) + (int)pol.uni(count[top]) : 0;
  for (int i = pol.lane(); i < nfast; i += pol.lanes()) {
    const uint32_t s = sym[i], l = lens[s] & 15u;   // 1 <= l <= top
    const uint16_t e = (uint16_t)(s | l << 9);
    for (int j = (int)bit_reverse((uint32_t)first[l] + ((uint32_t)i - start[l]), (int)l); j < fsize; j += 1 << l)
      fast[j] = e;
  }
  pol.sync();
  return left;
}

// The next symbol of a code, or -1 (no such code, or the input ends inside it).
template <class S, class P>
MH_INF_HD inline int decode_symbol(BitReader<S> &br, const uint16_t *fast, int fbits, const uint16_t *count,
                                   const uint16_t *sym, P &pol) {
  const uint32_t e = pol.uni(fast[br.peek(fbits)]);
  if (e) {
    const int l = (int)(e >> 9);
    if (br.cnt < l) return -1;
    br.drop(l);
    return (int)(e & 511u);
  }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l < 16; l++) {
    if (br.cnt < l) return -1;
    code |= (int)((br.buf >> (l - 1)) & 1u);
    const int c = (int)pol.uni(count[l]);
    if (code - c < first) {
      br.drop(l);
      return (int)pol.uni(sym[index + (code - first)]);
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// zlib's rule for a table that build_table found incomplete (inflate_table: `left > 0 && (type == CODES || max != 1)`).
MH_INF_HD inline bool table_ok(int left, int max_len, bool is_code_lengths) {
  if (left < 0) return false;
  if (left > 0 && max_len != 0 && (is_code_lengths || max_len != 1)) return false;
  return true;
}

// Inflates the raw deflate stream in[0, n), read through src (stored blocks are copied from `in` itself), into at most
// isize bytes through `out`.  *produced: the bytes written.
template <class S, class Out, class P>
MH_INF_HD inline int32_t inflate_raw(S &src, const uint8_t *in, int64_t n, uint32_t isize, Out &out, Tables &T, P &pol,
                                     uint32_t *produced) {
  BitReader<S> br{src, n, 0, 0, 0};
  uint32_t pos = 0;
  int kind = 0;   // the tables at hand: 1 fixed, 2 dynamic
  *produced = 0;
  for (;;) {   // a deflate block: at least 3 bits of input each
    br.refill();
    if (br.cnt < 3) return ST_BAD_STREAM;
    const uint32_t final = br.take(1), type = br.take(2);
    if (type == 0) {
      br.drop(br.cnt & 7);
      br.refill();
      if (br.cnt < 32) return ST_BAD_STREAM;
      const uint32_t len = br.take(16), nlen = br.take(16);
      if (len != (~nlen & 0xffffu)) return ST_BAD_STREAM;
      br.pos -= br.cnt >> 3;   // the whole bytes still in the buffer
      br.buf = 0;
      br.cnt = 0;
      if (br.n - br.pos < (int64_t)len) return ST_BAD_STREAM;
      if (isize - pos < len) return ST_LENGTH;
      out.store(pos, in + br.pos, len);
      pos += len;
      br.pos += len;
    } else if (type == 3) {
      return ST_BAD_STREAM;
    } else {
      if (type == 1) {
        if (kind != 1) {
          for (int s = 0; s < NLIT; s++) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
          for (int s = 0; s < NDIST; s++) T.lens[NLIT + s] = 5;
          int mx;
          build_table(T.lens, NLIT, T.lcount, T.lsym, T.offs, T.lfast, FAST_L, &mx, pol);
          build_table(T.lens + NLIT, NDIST, T.dcount, T.dsym, T.offs, T.dfast, FAST_D, &mx, pol);
          kind = 1;
        }
      } else {
        kind = 0;
        if (br.cnt < 14) return ST_BAD_STREAM;
        const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncode = (int)br.take(4) + 4;
        if (nlen > 286 || ndist > 30) return ST_BAD_STREAM;
        for (int i = 0; i < NCL; i++) T.lens[i] = 0;
        for (int i = 0; i < ncode; i++) {
          br.refill();
          if (br.cnt < 3) return ST_BAD_STREAM;
          T.lens[cl_order(i)] = (uint8_t)br.take(3);
        }
        int mx = 0;
        int left = build_table(T.lens, NCL, T.ccount, T.csym, T.offs, T.cfast, FAST_C, &mx, pol);
        if (!table_ok(left, mx, true)) return ST_BAD_STREAM;
        const int total = nlen + ndist;
        int have = 0;
        while (have < total) {   // each turn consumes at least one bit
          br.refill();
          const int s = decode_symbol(br, T.cfast, FAST_C, T.ccount, T.csym, pol);
          if (s < 0) return ST_BAD_STREAM;
          if (s < 16) {
            T.lens[have++] = (uint8_t)s;
            continue;
          }
          uint8_t prev = 0;
          int rep;
          if (s == 16) {
            if (have == 0 || br.cnt < 2) return ST_BAD_STREAM;
            prev = (uint8_t)pol.uni(T.lens[have - 1]);
            rep = 3 + (int)br.take(2);
          } else if (s == 17) {
            if (br.cnt < 3) return ST_BAD_STREAM;
            rep = 3 + (int)br.take(3);
          } else {
            if (br.cnt < 7) return ST_BAD_STREAM;
            rep = 11 + (int)br.take(7);
          }
          if (have + rep > total) return ST_BAD_STREAM;
          while (rep-- > 0) T.lens[have++] = prev;
        }
        if (pol.uni(T.lens[256]) == 0) return ST_BAD_STREAM;   // no end-of-block code
        left = build_table(T.lens, nlen, T.lcount, T.lsym, T.offs, T.lfast, FAST_L, &mx, pol);
        if (!table_ok(left, mx, false)) return ST_BAD_STREAM;
        left = build_table(T.lens + nlen, ndist, T.dcount, T.dsym, T.offs, T.dfast, FAST_D, &mx, pol);
        if (!table_ok(left, mx, false)) return ST_BAD_STREAM;
        kind = 2;
      }
      for (;;) {   // a symbol: at least one bit of input each
        br.refill();
        int s = decode_symbol(br, T.lfast, FAST_L, T.lcount, T.lsym, pol);
        if (s < 0) return ST_BAD_STREAM;
        if (s < 256) {
          if (pos >= isize) return ST_LENGTH;
          out.lit(pos++, (uint8_t)s);
          continue;
        }
        if (s == 256) break;
        s -= 257;
        if (s >= 29) return ST_BAD_STREAM;   // symbols 286, 287
        const int lx = len_extra(s);
        if (br.cnt < lx) return ST_BAD_STREAM;
        const uint32_t len = (uint32_t)len_base(s) + br.take(lx);
        const int d = decode_symbol(br, T.dfast, FAST_D, T.dcount, T.dsym, pol);
        if (d < 0 || d >= 30) return ST_BAD_STREAM;
        const int dx = dist_extra(d);
        if (br.cnt < dx) return ST_BAD_STREAM;
        const uint32_t dist = (uint32_t)dist_base(d) + br.take(dx);
        if (dist > pos) return ST_BAD_STREAM;   // before the member's first byte: BGZF has no preset dictionary
        if (isize - pos < len) return ST_LENGTH;
        out.copy(pos, dist, len);
        pos += len;
      }
    }
    if (final) break;
  }
  *produced = pos;
  return pos == isize ? ST_OK : ST_LENGTH;
}

// ---- CRC-32 (RFC 1952, reflected polynomial) -------------------------------------------------------------------------
constexpr uint32_t CRC_POLY = 0xedb88320u;

MH_INF_HD constexpr inline uint32_t crc_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ CRC_POLY : c >> 1;
  return c;
}
// a * b modulo the polynomial (reflected bit order)
MH_INF_HD constexpr inline uint32_t crc_multmodp(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1)) == 0) break;
    }
    b = b & 1 ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}
// The raw CRC register (starting at 0, no inversion) is linear, so a buffer's raw CRC is the XOR of its slices' raw
// CRCs, each multiplied by x^(8 * bytes after the slice).  With slices of CRC_SEG bytes and n = q CRC_SEG + r, whole
// slice i < q takes x^(8 CRC_SEG (q - 1 - i)) and then, all together, x^(8 r); the partial slice takes nothing; and
// crc32 = ~(raw ^ 0xffffffff * x^(8 n)).  CRC_SEG = 132 (33 words): lanes' reads at that stride fall in different
// LDS banks.
constexpr int CRC_SEG = 132;
constexpr int CRC_NSEG = (MAX_ISIZE + CRC_SEG - 1) / CRC_SEG;   // 497
struct CrcPowers {
  uint32_t seg[CRC_NSEG + 1];   // x^(8 CRC_SEG j)
  uint32_t byte[CRC_SEG];       // x^(8 r)
};
constexpr CrcPowers make_crc_powers() {
  CrcPowers t{};
  uint32_t p = 1u << 31;   // x^0
  for (int r = 0; r < CRC_SEG; r++) {
    t.byte[r] = p;
    p = crc_multmodp(1u << 23, p);   // * x^8
  }
  uint32_t q = 1u << 31;
  for (int j = 0; j <= CRC_NSEG; j++) {
    t.seg[j] = q;
    q = crc_multmodp(p, q);
  }
  return t;
}
MH_INF_HD inline uint32_t crc_raw(const uint8_t *b, int a, int e, const uint32_t *tab) {
  uint32_t c = 0;
  for (int k = a; k < e; k++) c = tab[(c ^ b[k]) & 0xffu] ^ (c >> 8);
  return c;
}
// crc32 of b[0, n) by the slice method, the slices shared among `lanes` (the device's lanes XOR their acc together)
MH_INF_HD inline void crc_slices(const uint8_t *b, int n, const CrcPowers &P, const uint32_t *tab, int lane, int lanes,
                                 uint32_t *acc, uint32_t *tail) {
  const int q = n / CRC_SEG;
  uint32_t a = 0, t = 0;
  for (int i = lane; i * CRC_SEG < n; i += lanes) {
    const int s = i * CRC_SEG, e = s + CRC_SEG < n ? s + CRC_SEG : n;
    const uint32_t c = crc_raw(b, s, e, tab);
    if (i < q) a ^= crc_multmodp(P.seg[q - 1 - i], c);
    else t = c;
  }
  *acc = a;
  *tail = t;
}
MH_INF_HD inline uint32_t crc_finish(uint32_t acc, uint32_t tail, int n, const CrcPowers &P) {
  const int q = n / CRC_SEG, r = n - q * CRC_SEG;
  const uint32_t raw = crc_multmodp(P.byte[r], acc) ^ tail;
  return ~(crc_multmodp(crc_multmodp(P.seg[q], P.byte[r]), 0xffffffffu) ^ raw);
}

}  // namespace inf

// ---- the inflater as mh_bamread.cpp sees it (plain C++; implemented in mh_inflate.hip) -------------------------------
// One member of a batch: its deflate payload in the caller's compressed bytes and its place in the caller's output.
struct InflateMember {
  int64_t src;      // payload offset from `base`
  int64_t dst;      // output offset from `out`
  uint32_t clen;    // payload bytes
  uint32_t isize;   // <= 65536
  uint32_t crc;
  uint32_t status;  // out: inf::ST_*
};

// mh_bamread.cpp is also built without the HIP half of the library (its sanitizer test links it alone): it defines
// MH_INFLATE_OPTIONAL, the three functions are then weak references, and mh_bamfile_open_gpu fails cleanly when they
// are absent.
#ifdef MH_INFLATE_OPTIONAL
#define MH_INF_WEAK __attribute__((weak))
#else
#define MH_INF_WEAK
#endif

// A device inflater: one stream, two page-locked staging buffers and its device buffers, all grown on demand.  It
// uses no mh_ctx and calls hipSetDevice in whichever thread runs it; one thread uses it at a time.
class Inflater;
MH_INF_WEAK int32_t inflater_create(int device, Inflater **out, std::string *err);   // MH_OK, or MH_E_* with *err
MH_INF_WEAK void inflater_destroy(Inflater *);
// Inflates m[0, n): payloads at base + m[k].src, results at out + m[k].dst (out_bytes in all), m[k].status filled.
// The copies into and out of the page-locked buffers are shared among `threads` host threads.
// MH_OK when the launch ran (statuses say what each member did), MH_E_HIP / MH_E_OOM with *err otherwise.
MH_INF_WEAK int32_t inflater_run(Inflater *, const uint8_t *base, InflateMember *m, size_t n, uint8_t *out,
                                 int64_t out_bytes, int threads, std::string *err);

}  // namespace mh
