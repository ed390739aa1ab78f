// Host check of the single-thread parts of the device BGZF compressor (mitty_amd/csrc/mh_deflate.h: Huffman code
// lengths, canonical codes, the dynamic block header, CRC-32 combination).  Test infrastructure: compresses a file
// into BGZF with a sequential restatement of mh_deflate.hip's parse (256-position steps, hash of earlier steps, run
// candidate, MIN_MATCH-byte matches, every match a step's positions start, eight slices per block with sync flushes)
// and the shared header code; tests/test_deflate_cpu.py then inflates the output with Python's zlib.
//   deflate_host IN OUT                  exit 3 when a block's codes do not fit a BGZF block (stderr: "steps N")
//   deflate_host --device-rules IN OUT   k_bgzf_blocks' "store instead" rule and k_bgzf_pack's stored block, so the
//                                        output is what the device writes, byte for byte (tests/test_gpu_deflate.py);
//                                        stderr: one JSON line describing the parse (see Report)
//   deflate_host --fuzz-huffman N SEED   huffman_from_sorted on N random frequency sets per limit (15, 7) and family
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../mitty_amd/csrc/mh_deflate.h"

using namespace mh::df;

namespace {

constexpr int WAVES = 8, SLICE = (BLOCK + WAVES - 1) / WAVES, HB = 11;
// --device-rules restates three constants of mh_deflate.hip (not included here: it is device code):
constexpr int DEV_REGION = 9216;      // REGION: a slice's bytes in the block's slot; flush_bits stores the block when
                                      // (bits written >> 3) + 8 exceeds it
constexpr int DEV_STORED_HDR = 5;     // k_bgzf_pack's stored block: 01, LEN, ~LEN (the `tot >= 5 + n` rule)
constexpr int DEV_STAGE_WORD = 32;    // stage_or's staging words: a code at bit offset r lands in words r / 32 ...

uint32_t load4(const uint8_t *b, int x) { return b[x] | b[x + 1] << 8 | b[x + 2] << 16 | (uint32_t)b[x + 3] << 24; }
uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - HB); }

struct Tok {
  int lit;          // >= 0: a literal byte
  int len, dist;    // else a match
  int step;         // the parse step that took it
};

int g_steps = 0;   // parse steps (the device's cost unit), reported on stderr

// What --device-rules reports (one JSON line on stderr), all of it from this restatement alone, so a test can assert
// that its input has the shape it claims.  Counts are sums and sets are unions over the slices of the deflated
// blocks (a stored block's slices are parsed by the device too, but none of their codes reach the output); max_*
// are maxima over those slices.
struct Report {
  long blocks = 0, stored = 0, slices = 0, steps = 0, matches = 0;
  std::set<int> len_codes, dist_codes;
  std::map<int, std::pair<int, int>> len_x, dist_x;   // code with extra bits -> (min, max) extra value
  int max_lit_syms = 0, max_dist_syms = 0;            // used symbols of one slice
  long fold_lit = 0, fold_dist = 0, fold_cl = 0;      // slices whose unlimited Huffman depth exceeds 15, 15, 7
  int max_depth_lit = 0, max_depth_dist = 0, max_depth_cl = 0;   // the deepest unlimited code seen
  int max_token_bits = 0;
  long third_word_tokens = 0;   // tokens with (bit offset in the slice's stream mod 32) + bits > 64
  long third_word_set = 0;      // ... of which those with a 1 among the bits past the second word (stage_or's hi2)
  int max_step_span = 0, max_step_bits = 0, max_header_bits = 0;
  void merge(const Report &o) {
    slices += o.slices, steps += o.steps, matches += o.matches;
    len_codes.insert(o.len_codes.begin(), o.len_codes.end());
    dist_codes.insert(o.dist_codes.begin(), o.dist_codes.end());
    for (auto *pr : {&len_x, &dist_x}) {
      const auto &src = pr == &len_x ? o.len_x : o.dist_x;
      for (const auto &kv : src) {
        auto it = pr->find(kv.first);
        if (it == pr->end()) (*pr)[kv.first] = kv.second;
        else {
          it->second.first = std::min(it->second.first, kv.second.first);
          it->second.second = std::max(it->second.second, kv.second.second);
        }
      }
    }
    max_lit_syms = std::max(max_lit_syms, o.max_lit_syms), max_dist_syms = std::max(max_dist_syms, o.max_dist_syms);
    fold_lit += o.fold_lit, fold_dist += o.fold_dist, fold_cl += o.fold_cl;
    max_depth_lit = std::max(max_depth_lit, o.max_depth_lit);
    max_depth_dist = std::max(max_depth_dist, o.max_depth_dist);
    max_depth_cl = std::max(max_depth_cl, o.max_depth_cl);
    max_token_bits = std::max(max_token_bits, o.max_token_bits);
    third_word_tokens += o.third_word_tokens;
    third_word_set += o.third_word_set;
    max_step_span = std::max(max_step_span, o.max_step_span);
    max_step_bits = std::max(max_step_bits, o.max_step_bits);
    max_header_bits = std::max(max_header_bits, o.max_header_bits);
  }
  static void note(std::map<int, std::pair<int, int>> &m, int code, int x) {
    auto it = m.find(code);
    if (it == m.end()) m[code] = {x, x};
    else it->second = {std::min(it->second.first, x), std::max(it->second.second, x)};
  }
  void print(FILE *f) const {
    auto set_json = [&](const std::set<int> &s) {
      std::string r = "[";
      for (int v : s) r += (r.size() > 1 ? "," : "") + std::to_string(v);
      return r + "]";
    };
    auto map_json = [&](const std::map<int, std::pair<int, int>> &m) {
      std::string r = "{";
      for (const auto &kv : m)
        r += std::string(r.size() > 1 ? "," : "") + "\"" + std::to_string(kv.first) + "\":[" +
             std::to_string(kv.second.first) + "," + std::to_string(kv.second.second) + "]";
      return r + "}";
    };
    fprintf(f,
            "{\"blocks\":%ld,\"stored_blocks\":%ld,\"slices\":%ld,\"steps\":%ld,\"matches\":%ld,\"len_codes\":%s,"
            "\"dist_codes\":%s,\"len_extra\":%s,\"dist_extra\":%s,\"max_lit_syms\":%d,\"max_dist_syms\":%d,"
            "\"fold_lit\":%ld,\"fold_dist\":%ld,\"fold_cl\":%ld,\"max_depth_lit\":%d,\"max_depth_dist\":%d,"
            "\"max_depth_cl\":%d,\"max_token_bits\":%d,\"third_word_tokens\":%ld,\"third_word_set\":%ld,"
            "\"max_step_span\":%d,"
            "\"max_step_bits\":%d,\"max_header_bits\":%d}\n",
            blocks, stored, slices, steps, matches, set_json(len_codes).c_str(), set_json(dist_codes).c_str(),
            map_json(len_x).c_str(), map_json(dist_x).c_str(), max_lit_syms, max_dist_syms, fold_lit, fold_dist,
            fold_cl, max_depth_lit, max_depth_dist, max_depth_cl, max_token_bits, third_word_tokens, third_word_set,
            max_step_span,
            max_step_bits, max_header_bits);
  }
};

// mh_deflate.hip's parse: one step covers SW = DF_NP x 64 positions; every position's candidate from the table as it
// was at the step's start (or the run at distance 1); a greedy walk takes the step's matches in order (literals
// between), each extended to its end
std::vector<Tok> parse(const uint8_t *s, int S, std::vector<int> *spans = nullptr) {
  const int SW = getenv("DF_SW") ? atoi(getenv("DF_SW")) : 256;   // positions per step (mh_deflate.hip DF_NP x 64)
  std::vector<uint32_t> ht(1 << HB, 0);
  std::vector<Tok> out;
  std::vector<int> cand(SW);
  int step = 0;
  for (int cur = 0; cur < S; step++) {
    g_steps++;
    const int W = S - cur < SW ? S - cur : SW;
    for (int l = 0; l < SW; l++) {
      const int p = cur + l;
      cand[l] = -1;
      if (l >= W || p + MIN_MATCH > S) continue;
      const uint32_t w = load4(s, p);
      auto match = [&](int c) { return std::memcmp(s + p, s + c, MIN_MATCH) == 0; };
      if (p >= 1 && match(p - 1)) {
        cand[l] = p - 1;
      } else {
        const int c = (int)ht[hash4(w)] - 1;
        if (c >= 0 && match(c)) cand[l] = c;
      }
    }
    int x = 0, next = cur + W;
    while (x < W) {
      int m = x;
      while (m < W && cand[m] < 0) m++;
      for (int l = x; l < m; l++) out.push_back({s[cur + l], 0, 0, step});
      if (m >= W) {
        next = cur + W;
        break;
      }
      const int q = cur + m, j = cand[m], cap = S - q < MAX_MATCH ? S - q : MAX_MATCH;
      int L = MIN_MATCH;
      while (L < cap && s[q + L] == s[j + L]) L++;
      out.push_back({-1, L, q - j, step});
      x = m + L;
      next = cur + x;
    }
    for (int k = cur; k < next; k++)
      if (k + HASH_BYTES <= S) {
        uint32_t &e = ht[hash4(load4(s, k))];
        if ((uint32_t)(k + 1) > e) e = (uint32_t)(k + 1);
      }
    if (spans) spans->push_back(next - cur);
    cur = next;
  }
  return out;
}

// the deepest code of the unlimited Huffman tree over f's used symbols (huffman_from_sorted with limit 31)
int unlimited_depth(const uint32_t *f, int n) {
  std::vector<uint32_t> keys, A(NLIT);
  std::vector<uint8_t> len(512, 0);
  for (int s = 0; s < n; s++)
    if (f[s]) keys.push_back((f[s] << 9) | (uint32_t)s);
  std::sort(keys.begin(), keys.end());
  int32_t count[32];
  huffman_from_sorted(keys.data(), (int)keys.size(), 31, len.data(), A.data(), count);
  int d = 0;
  for (int s = 0; s < n; s++) d = std::max(d, (int)len[s]);
  return d;
}

void codes(const uint32_t *f, int n, int limit, uint8_t *len, uint16_t *code) {
  std::vector<uint32_t> keys, A(NLIT);
  for (int s = 0; s < n; s++) {
    len[s] = 0;
    if (f[s]) keys.push_back((f[s] << 9) | (uint32_t)s);
  }
  std::sort(keys.begin(), keys.end());
  int32_t count[32], next[16];
  huffman_from_sorted(keys.data(), (int)keys.size(), limit, len, A.data(), count);
  canonical_codes(len, n, code, count, next);
}

// one slice as a deflate block (final or followed by a sync flush); returns its bytes.  rep: the slice's shape is
// added to it
std::string slice_bits(const uint8_t *s, int S, bool last, Report *rep = nullptr) {
  std::vector<int> spans;
  const std::vector<Tok> t = parse(s, S, &spans);
  uint32_t lf[NLIT] = {0}, dfq[NDIST] = {0};
  for (const Tok &k : t) {
    if (k.lit >= 0) lf[k.lit]++;
    else {
      lf[257 + len_code(k.len)]++;
      dfq[dist_code(k.dist)]++;
    }
  }
  lf[256] = 1;
  uint8_t llen[NLIT], dlen[NDIST];
  uint16_t lcode[NLIT], dcode[NDIST];
  codes(lf, NLIT, 15, llen, lcode);
  codes(dfq, NDIST, 15, dlen, dcode);
  std::vector<uint8_t> buf(4 * S + 4096, 0);
  BitSink bs{buf.data(), 0, 0, 0};
  bs.put(last ? 1u : 0u, 1);
  bs.put(2u, 2);
  HeaderScratch H;
  write_dynamic_header(bs, llen, dlen, H);
  const int64_t hbits = bs.pos * 8 + bs.nacc;
  std::vector<int> step_bits(spans.size(), 0);
  for (const Tok &k : t) {
    const int64_t at = bs.pos * 8 + bs.nacc;
    if (k.lit >= 0) {
      bs.put(lcode[k.lit], llen[k.lit]);
    } else {
      const int lc = len_code(k.len), dc = dist_code(k.dist);
      bs.put(lcode[257 + lc], llen[257 + lc]);
      bs.put((uint32_t)(k.len - len_base(lc)), len_extra(lc));
      bs.put(dcode[dc], dlen[dc]);
      bs.put((uint32_t)(k.dist - dist_base(dc)), dist_extra(dc));
      if (rep) {
        rep->matches++;
        rep->len_codes.insert(lc);
        rep->dist_codes.insert(dc);
        if (len_extra(lc)) Report::note(rep->len_x, lc, k.len - len_base(lc));
        if (dist_extra(dc)) Report::note(rep->dist_x, dc, k.dist - dist_base(dc));
      }
    }
    if (rep) {
      const int bits = (int)(bs.pos * 8 + bs.nacc - at);
      rep->max_token_bits = std::max(rep->max_token_bits, bits);
      const int sh = (int)(at % DEV_STAGE_WORD);
      if (sh + bits > 2 * DEV_STAGE_WORD) {
        rep->third_word_tokens++;
        uint64_t top = 0;   // the token's bits from 2 * DEV_STAGE_WORD - sh on, read back from the stream
        for (int64_t i = at + 2 * DEV_STAGE_WORD - sh; i < at + bits; i++)
          top |= i < bs.pos * 8 ? (uint64_t)((buf[i >> 3] >> (i & 7)) & 1) : (bs.acc >> (i - bs.pos * 8)) & 1;
        if (top) rep->third_word_set++;
      }
      step_bits[k.step] += bits;
    }
  }
  bs.put(lcode[256], llen[256]);
  if (!last) {
    bs.put(0, 3);
    if (bs.nacc) bs.put(0, 8 - bs.nacc);
    bs.put(0xffff0000u, 32);
  }
  if (bs.nacc) bs.put(0, 8 - bs.nacc);
  if (rep) {
    rep->slices++;
    rep->steps += (long)spans.size();
    int nl = 0, nd = 0;
    for (int i = 0; i < NLIT; i++) nl += lf[i] != 0;
    for (int i = 0; i < NDIST; i++) nd += dfq[i] != 0;
    rep->max_lit_syms = std::max(rep->max_lit_syms, nl);
    rep->max_dist_syms = std::max(rep->max_dist_syms, nd);
    const int dl = unlimited_depth(lf, NLIT), dd = unlimited_depth(dfq, NDIST), dc = unlimited_depth(H.cf, NCL);
    rep->fold_lit += dl > 15, rep->fold_dist += dd > 15, rep->fold_cl += dc > 7;
    rep->max_depth_lit = std::max(rep->max_depth_lit, dl);
    rep->max_depth_dist = std::max(rep->max_depth_dist, dd);
    rep->max_depth_cl = std::max(rep->max_depth_cl, dc);
    for (int v : spans) rep->max_step_span = std::max(rep->max_step_span, v);
    for (int v : step_bits) rep->max_step_bits = std::max(rep->max_step_bits, v);
    rep->max_header_bits = std::max(rep->max_header_bits, (int)hbits);
  }
  return std::string((const char *)buf.data(), (size_t)bs.pos);
}

uint32_t crc_bytes(const uint8_t *p, int64_t n) {
  uint32_t c = 0xffffffffu;
  for (int64_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ CRC_POLY : c >> 1;
  }
  return ~c;
}

// ---- --fuzz-huffman: huffman_from_sorted against its own unlimited result -------------------------------------------
struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

// One frequency set of family fam (0 random, 1 Fibonacci, 2 near-flat, 3 powers of two) over an alphabet of `syms`
// symbols, m of them used; checks the lengths for `limit`.  Returns 0, or a failure code; *folded: the limit bound.
int fuzz_one(Rng &R, int fam, int limit, int *folded) {
  const int syms = limit == 7 ? NCL : NLIT;
  const int maxm = limit == 7 ? NCL : (fam == 1 ? 34 : (fam == 3 ? 22 : NLIT));   // (frequencies stay below 2^23)
  const int m = 2 + (int)R.below((uint32_t)(maxm - 1));
  std::vector<int> sym(syms);
  for (int i = 0; i < syms; i++) sym[i] = i;
  for (int i = syms - 1; i > 0; i--) std::swap(sym[i], sym[R.below((uint32_t)i + 1)]);
  std::vector<uint32_t> f(syms, 0);
  uint32_t a = 1, b = 1;
  for (int i = 0; i < m; i++) {
    uint32_t v;
    if (fam == 0) v = 1 + R.below(R.below(2) ? 20u : 5000u);
    else if (fam == 1) {
      v = a;
      const uint32_t c = a + b;
      a = b, b = c;
    } else if (fam == 2) v = 1000 + R.below(3);
    else v = 1u << i;
    f[sym[i]] = v;
  }
  std::vector<uint32_t> keys, A(NLIT);
  for (int s = 0; s < syms; s++)
    if (f[s]) keys.push_back((f[s] << 9) | (uint32_t)s);
  std::sort(keys.begin(), keys.end());
  std::vector<uint8_t> len(512, 0), un(512, 0);
  int32_t count[32];
  huffman_from_sorted(keys.data(), m, limit, len.data(), A.data(), count);
  huffman_from_sorted(keys.data(), m, 31, un.data(), A.data(), count);
  uint64_t kraft = 0;   // in units of 2^-31
  int deepest = 0;
  for (int s = 0; s < syms; s++) {
    if (!f[s]) {
      if (len[s]) return 1;   // an unused symbol with a code
      continue;
    }
    if (len[s] < 1 || len[s] > limit) return 2;
    kraft += 1ull << (31 - len[s]);
    deepest = std::max(deepest, (int)un[s]);
  }
  if (kraft != 1ull << 31) return 3;
  for (int i = 1; i < m; i++)   // a more frequent symbol never has the longer code
    if ((keys[i] >> 9) > (keys[i - 1] >> 9) && len[keys[i] & 511u] > len[keys[i - 1] & 511u]) return 4;
  if (deepest <= limit) {
    for (int s = 0; s < syms; s++)
      if (len[s] != un[s]) return 5;   // the limit changed a tree that fitted
  } else {
    ++*folded;
  }
  return 0;
}

int fuzz_huffman(long n, uint64_t seed) {
  Rng R{seed};
  for (int limit : {15, 7}) {
    int folded = 0;
    for (int fam = 0; fam < 4; fam++)
      for (long i = 0; i < n; i++) {
        const int rc = fuzz_one(R, fam, limit, &folded);
        if (rc) {
          fprintf(stderr, "huffman fuzz: limit %d family %d case %ld: failure %d\n", limit, fam, i, rc);
          return 1;
        }
      }
    fprintf(stderr, "huffman fuzz: limit %d: %ld cases, %d folded\n", limit, 4 * n, folded);
    if (!folded) return 1;   // the fuzz must reach the limiter
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "--fuzz-huffman")) return fuzz_huffman(atol(argv[2]), strtoull(argv[3], 0, 10));
  const bool dev = argc == 4 && !strcmp(argv[1], "--device-rules");
  if (argc != 3 && !dev) return 2;
  if (dev) argv++;
  FILE *fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  std::vector<uint8_t> in;
  uint8_t tmp[1 << 16];
  size_t r;
  while ((r = fread(tmp, 1, sizeof(tmp), fi)) > 0) in.insert(in.end(), tmp, tmp + r);
  fclose(fi);
  in.resize(in.size() + 8, 0);   // (load4 reads past the end)
  const int64_t n = (int64_t)in.size() - 8;
  std::string out;
  Report rep;
  for (int64_t b = 0; b * BLOCK < n; b++) {
    const uint8_t *blk = in.data() + b * BLOCK;
    const int bn = (int)(n - b * BLOCK < BLOCK ? n - b * BLOCK : BLOCK);
    std::string z;
    Report brep;
    bool region_over = false;
    for (int w = 0; w < WAVES; w++) {
      const int s0 = w * SLICE;
      if (s0 >= bn) break;
      const int S = bn - s0 < SLICE ? bn - s0 : SLICE;
      const std::string zs = slice_bits(blk + s0, S, s0 + SLICE >= bn, dev ? &brep : nullptr);
      // flush_bits' check, at the slice's last flush (the bit position only grows): bytes + 8 > REGION
      if ((int64_t)zs.size() + 8 > DEV_REGION) region_over = true;
      z += zs;
    }
    // CRC by segments (the device's method) must equal the direct CRC; so must the combination of two halves
    static const CrcPowers P = make_crc_powers();
    static uint32_t tab[256];
    if (!tab[1])
      for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ CRC_POLY : c >> 1;
        tab[i] = c;
      }
    const uint32_t c = crc32_segments(blk, bn, P, tab);
    const int half = bn / 2;
    if (c != crc_bytes(blk, bn) ||
        crc_combine(crc_bytes(blk, half), crc_bytes(blk + half, bn - half), (uint64_t)(bn - half)) != c) {
      fprintf(stderr, "crc combine mismatch in block %lld\n", (long long)b);
      return 1;
    }
    rep.blocks++;
    if (dev) {
      // k_bgzf_blocks' decision (I.stored) and k_bgzf_pack's stored block
      const int64_t tot = (int64_t)z.size();
      if (region_over || HDR + tot + TRL > MAX_BSIZE || tot >= DEV_STORED_HDR + (int64_t)bn) {
        const uint8_t sh[5] = {1, (uint8_t)bn, (uint8_t)(bn >> 8), (uint8_t)~bn, (uint8_t)(~bn >> 8)};
        z.assign((const char *)sh, 5);
        z.append((const char *)blk, (size_t)bn);
        rep.stored++;
      } else {
        rep.merge(brep);
      }
    }
    const int64_t bsize = HDR + (int64_t)z.size() + TRL;
    if (bsize > MAX_BSIZE) {
      fprintf(stderr, "block %lld: %lld bytes compressed (stored on the device)\n", (long long)b, (long long)bsize);
      return 3;
    }
    const uint8_t h[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                           (uint8_t)((bsize - 1) & 0xff), (uint8_t)((bsize - 1) >> 8)};
    out.append((const char *)h, 18);
    out += z;
    const uint8_t t[8] = {(uint8_t)c, (uint8_t)(c >> 8), (uint8_t)(c >> 16), (uint8_t)(c >> 24),
                          (uint8_t)bn, (uint8_t)(bn >> 8), (uint8_t)(bn >> 16), (uint8_t)(bn >> 24)};
    out.append((const char *)t, 8);
  }
  FILE *fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  fwrite(out.data(), 1, out.size(), fo);
  fclose(fo);
  if (dev) rep.print(stderr);
  else fprintf(stderr, "steps %d\n", g_steps);
  return 0;
}
