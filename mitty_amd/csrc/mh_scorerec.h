// mh_scorerec.h — the one device statement of a BAM record's alignment score (readgenerate.parse_qname :259-291 and
// score_alignment_error :294-319 of the reference): the heads of a tile's records staged in LDS, and the record's
// verdict (skipped, failed, or d_err with the scored group's v_list).  k_score (mh_score.hip) fills its matrices from
// it, k_filter_mark (mh_filter.hip) keeps or drops the record by it.  Included after mh_internal.h.
#pragma once

namespace mh {

constexpr int SC_ROW = 192;       // LDS bytes per record head (4 + 32 fixed bytes, then the name; up to 15 bytes of lead)
constexpr int SC_FIELDS = 13;     // rid, chrom, cpy + 2 x (strand, pos, rlen, cigar, v_list)

enum { SE_STRUCT = 1, SE_TID = 2, SE_PARSE = 3, SE_MATE = 4, SE_MAPQ = 5 };

// The texts of those kinds (a session's RecTexts::kind), by kind
inline constexpr const char *SCORE_KIND_TEXT[6] = {
    "", "record shorter than its fixed fields", "tid outside the header's references",
    "qname does not parse (readgenerate.parse_qname)", "read2 record whose qname has one read group",
    "MAPQ of 100 or more (mq_mat has 100 rows)"};

// What a record is scored against
struct ScoreRule {
  const char *names;           // header names, concatenated
  const int32_t *name_off;     // [n_refs + 1]
  int32_t n_refs;
  const uint8_t *prefix;       // sample prefix (plen 0: none)
  int32_t plen;
  int32_t max_d, strict;
};
inline ScoreRule RefNames::rule(int32_t max_d, int32_t strict) const {
  return ScoreRule{(const char *)names.p, (const int32_t *)name_off.p, n_refs, (const uint8_t *)prefix.p, plen, max_d,
                   strict};
}

// A record's verdict.  kind != 0: the record fails the session (SE_*).  Otherwise skip_tid / skip_smp: not scored
// (tid < 0; the sample prefix differs), or scored: d_err in [-max_d, max_d], and the scored group's v_list at
// q[vs, ve) with v_items items (-1 when not scored).  q: the read name (the record's bytes at 36); mapq: the record's.
struct ScoreRec {
  int32_t kind;
  int32_t skip_tid, skip_smp, scored;
  int32_t d_err, mapq;
  int32_t vs, ve, v_items;
  const uint8_t *q;
};

// int() of q[a, b): optional sign, then digits only; values saturate at 2^40.  False when it is not such a number.
__device__ __forceinline__ bool sc_int(const uint8_t *q, int a, int b, int64_t &v) {
  if (a >= b) return false;
  bool neg = false;
  if (q[a] == '-' || q[a] == '+') { neg = q[a] == '-'; a++; }
  if (a >= b) return false;
  int64_t x = 0;
  for (; a < b; a++) {
    const uint32_t d = (uint32_t)q[a] - '0';
    if (d > 9) return false;
    x = x * 10 + d;
    if (x > ((int64_t)1 << 40)) x = (int64_t)1 << 40;
  }
  v = neg ? -x : x;
  return true;
}

// [int(v) for v in v_list.split(',') if v is not '']: false when an item is not a number; *items = the list's length
__device__ __forceinline__ bool sc_vlist_ok(const uint8_t *q, int a, int b, int *items) {
  int n = 0, st = a;
  for (int i = a; i <= b; i++) {
    if (i == b || q[i] == ',') {
      if (i > st) {
        int64_t v;
        if (!sc_int(q, st, i, v)) return false;
        n++;
      }
      st = i + 1;
    }
  }
  *items = n;
  return true;
}

// The heads of the wave's 64 records (tile * 256 + 64 wave + j) into rows[256 * SC_ROW]: one 16-byte load per lane per
// record, all in flight together.  A head is staged from the 16-byte boundary at or below the record's start; nothing
// outside [recs, recs + avail) is read.  Called by every lane of the wave, between two __syncthreads.
__device__ __forceinline__ void sc_stage_heads(uint8_t *rows, const uint8_t *recs, const int64_t *roff, int64_t n,
                                               int64_t avail, int64_t tile, int wave, int lane) {
  const int64_t tw = tile * 256 + 64 * wave;
  const int64_t tl = tw + lane;
  const int64_t s0 = tl < n ? roff[tl] : 0, e0 = tl < n ? roff[tl + 1] : 0;
#pragma unroll 8
  for (int j = 0; j < 64; j++) {
    const int64_t s = __shfl(s0, j, 64), e = __shfl(e0, j, 64);
    const int64_t c0 = s & ~(int64_t)15;
    int64_t nch = (e - c0 + 15) >> 4;
    if (nch > SC_ROW / 16) nch = SC_ROW / 16;
    if (tw + j < n && e > s && s >= 0 && c0 + 16 * nch <= avail && lane < nch)
      *(uint4 *)(rows + (64 * wave + j) * SC_ROW + 16 * lane) = *(const uint4 *)(recs + c0 + 16 * lane);
  }
}

// The bytes of the thread's record [s, e) (size >= 36, inside avail): its staged row when the fixed fields and the whole
// name are in it, else the record in memory.
__device__ __forceinline__ const uint8_t *sc_head(const uint8_t *rows, const uint8_t *recs, int64_t s, int64_t e,
                                                  int64_t avail) {
  const int64_t c0 = s & ~(int64_t)15;
  int64_t nch = (e - c0 + 15) >> 4;
  if (nch > SC_ROW / 16) nch = SC_ROW / 16;
  const bool row_ok = c0 + 16 * nch <= avail;
  const int64_t rb = 16 * nch - (s - c0);   // the record's bytes in its row
  const uint8_t *lp = recs + s;
  if (row_ok && rb >= 36) {
    const uint8_t *rp = rows + threadIdx.x * SC_ROW + (s - c0);
    if (36 + (int64_t)rp[12] <= rb) lp = rp;   // a name longer than its row is read from memory
  }
  return lp;
}

// The verdict of the record at lp (`size` bytes, >= 36; every read stays inside them) with the given flag, tid and pos.
// MAPQ is reported, not judged: what a MAPQ means to the caller is the caller's.
__device__ __forceinline__ ScoreRec score_record(const uint8_t *lp, int64_t size, int32_t flag, int32_t tid,
                                                 int32_t pos, const ScoreRule &a) {
  ScoreRec r{0, 0, 0, 0, 0, (int32_t)lp[13], 0, 0, -1, lp + 36};
  int nmax = lp[12];
  if (nmax > size - 36) nmax = (int)(size - 36);
  const uint8_t *q = lp + 36;
  int nlen = 0;
  while (nlen < nmax && q[nlen] != 0) nlen++;
  bool pass = true;
  if (tid < 0) {
    r.skip_tid = 1;   // fetch(reference=SN) per @SQ never yields these
    pass = false;
  } else if (tid >= a.n_refs) {
    r.kind = SE_TID;
    pass = false;
  } else if (a.plen > 0) {   // qname.startswith(sample_name)
    bool eq = nlen >= a.plen;
    for (int k = 0; eq && k < a.plen; k++) eq = q[k] == a.prefix[k];
    if (!eq) { r.skip_smp = 1; pass = false; }
  }
  if (!pass) return r;
  int32_t kind = 0;
  // qname.split('|'): rid, chrom, cpy, then (strand, pos, rlen, cigar, v_list) per read
  int fs[SC_FIELDS], fe[SC_FIELDS];
  int nf = 0, st = 0;
  for (int i = 0; i <= nlen; i++) {
    if (i == nlen || q[i] == '|') {
      if (nf < SC_FIELDS) { fs[nf] = st; fe[nf] = i; }
      nf++;
      st = i + 1;
    }
  }
  const int ng = nf >= 3 ? (nf - 3) / 5 : 0;   // zip(d[3::5], ..., d[7::5]): whole groups only
  const int want = (flag & 0x80) ? 1 : 0;
  int64_t iv;
  if (nf < 3) kind = SE_PARSE;
  if (!kind) {   // sample, _ = rid.split(':', 1); int(cpy)
    bool colon = false;
    for (int k = fs[0]; k < fe[0]; k++) colon |= q[k] == ':';
    if (!colon || !sc_int(q, fs[2], fe[2], iv)) kind = SE_PARSE;
  }
  int items[2] = {0, 0};
  for (int g = 0; !kind && g < ng && g < 2; g++) {
    const int f = 3 + 5 * g;
    if (!sc_int(q, fs[f], fe[f], iv) || !sc_int(q, fs[f + 1], fe[f + 1], iv) ||
        !sc_int(q, fs[f + 2], fe[f + 2], iv) || fe[f + 3] <= fs[f + 3] ||
        !sc_vlist_ok(q, fs[f + 4], fe[f + 4], &items[g]))
      kind = SE_PARSE;
  }
  if (!kind && want >= ng) kind = (want == 1 && ng >= 1) ? SE_MATE : SE_PARSE;
  if (!kind) {
    const int f = 3 + 5 * want;
    int64_t rpos = 0;
    (void)sc_int(q, fs[f + 1], fe[f + 1], rpos);
    int cs = fs[f + 3], ce = fe[f + 3];
    if (q[cs] == '>') {   // '>p:nI' -> 'nI' (parse_qname: split(':')[-1])
      int k = ce;
      while (k > cs && q[k - 1] != ':') k--;
      cs = k;
    }
    // reference_name == ri.chrom, as strings
    const int32_t no = a.name_off[tid], nl = a.name_off[tid + 1] - no;
    bool same = nl == fe[1] - fs[1];
    for (int k = 0; same && k < nl; k++) same = a.names[no + k] == (char)q[fs[1] + k];
    const int64_t p1 = (int64_t)pos + 1, md = a.max_d;
    int64_t D = md;
    if (!a.strict && ce <= cs) {
      kind = SE_PARSE;   // ri.cigar[0] of an empty cigar raises
    } else if (a.strict || q[cs] == '>') {
      if (same) D = p1 - rpos > md ? md : (p1 - rpos < -md ? -md : p1 - rpos);
    } else if (same) {
      // cigar_parser.findall: (\d+)(\D); '=', 'M', 'X' are breakpoints, 'D' only advances
      int64_t cp = rpos, cnt = 0;
      bool have = false;
      for (int k = cs; k < ce; k++) {
        const uint32_t d = (uint32_t)q[k] - '0';
        if (d <= 9) {
          cnt = cnt * 10 + d;
          if (cnt > ((int64_t)1 << 40)) cnt = (int64_t)1 << 40;
          have = true;
          continue;
        }
        if (have) {
          const uint8_t op = q[k];
          if (op == '=' || op == 'M' || op == 'X') {
            const int64_t df = p1 - cp;
            if ((df < 0 ? -df : df) < (D < 0 ? -D : D)) D = df;
            cp += cnt;
          } else if (op == 'D') {
            cp += cnt;
          }
        }
        cnt = 0;
        have = false;
      }
    }
    if (!kind) {
      r.d_err = (int32_t)D;
      r.vs = fs[f + 4];
      r.ve = fe[f + 4];
      r.v_items = items[want];
      r.scored = 1;
    }
  }
  r.kind = kind;
  return r;
}

}  // namespace mh
