// mh_cov.hip — gc-cov's pass (reference mitty/empirical/gc.py:24-59 per block, :62-78 over the header's first 24
// contigs) on the device: a depth track over the visited contigs, per-block sums over the records, and the N / GC
// counts of the FASTA's blocks.
//
//   BAM records in HBM (a chunk uploaded from the host reader, or the context's own god-aligner store)
//     -> k_cov_head    thread per record: fixed fields, the CIGAR walked into the record's reference span, its class
//                  (used, or why it is skipped) and a 24-byte descriptor; the first failing record into the error word
//     -> k_cov_apply   does nothing once a record has failed; else thread per descriptor: the counts, +1 / -1 into the
//                  difference track, and per overlapped block the span sum, min pos and max end (64-bit atomics).  A
//                  record over more than two blocks has its blocks spread over the wave's lanes.
//   at result
//     -> device_scan   the difference track into the depth (a second buffer: records may still be added afterwards).
//                  Contig c owns LN_c + 1 cells and its cells sum to zero, so one unsegmented scan serves all contigs.
//     -> k_cov_covered   per block the number of positions of [a, b) with depth > 0, a wave per block (a lane per block
//                  when blocks are shorter than a wave)
//   k_cov_gc   per block of an uploaded contig the bytes 'N' and 'G' / 'C' (upper case only, as str.count), a wave per
//              block, 16-byte loads over the aligned middle of [a, b)
//
// The rule (tests/cov_util.py states it in NumPy): block k of a contig is [a, b) = [k bl, min(k bl + bl + 1, LN)); a
// used record [pos, end) belongs to the blocks with pos < b and end > a, which are k = max(0, ceil(pos / bl) - 1) ..
// min(nb - 1, (end - 1) / bl).  k_cov_apply writes only after the whole chunk has been classified (the error word is
// final for the chunk when it starts), so a chunk with a failing record, and every later chunk, leaves the session's
// sums as they were without a copy of the track.
//
// Every read stays inside [roff[i], roff[i + 1]) and inside `avail`: the CIGAR is read only after 36 + l_read_name +
// 4 n_cigar <= the record's size has been checked.  Track cells: 0 <= pos < LN and pos < end, so both cells lie in the
// contig's LN + 1.
#include <algorithm>
#include <climits>
#include <cstring>

#include "mh_device.h"
#include "mh_internal.h"
#include "mh_scan.h"

namespace mh {

const RecTexts COV_TEXTS = {
    "gc-cov", "call mh_cov_begin first", "the record store has spilled to the host (mh_bam_set_capacity): use its BAM file",
    {"", "fields do not fit the record", "tid outside the header's references", "pos outside its reference"}};

namespace {

constexpr int CV_REF = CovState::N_REF;
constexpr int CV_NCNT = 6;   // seen, used, skipped: unplaced, refID >= 24, flag, no reference span
constexpr int32_t CV_FLAG_MASK = 0x4 | 0x100 | 0x200 | 0x400;   // pysam's pileup stepper 'all'

enum { CE_STRUCT = 1, CE_TID = 2, CE_POS = 3 };
enum { CK_USED = 0, CK_UNPLACED = 2, CK_REF = 3, CK_FLAG = 4, CK_NOSPAN = 5, CK_NONE = 6 };   // a record's class

struct CovDesc {   // 24 bytes per record of the chunk
  int64_t pos, end;
  int32_t contig, kind;
};

struct CovArgs {
  const uint8_t *recs;
  const int64_t *roff;
  int64_t n, avail, base_rec, bl;
  int32_t n_refs, n_vis;
  const int64_t *ln, *cbase, *bbase;   // device: [CV_REF], [CV_REF + 1], [CV_REF + 1]
  int32_t *track;
  unsigned long long *span, *minpos, *maxend, *cnt, *err;
  CovDesc *desc;
};

__global__ void __launch_bounds__(256) k_cov_head(CovArgs a) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < a.n; t += (int64_t)gridDim.x * 256) {
    int64_t s, size;
    CovDesc d{0, 0, -1, CK_NONE};
    int32_t fail = 0;
    if (!rec_span(a.roff, t, a.avail, &s, &size)) {
      fail = CE_STRUCT;
    } else {
      const uint8_t *p = a.recs + s;
      const int32_t tid = (int32_t)le32(p + 4), flag = (int32_t)le16(p + 18);
      if (tid < 0) {
        d.kind = CK_UNPLACED;   // pileup(region=SN:..) never yields these
      } else if (tid >= a.n_refs) {
        fail = CE_TID;
      } else if (tid >= a.n_vis) {
        d.kind = CK_REF;        // range(0, min(24, len(SQ)))
      } else if (flag & CV_FLAG_MASK) {
        d.kind = CK_FLAG;
      } else {
        const int64_t n_cig = le16(p + 16), c0 = 36 + (int64_t)p[12];
        if (c0 + 4 * n_cig > size) {
          fail = CE_STRUCT;
        } else {
          int64_t span = 0;
          for (int64_t i = 0; i < n_cig; i++) {
            const uint32_t v = le32(p + c0 + 4 * i), op = v & 15u;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += (int64_t)(v >> 4);   // M D N = X
          }
          const int64_t pos = (int64_t)(int32_t)le32(p + 8);
          if (span == 0) {
            d.kind = CK_NOSPAN;
          } else if (pos < 0 || pos >= a.ln[tid]) {
            fail = CE_POS;
          } else {
            d.pos = pos;
            d.end = pos + span;
            d.contig = tid;
            d.kind = CK_USED;
          }
        }
      }
    }
    if (fail) rec_fail(a.err, a.base_rec + t, fail);
    a.desc[t] = d;
  }
}

// one block's share of one record
__device__ __forceinline__ void cov_block_add(const CovArgs &a, int64_t g, int64_t pos, int64_t end) {
  atomicAdd(&a.span[g], (unsigned long long)(end - pos));
  atomicMin(&a.minpos[g], (unsigned long long)pos);
  atomicMax(&a.maxend[g], (unsigned long long)end);
}

__global__ void __launch_bounds__(256) k_cov_apply(CovArgs a) {
  if (*a.err != ~0ull) return;   // a record failed: nothing of this chunk, or of any later one, is kept
  __shared__ uint32_t l_cnt[CV_NCNT];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < CV_NCNT) l_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tiles = (a.n + 255) / 256;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t = tile * 256 + threadIdx.x;
    CovDesc d{0, 0, -1, CK_NONE};
    if (t < a.n) d = a.desc[t];
    {
      const uint64_t b[CV_NCNT] = {__ballot(t < a.n), __ballot(d.kind == CK_USED), __ballot(d.kind == CK_UNPLACED),
                                   __ballot(d.kind == CK_REF), __ballot(d.kind == CK_FLAG), __ballot(d.kind == CK_NOSPAN)};
      if (lane < CV_NCNT && b[lane]) atomicAdd(&l_cnt[lane], (uint32_t)__popcll(b[lane]));
    }
    int64_t k0 = 0, nk = 0, bb = 0;
    if (d.kind == CK_USED) {
      const int64_t ln = a.ln[d.contig], cb = a.cbase[d.contig];
      bb = a.bbase[d.contig];
      const int64_t nb = a.bbase[d.contig + 1] - bb;
      atomicAdd(&a.track[cb + d.pos], 1);
      atomicAdd(&a.track[cb + min(d.end, ln)], -1);
      k0 = max((int64_t)0, (d.pos + a.bl - 1) / a.bl - 1);
      nk = min(nb - 1, (d.end - 1) / a.bl) - k0 + 1;   // (<= 0: a contig without blocks)
      if (nk >= 1 && nk <= 2) {
        cov_block_add(a, bb + k0, d.pos, d.end);
        if (nk == 2) cov_block_add(a, bb + k0 + 1, d.pos, d.end);
      }
    }
    // records over more than two blocks (a long N operation, a small block_len): the wave walks each one's blocks
    uint64_t pend = __ballot(nk > 2);
    while (pend) {
      const int j = __ffsll((unsigned long long)pend) - 1;
      pend &= pend - 1;
      const int64_t g0 = __shfl(bb + k0, j, 64), m = __shfl(nk, j, 64);
      const int64_t pos = __shfl(d.pos, j, 64), end = __shfl(d.end, j, 64);
      for (int64_t i = lane; i < m; i += 64) cov_block_add(a, g0 + i, pos, end);
    }
  }
  __syncthreads();
  if (threadIdx.x < CV_NCNT && l_cnt[threadIdx.x])
    atomicAdd(&a.cnt[threadIdx.x], (unsigned long long)l_cnt[threadIdx.x]);
}

struct TrackLoad {
  const int32_t *p;
  __device__ __forceinline__ int32_t operator()(int64_t i) const { return p[i]; }
};
struct DepthStore {
  int32_t *p;
  __device__ __forceinline__ void operator()(int64_t i, int32_t incl, int32_t) const { p[i] = incl; }
};

// the contig of global block g
__device__ __forceinline__ int cov_contig_of(const int64_t *bbase, int n_vis, int64_t g) {
  int c = 0;
  while (c + 1 < n_vis && g >= bbase[c + 1]) c++;
  return c;
}

__device__ __forceinline__ int64_t cov_block_covered(const int32_t *depth, const int64_t *ln, const int64_t *cbase,
                                                     const int64_t *bbase, int n_vis, int64_t bl, int64_t g, int first,
                                                     int step) {
  const int c = cov_contig_of(bbase, n_vis, g);
  const int64_t a0 = (g - bbase[c]) * bl, b = min(a0 + bl + 1, ln[c]);
  const int32_t *dp = depth + cbase[c];
  int64_t n = 0;
  for (int64_t x = a0 + first; x < b; x += step) n += dp[x] > 0;
  return n;
}

__global__ void __launch_bounds__(256) k_cov_covered(const int32_t *depth, const int64_t *ln, const int64_t *cbase,
                                                     const int64_t *bbase, int32_t n_vis, int64_t bl, int64_t n_blk,
                                                     long long *covered) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
  if (bl + 1 <= 32) {   // blocks shorter than a wave: a lane per block
    for (int64_t g = tid; g < n_blk; g += nthr)
      covered[g] = cov_block_covered(depth, ln, cbase, bbase, n_vis, bl, g, 0, 1);
    return;
  }
  const int lane = threadIdx.x & 63;
  for (int64_t g = tid >> 6; g < n_blk; g += nthr >> 6) {   // (wave-uniform)
    int64_t n = cov_block_covered(depth, ln, cbase, bbase, n_vis, bl, g, lane, 64);
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1) n += __shfl_xor(n, dlt, 64);
    if (lane == 0) covered[g] = n;
  }
}

// block k: the disjoint [k bl, min((k + 1) bl, LN)) and the one base at (k + 1) bl it shares with block k + 1
__global__ void __launch_bounds__(256) k_cov_gc(const uint8_t *seq, int64_t ln, int64_t bl, int64_t nb, uint32_t *n_n,
                                                uint32_t *n_gc) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwave = ((int64_t)gridDim.x * 256) >> 6;
  for (int64_t k = wave; k < nb; k += nwave) {
    const int64_t s = k * bl, e = min(s + bl, ln);
    const int64_t a0 = s & ~(int64_t)15;   // 16-byte pieces of the (aligned) buffer that meet [s, e)
    int nn = 0, ngc = 0;
    for (int64_t lo = a0 + 16 * (int64_t)lane; lo < e; lo += 16 * 64) {
      if (lo >= s && lo + 16 <= e) {
        const uint4 v = *reinterpret_cast<const uint4 *>(seq + lo);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
          nn += count_eq4(w[i], 'N');
          ngc += count_eq4(w[i], 'G') + count_eq4(w[i], 'C');
        }
      } else {
        for (int64_t x = max(lo, s); x < min(lo + 16, e); x++) {
          const uint8_t ch = seq[x];
          nn += ch == 'N';
          ngc += ch == 'G' || ch == 'C';
        }
      }
    }
    if (lane == 0 && s + bl < ln) {
      const uint8_t ch = seq[s + bl];
      nn += ch == 'N';
      ngc += ch == 'G' || ch == 'C';
    }
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1) {
      nn += __shfl_xor(nn, dlt, 64);
      ngc += __shfl_xor(ngc, dlt, 64);
    }
    if (lane == 0) {
      n_n[k] = (uint32_t)nn;
      n_gc[k] = (uint32_t)ngc;
    }
  }
}

// the per-block arrays inside S.blk
struct CovBlk {
  unsigned long long *span, *minpos, *maxend;
  long long *covered;
  uint32_t *n_n, *n_gc;
};
CovBlk cov_blk(const CovState &S) {
  uint8_t *p = (uint8_t *)S.blk.p;
  const size_t n = (size_t)std::max<int64_t>(S.n_blk, 1);
  return {(unsigned long long *)p, (unsigned long long *)(p + 8 * n), (unsigned long long *)(p + 16 * n),
          (long long *)(p + 24 * n), (uint32_t *)(p + 32 * n), (uint32_t *)(p + 36 * n)};
}

int32_t cov_launch(mh_ctx *ctx, const RecChunk &c) {
  CovState &S = ctx->cov;
  hipStream_t st = ctx->stream;
  MH_TRY(ensure(ctx, S.desc, sizeof(CovDesc) * (size_t)c.n));
  const CovBlk b = cov_blk(S);
  const int64_t *tab = (const int64_t *)S.tab.p;
  CovArgs a{c.recs, c.roff, c.n, c.avail, c.base_rec, S.block_len, S.n_refs, S.n_vis, tab, tab + CV_REF,
            tab + 2 * CV_REF + 1, (int32_t *)S.track.p, b.span, b.minpos, b.maxend, (unsigned long long *)S.cnt.p,
            (unsigned long long *)S.ses.err.p, (CovDesc *)S.desc.p};
  const unsigned grid = grid_for(c.n, 256, 8 * (int64_t)ctx->max_cu);
  hipLaunchKernelGGL(k_cov_head, dim3(grid), dim3(256), 0, st, a);
  HIPCHK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_cov_apply, dim3(grid), dim3(256), 0, st, a);
  HIPCHK(ctx, hipGetLastError());
  S.scanned = false;
  return MH_OK;
}

// checked before anything of the call is staged or queued
int32_t cov_room(mh_ctx *ctx, int64_t n) {
  if (ctx->cov.ses.base_rec + n >= ((int64_t)1 << 31))
    return arg_fail(ctx, MH_E_CAPACITY, "gc-cov: 2^31 records or more in one session (the depth track is 32-bit)");
  return MH_OK;
}

int32_t cov_clear(mh_ctx *ctx) {
  CovState &S = ctx->cov;
  hipStream_t st = ctx->stream;
  MH_TRY(session_clear(ctx, S.ses));
  const size_t n = (size_t)std::max<int64_t>(S.n_blk, 1);
  HIPCHK(ctx, hipMemsetAsync(S.track.p, 0, 4 * (size_t)std::max<int64_t>(S.n_cells, 1), st));
  HIPCHK(ctx, hipMemsetAsync(S.blk.p, 0, 40 * n, st));
  HIPCHK(ctx, hipMemsetAsync((uint8_t *)S.blk.p + 8 * n, 0xff, 8 * n, st));   // min pos: none
  HIPCHK(ctx, hipMemsetAsync(S.cnt.p, 0, 8 * CV_NCNT, st));
  SYNCCHK(ctx, hipStreamSynchronize(st));
  S.scanned = false;
  return MH_OK;
}

}  // namespace

int32_t cov_begin(mh_ctx *ctx, int32_t n_refs, const int64_t *lengths, int64_t block_len) {
  CovState &S = ctx->cov;
  if (block_len < 1) return arg_fail(ctx, MH_E_ARG, "block_len must be at least 1");
  S.ses.begun = false;
  S.n_refs = n_refs;
  S.n_vis = std::min(n_refs, CV_REF);
  S.block_len = block_len;
  int64_t tab[3 * CV_REF + 2] = {0};
  int64_t *ln = tab, *cbase = tab + CV_REF, *bbase = tab + 2 * CV_REF + 1;
  for (int c = 0; c < CV_REF; c++) {
    const int64_t L = c < S.n_vis ? lengths[c] : 0;
    if (L < 0 || L > INT32_MAX) return arg_fail(ctx, MH_E_ARG, "reference length outside 0..2^31-1");
    const int64_t nb = L < 2 ? 0 : (L - 1 + block_len - 1) / block_len;   // len(range(1, LN, block_len))
    if (nb > INT32_MAX) return arg_fail(ctx, MH_E_ARG, "2^31 blocks or more in one contig");
    ln[c] = L;
    cbase[c + 1] = cbase[c] + (c < S.n_vis ? L + 1 : 0);
    bbase[c + 1] = bbase[c] + nb;
  }
  std::memcpy(S.ln, ln, sizeof S.ln);
  std::memcpy(S.cbase, cbase, sizeof S.cbase);
  std::memcpy(S.bbase, bbase, sizeof S.bbase);
  S.n_cells = cbase[CV_REF];
  S.n_blk = bbase[CV_REF];
  MH_TRY(ensure(ctx, S.tab, sizeof tab));
  MH_TRY(ensure(ctx, S.track, 4 * (size_t)std::max<int64_t>(S.n_cells, 1)));
  MH_TRY(ensure(ctx, S.blk, 40 * (size_t)std::max<int64_t>(S.n_blk, 1)));
  MH_TRY(ensure(ctx, S.cnt, 64));
  HIPCHK(ctx, hipMemcpyAsync(S.tab.p, tab, sizeof tab, hipMemcpyHostToDevice, ctx->stream));
  MH_TRY(cov_clear(ctx));   // (waits: `tab` is on this frame)
  S.ses.begun = true;
  return MH_OK;
}

int32_t cov_add_records(mh_ctx *ctx, const uint8_t *recs, int64_t len, const int64_t *roff, int64_t n) {
  MH_TRY(cov_room(ctx, n));
  return session_add_records(ctx, ctx->cov.ses, recs, len, roff, n,
                             [ctx](const RecChunk &c) { return cov_launch(ctx, c); });
}

int32_t cov_add_store(mh_ctx *ctx) {
  CovState &S = ctx->cov;
  const BamStore &B = ctx->bam;
  if (S.ses.begun && B.refs_set) {   // (else session_add_store says which of the two is missing)
    if ((int64_t)B.ref_len.size() != S.n_refs) return arg_fail(ctx, MH_E_STATE, "the store's references are not the session's");
    for (int c = 0; c < S.n_vis; c++)
      if (B.ref_len[c] != S.ln[c]) return arg_fail(ctx, MH_E_STATE, "the store's reference lengths are not the session's");
    MH_TRY(cov_room(ctx, B.n_rec));
  }
  return session_add_store(ctx, S.ses, [ctx](const RecChunk &c) { return cov_launch(ctx, c); });
}

int32_t cov_gc(mh_ctx *ctx, int32_t ref_index, int32_t contig_id) {
  CovState &S = ctx->cov;
  MH_TRY(session_begun(ctx, S.ses));
  if (ref_index < 0 || ref_index >= S.n_vis) return arg_fail(ctx, MH_E_ARG, "not one of the session's visited contigs");
  auto it = ctx->contigs.find(contig_id);
  if (it == ctx->contigs.end()) return arg_fail(ctx, MH_E_ARG, "no such uploaded contig");
  if (it->second.len != S.ln[ref_index])
    return arg_fail(ctx, MH_E_ARG, "the uploaded contig has " + std::to_string(it->second.len) + " bases, the header's " +
                                       std::to_string(S.ln[ref_index]));
  const int64_t nb = S.bbase[ref_index + 1] - S.bbase[ref_index];
  if (nb == 0) return MH_OK;
  const CovBlk b = cov_blk(S);
  hipLaunchKernelGGL(k_cov_gc, dim3(grid_for(nb, 4, 8 * (int64_t)ctx->max_cu)), dim3(256), 0, ctx->stream,
                     (const uint8_t *)it->second.seq.p, S.ln[ref_index], S.block_len, nb, b.n_n + S.bbase[ref_index],
                     b.n_gc + S.bbase[ref_index]);
  HIPCHK(ctx, hipGetLastError());
  SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the caller may replace the contig next)
  return MH_OK;
}

int32_t cov_result(mh_ctx *ctx, int32_t ref_index, uint32_t *n_n, uint32_t *n_gc, int64_t *covered, uint64_t *span_sum,
                   int64_t *min_pos, int64_t *max_end, int64_t n_blocks, int64_t *counts) {
  CovState &S = ctx->cov;
  hipStream_t st = ctx->stream;
  MH_TRY(session_begun(ctx, S.ses));
  if (ref_index < 0 || ref_index >= S.n_vis) return arg_fail(ctx, MH_E_ARG, "not one of the session's visited contigs");
  const int64_t b0 = S.bbase[ref_index], nb = S.bbase[ref_index + 1] - b0;
  if (n_blocks != nb) return arg_fail(ctx, MH_E_ARG, "the contig has " + std::to_string(nb) + " blocks");
  std::string failed;   // the arrays are still filled: the sums of the calls before the failing one
  MH_TRY(session_failed(ctx, S.ses, &failed));
  const CovBlk b = cov_blk(S);
  if (!S.scanned && S.n_blk > 0) {
    const int64_t np = scan_partials_count(S.n_cells);
    MH_TRY(ensure(ctx, S.depth, 4 * (size_t)S.n_cells));
    MH_TRY(ensure(ctx, S.partials, 4 * (size_t)(np + 1)));
    int32_t *part = (int32_t *)S.partials.p;
    HIPCHK(ctx, device_scan<int32_t>(st, S.n_cells, TrackLoad{(const int32_t *)S.track.p}, DepthStore{(int32_t *)S.depth.p},
                                     OpSum(), 0, part, part + np));
    const int64_t *tab = (const int64_t *)S.tab.p;
    const int64_t per_wg = S.block_len + 1 <= 32 ? 256 : 4;
    hipLaunchKernelGGL(k_cov_covered, dim3(grid_for(S.n_blk, (int)per_wg, 8 * (int64_t)ctx->max_cu)), dim3(256), 0, st,
                       (const int32_t *)S.depth.p, tab, tab + CV_REF, tab + 2 * CV_REF + 1, S.n_vis, S.block_len, S.n_blk,
                       b.covered);
    HIPCHK(ctx, hipGetLastError());
    S.scanned = true;
  }
  const size_t n = (size_t)nb;
  if (n) {
    if (n_n) HIPCHK(ctx, hipMemcpyAsync(n_n, b.n_n + b0, 4 * n, hipMemcpyDeviceToHost, st));
    if (n_gc) HIPCHK(ctx, hipMemcpyAsync(n_gc, b.n_gc + b0, 4 * n, hipMemcpyDeviceToHost, st));
    if (covered) HIPCHK(ctx, hipMemcpyAsync(covered, b.covered + b0, 8 * n, hipMemcpyDeviceToHost, st));
    if (span_sum) HIPCHK(ctx, hipMemcpyAsync(span_sum, b.span + b0, 8 * n, hipMemcpyDeviceToHost, st));
    if (min_pos) HIPCHK(ctx, hipMemcpyAsync(min_pos, b.minpos + b0, 8 * n, hipMemcpyDeviceToHost, st));
    if (max_end) HIPCHK(ctx, hipMemcpyAsync(max_end, b.maxend + b0, 8 * n, hipMemcpyDeviceToHost, st));
  }
  if (counts) HIPCHK(ctx, hipMemcpyAsync(counts, S.cnt.p, 8 * CV_NCNT, hipMemcpyDeviceToHost, st));
  SYNCCHK(ctx, hipStreamSynchronize(st));
  if (min_pos)
    for (size_t i = 0; i < n; i++)
      if (min_pos[i] < 0) min_pos[i] = MH_COV_NO_POS;   // (the device's cell is all ones where no record met the block)
  if (!failed.empty()) return arg_fail(ctx, MH_E_ARG, failed);
  return MH_OK;
}

int32_t cov_reset(mh_ctx *ctx) {
  MH_TRY(session_begun(ctx, ctx->cov.ses));
  return cov_clear(ctx);
}

void cov_release(CovState &S) {
  release(S.track); release(S.depth); release(S.blk); release(S.cnt); release(S.desc);
  release(S.partials); release(S.tab);
  session_release(S.ses);
}

}  // namespace mh
