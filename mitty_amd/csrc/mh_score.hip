// mh_score.hip — alignment scoring for mq-plot / derr-plot (reference mitty/benchmarking/mq.py:50-68,
// derr.py:53-76 over readgenerate.parse_qname :259-291 and score_alignment_error :294-319) on the device.
//
//   BAM records in HBM (a chunk uploaded from the host reader, or the context's own god-aligner store)
//     -> k_score   thread per record: the record's head (fixed fields + read name) staged in LDS with 16-byte loads,
//                  sample-prefix filter, parse_qname of the mate's group (flag 0x80), chrom against the header name of
//                  tid, d_err, then both matrices from the one pass:
//                    mq_mat[mapq, d_err + max_d]          u64[100][2 max_d + 1]
//                    d_err_mat[max_v + v, d_err + max_d]  u64[2 max_v + 2][2 max_d + 1]   (last row: empty v_list)
//     -> session_commit   the chunk's sums join the session's, unless a record of this or an earlier chunk failed
//
// Contention: nearly every read of a good aligner lands in (MAPQ 60, d_err 0) and (ref or SNP row, d_err 0).  Lanes of
// a wave with equal cells are combined into one add (ballot + popcount); the d_err = 0 column of both matrices is
// kept in per-workgroup LDS counters; a workgroup walks many 256-record tiles and flushes those counters once, with
// 64-bit global atomics.  Integer adds: the result does not depend on the order and is exact.
//
// Every read of a record stays inside [roff[i], roff[i + 1]): lengths taken from the record are clamped to it.  A
// record whose name does not parse (or any other failure) sets the error word with its index and adds nothing.
//
// The staging of the heads and the per-record rule (parse_qname, d_err) are mh_scorerec.h's, shared with filter-bam
// (mh_filter.hip): k_score owns the matrices, the counters and what MAPQ >= 100 means to them.
#include <algorithm>
#include <cstring>

#include "mh_internal.h"
#include "mh_scorerec.h"

namespace mh {

const RecTexts SCORE_TEXTS = {
    "scoring", "call mh_score_begin first",
    "the record store has spilled to the host (mh_bam_set_capacity): score its BAM file",
    {SCORE_KIND_TEXT[0], SCORE_KIND_TEXT[1], SCORE_KIND_TEXT[2], SCORE_KIND_TEXT[3], SCORE_KIND_TEXT[4],
     SCORE_KIND_TEXT[5]}};

namespace {

constexpr int SC_NV_LDS = 1026;   // d_err_mat rows with an LDS counter for their d_err = 0 column (max_v_len <= 512)

struct ScoreArgs {
  const uint8_t *recs;
  const int64_t *roff;
  int64_t n, avail;            // records; bytes readable at recs
  ScoreRule rule;              // header names, sample prefix, max_d, strict
  int32_t max_d, max_v;
  unsigned long long *mq, *dv, *cnt;   // the chunk's sums
  unsigned long long *err;
  int64_t base_rec;
};

// One add per distinct cell among the wave's lanes (cell < 0: none).  The d_err = 0 column goes to the workgroup's LDS
// counters (row < lds_rows), everything else to the chunk's matrix in memory.  Called by every lane of the wave.
__device__ __forceinline__ void wave_add(int32_t cell, int lane, int32_t ncol, int32_t zero_col, uint32_t *lds,
                                         int32_t lds_rows, unsigned long long *g) {
  wave_distinct(cell, lane, [&](int32_t lc, uint32_t c) {
    const int32_t row = lc / ncol, col = lc - row * ncol;
    if (col == zero_col && row < lds_rows) atomicAdd(&lds[row], c);
    else atomicAdd(&g[lc], (unsigned long long)c);
  });
}

__global__ void __launch_bounds__(256) k_score(ScoreArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t rows[256 * SC_ROW];
  __shared__ uint32_t l_mq[100], l_dv[SC_NV_LDS], l_cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t ncol = 2 * a.max_d + 1, n_vrow = 2 * a.max_v + 2;
  const int32_t lds_vrows = n_vrow < SC_NV_LDS ? n_vrow : SC_NV_LDS;
  for (int i = threadIdx.x; i < 100; i += 256) l_mq[i] = 0;
  for (int i = threadIdx.x; i < SC_NV_LDS; i += 256) l_dv[i] = 0;
  if (threadIdx.x < 4) l_cnt[threadIdx.x] = 0;
  const int64_t tiles = (a.n + 255) / 256;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();   // the counters are zero / the previous tile's rows are no longer read
    sc_stage_heads(rows, a.recs, a.roff, a.n, a.avail, tile, wave, lane);
    __syncthreads();
    // ---- the thread's record
    const int64_t t = tile * 256 + threadIdx.x;
    int32_t mq_cell = -1, col = 0, kind = 0;
    int vs = 0, ve = 0, v_items = -1;      // the scored group's v_list in the name; -1: nothing to add
    const uint8_t *q = nullptr;            // the read name
    int seen = 0, scored = 0, skip_tid = 0, skip_smp = 0;
    if (t < a.n) {
      const int64_t s = a.roff[t], e = a.roff[t + 1];
      const int64_t size = e - s;
      seen = 1;
      if (size < 36 || s < 0 || e > a.avail) {
        kind = SE_STRUCT;
      } else {
        const uint8_t *lp = sc_head(rows, a.recs, s, e, a.avail);
        const ScoreRec r = score_record(lp, size, (int32_t)le16(lp + 18), (int32_t)le32(lp + 4),
                                        (int32_t)le32(lp + 8), a.rule);
        q = r.q;
        kind = r.kind;
        skip_tid = r.skip_tid;
        skip_smp = r.skip_smp;
        if (r.scored) {
          if (r.mapq >= 100) {
            kind = SE_MAPQ;   // mq_mat[r.mapq, ...] raises IndexError
          } else {
            col = r.d_err + a.max_d;
            mq_cell = r.mapq * ncol + col;
            vs = r.vs;
            ve = r.ve;
            v_items = r.v_items;
            scored = 1;
          }
        }
      }
      if (kind) rec_fail(a.err, a.base_rec + t, kind);
    }
    {   // the four counts: one LDS add per wave each
      const uint64_t b[4] = {__ballot(seen), __ballot(scored), __ballot(skip_tid), __ballot(skip_smp)};
      if (lane < 4 && b[lane]) atomicAdd(&l_cnt[lane], (uint32_t)__popcll(b[lane]));
    }
    // ---- both matrices
    wave_add(mq_cell, lane, ncol, a.max_d, l_mq, 100, a.mq);
    // d_err_mat: a row per v of the v_list inside +-max_v, the last row for an empty list; the wave goes round once per
    // list position
    int32_t left = v_items < 0 ? 0 : (v_items == 0 ? 1 : v_items);
    int vi = vs;
    while (__ballot(left > 0)) {
      int32_t cell = -1;
      if (left > 0) {
        left--;
        if (v_items == 0) {
          cell = (n_vrow - 1) * ncol + col;
        } else {
          int st = vi;
          while (st < ve && q[st] == ',') st++;   // empty items are skipped
          int en = st;
          while (en < ve && q[en] != ',') en++;
          int64_t v = 0;
          (void)sc_int(q, st, en, v);
          vi = en + 1;
          const int64_t r = (int64_t)a.max_v + v;
          if (r >= 0 && r < 2 * (int64_t)a.max_v + 1) cell = (int32_t)r * ncol + col;
        }
      }
      wave_add(cell, lane, ncol, a.max_d, l_dv, lds_vrows, a.dv);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 100; i += 256)
    if (l_mq[i]) atomicAdd(&a.mq[(int64_t)i * ncol + a.max_d], (unsigned long long)l_mq[i]);
  for (int i = threadIdx.x; i < lds_vrows; i += 256)
    if (l_dv[i]) atomicAdd(&a.dv[(int64_t)i * ncol + a.max_d], (unsigned long long)l_dv[i]);
  if (threadIdx.x < 4 && l_cnt[threadIdx.x]) atomicAdd(&a.cnt[threadIdx.x], (unsigned long long)l_cnt[threadIdx.x]);
}

// the chunk's sums zeroed, the records scored, the sums committed; all queued on the context's stream.  Header names:
// the store's own on that path, the session's otherwise
int32_t score_launch(mh_ctx *ctx, const RecChunk &c) {
  ScoreState &S = ctx->score;
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemsetAsync(S.delta.p, 0, sizeof(uint64_t) * S.n_all, st));
  unsigned long long *d = (unsigned long long *)S.delta.p;
  ScoreRule rule = S.refs.rule(S.max_d, S.strict);
  if (c.store) {
    rule.names = (const char *)c.store->names.p;
    rule.name_off = (const int32_t *)c.store->name_off.p;
    rule.n_refs = (int32_t)c.store->ref_names.size();
  }
  ScoreArgs a{c.recs, c.roff, c.n, c.avail, rule, S.max_d, S.max_v, d, d + S.n_mq, d + S.n_mq + S.n_dv,
              (unsigned long long *)S.ses.err.p, c.base_rec};
  // a workgroup's LDS counters are 32-bit: at most 4096 tiles (2^20 records, < 2^8 list items each) per workgroup
  const int64_t tiles = (c.n + 255) / 256;
  const int64_t grid = std::min<int64_t>(tiles, std::max<int64_t>(8 * (int64_t)ctx->max_cu, (tiles + 4095) / 4096));
  hipLaunchKernelGGL(k_score, dim3((unsigned)grid), dim3(256), 0, st, a);
  HIPCHK(ctx, hipGetLastError());
  return session_commit(ctx, S.ses, S.delta, S.acc, S.n_all, S.n_all);   // (no cell is a maximum)
}

int32_t score_clear(mh_ctx *ctx) {
  ScoreState &S = ctx->score;
  MH_TRY(session_clear(ctx, S.ses));
  HIPCHK(ctx, hipMemsetAsync(S.acc.p, 0, sizeof(uint64_t) * S.n_all, ctx->stream));
  SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

}  // namespace

int32_t score_begin(mh_ctx *ctx, int32_t n_refs, const char *names, int32_t max_d, int32_t max_v_len, int32_t strict,
                    const char *sample_prefix) {
  ScoreState &S = ctx->score;
  if (n_refs < 0 || (n_refs > 0 && !names)) return arg_fail(ctx, MH_E_ARG, "bad reference list");
  if (max_d < 0 || max_d > (1 << 20)) return arg_fail(ctx, MH_E_ARG, "max_d must be 0..2^20");
  if (max_v_len < 51) max_v_len = 51;   // derr.py:21-23
  if (max_v_len > (1 << 20)) return arg_fail(ctx, MH_E_ARG, "max_v_len must be at most 2^20");
  const int64_t ncol = 2 * (int64_t)max_d + 1;
  if ((2 * (int64_t)max_v_len + 2) * ncol >= INT32_MAX) return arg_fail(ctx, MH_E_ARG, "d_err matrix of 2^31 cells or more");
  S.ses.begun = false;
  S.max_d = max_d;
  S.max_v = max_v_len;
  S.strict = strict ? 1 : 0;
  S.n_mq = 100 * ncol;
  S.n_dv = (2 * (int64_t)max_v_len + 2) * ncol;
  S.n_all = S.n_mq + S.n_dv + 4;
  MH_TRY(ensure(ctx, S.acc, sizeof(uint64_t) * S.n_all));
  MH_TRY(ensure(ctx, S.delta, sizeof(uint64_t) * S.n_all));
  MH_TRY(S.refs.upload(ctx, n_refs, names, sample_prefix));
  MH_TRY(score_clear(ctx));
  S.ses.begun = true;
  return MH_OK;
}

int32_t score_add_records(mh_ctx *ctx, const uint8_t *recs, int64_t len, const int64_t *roff, int64_t n) {
  return session_add_records(ctx, ctx->score.ses, recs, len, roff, n,
                             [ctx](const RecChunk &c) { return score_launch(ctx, c); });
}

// (the sums do not depend on the store's order)
int32_t score_add_store(mh_ctx *ctx) {
  return session_add_store(ctx, ctx->score.ses, [ctx](const RecChunk &c) { return score_launch(ctx, c); });
}

int32_t score_result(mh_ctx *ctx, uint64_t *mq_mat, uint64_t *derr_mat, int64_t *counts) {
  ScoreState &S = ctx->score;
  MH_TRY(session_begun(ctx, S.ses));
  std::string failed;
  MH_TRY(session_failed(ctx, S.ses, &failed));
  if (!failed.empty()) return arg_fail(ctx, MH_E_ARG, failed);
  const uint64_t *acc = (const uint64_t *)S.acc.p;
  if (mq_mat) HIPCHK(ctx, hipMemcpyAsync(mq_mat, acc, 8 * S.n_mq, hipMemcpyDeviceToHost, ctx->stream));
  if (derr_mat) HIPCHK(ctx, hipMemcpyAsync(derr_mat, acc + S.n_mq, 8 * S.n_dv, hipMemcpyDeviceToHost, ctx->stream));
  if (counts) HIPCHK(ctx, hipMemcpyAsync(counts, acc + S.n_mq + S.n_dv, 32, hipMemcpyDeviceToHost, ctx->stream));
  SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

int32_t score_reset(mh_ctx *ctx) {
  MH_TRY(session_begun(ctx, ctx->score.ses));
  return score_clear(ctx);
}

void score_release(ScoreState &S) {
  release(S.acc); release(S.delta);
  S.refs.release();
  session_release(S.ses);
}

}  // namespace mh
