// mh_model.hip — bam2illumina's pass (reference mitty/empirical/bam2illumina.py:17-59 summed over contigs by :84-105)
// on the device: the base-quality histogram per mate and base position, the template-length histogram, and the counts.
//
//   BAM records in HBM (a chunk uploaded from the host reader, or the context's own god-aligner store)
//     -> k_model_refcount, k_model_refscan   (every > 1 only) per 256-record tile and refID, the ordinal of the tile's
//                  first record among the session's records of that refID: the reference's enumerate() over a contig
//     -> k_model_head   thread per record: fixed fields, the rule's steps 1-3 (refID, every, flag), the counts, the
//                  template length, min / max l_seq; a 16-byte descriptor per used record (where its qualities are)
//     -> k_model_hist   wave per record, lane per base position, coalesced quality bytes into 32-bit LDS counters
//                  bq[position][quality] of ONE mate; flushed once per workgroup with 64-bit global atomics
//     -> session_commit   the chunk's sums join the session's, unless a record of this or an earlier chunk failed
//
// The same passes serve `bq` (reference mitty/empirical/bq.py:20-35, per contig by :38-54): a second ModelState whose
// table selector is the record's refID instead of its mate (by_ref), 24 tables of 500 x 100, no template lengths.
//
// LDS split: 2 x 300 x 94 x 4 B = 225 KB does not fit the CU's 160 KiB, one mate's 112.8 KB does.  A workgroup of 1024
// threads owns a 120 KiB table and takes the records of one mate (blockIdx chooses it); it skips the other mate's
// records by their descriptors, so no quality byte is loaded twice.  A shape whose mate table exceeds 120 KiB (max_bq
// up to 256, large max_bp) is cut further into slabs of base positions; a slab's workgroups read only bytes
// [p0, p1) of each record.  The lanes of a wave hold distinct positions of one record, hence distinct rows: the hot
// cells (every record of a run has the same quality at position i) meet only across waves, in LDS.  A counter gains at
// most 1 per record, and a workgroup sees fewer than 2^32 records, so the 32-bit counters cannot wrap.
//
// Every read stays inside [roff[i], roff[i + 1]) and inside `avail`: k_model_head checks 36 + l_read_name + 4 n_cigar +
// (l_seq + 1) / 2 + l_seq against the record's size before it writes the descriptor k_model_hist reads from.
#include <algorithm>
#include <climits>
#include <cstring>

#include "mh_internal.h"
#include "mh_scan.h"

namespace mh {

static constexpr RecTexts model_texts(const char *label) {
  return {label, "call the session's begin first",
          "the record store has spilled to the host (mh_bam_set_capacity): use its BAM file",
          {"", "fields do not fit the record", "tid outside the header's references", "l_seq is 0 (no qualities)",
           "read longer than max_bp", "base quality of max_bq or more (0xff: no qualities stored)"}};
}
const RecTexts MODEL_TEXTS = model_texts("read model"), BQ_TEXTS = model_texts("bq");

namespace {

constexpr int MD_REF = ModelState::N_REF;
constexpr int MD_LDS_CELLS = 30720;   // k_model_hist's table: 120 KiB of 32-bit counters
constexpr int MD_TLEN_LDS = 4096;     // tlen histograms up to this many bins are kept per workgroup in LDS
constexpr int MD_NCNT = 8;            // seen, used, 4 x skipped, INT32_MAX - min l_seq (0: none), max l_seq

enum { ME_STRUCT = 1, ME_TID = 2, ME_EMPTY = 3, ME_LONG = 4, ME_QUAL = 5 };

struct ModelDesc {   // 16 bytes per record of the chunk
  int64_t q;         // offset of the qualities from recs; -1: the record is not used
  int32_t len;       // l_seq
  int32_t bits;      // bit 0: reverse strand; bits 1..: the table (mate index m, 0: read1; by_ref: the refID)
};

struct ModelArgs {
  const uint8_t *recs;
  const int64_t *roff;
  int64_t n, avail;
  int32_t n_refs, every, min_mq, max_bq, max_bp, max_tlen;
  int32_t slab_bp, n_slab, wg_per_part, by_ref;
  unsigned long long *bq, *tlen, *cnt, *refcnt;   // the chunk's sums
  const unsigned long long *ref_base;             // the session's records per refID before this chunk
  unsigned long long *tile_ord;                   // [tiles][MD_REF]
  ModelDesc *desc;
  unsigned long long *err;
  int64_t base_rec;
};

// refID of record t when its fixed fields are readable and it is one of the visited contigs, else -1
__device__ __forceinline__ int32_t md_ref(const ModelArgs &a, int64_t t) {
  int64_t s, size;
  if (t >= a.n || !rec_span(a.roff, t, a.avail, &s, &size)) return -1;
  const int32_t tid = (int32_t)le32(a.recs + s + 4);
  return tid >= 0 && tid < a.n_refs && tid < MD_REF ? tid : -1;
}

// records per refID of each 256-record tile
__global__ void __launch_bounds__(256) k_model_refcount(ModelArgs a) {
  __shared__ uint32_t h[MD_REF];
  const int64_t tiles = (a.n + 255) / 256;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    if (threadIdx.x < MD_REF) h[threadIdx.x] = 0;
    __syncthreads();
    const int32_t r = md_ref(a, tile * 256 + threadIdx.x);
    if (r >= 0) atomicAdd(&h[r], 1u);
    __syncthreads();
    if (threadIdx.x < MD_REF) a.tile_ord[tile * MD_REF + threadIdx.x] = h[threadIdx.x];
    __syncthreads();
  }
}

// per refID (a wave takes every fourth) the exclusive prefix of the tiles' counts, from the session's count on; the
// chunk's total per refID goes to the chunk's sums and joins the session's when the chunk commits
__global__ void __launch_bounds__(256) k_model_refscan(ModelArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tiles = (a.n + 255) / 256;
  for (int r = wave; r < MD_REF; r += 4) {
    const unsigned long long base = a.ref_base[r];
    unsigned long long carry = base;
    for (int64_t b0 = 0; b0 < tiles; b0 += 64) {
      const int64_t i = b0 + lane;
      const unsigned long long v = i < tiles ? a.tile_ord[i * MD_REF + r] : 0ull;
      unsigned long long inc = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = shfl_up_t(inc, d);
        if (lane >= d) inc += o;
      }
      if (i < tiles) a.tile_ord[i * MD_REF + r] = carry + inc - v;
      carry += shfl_idx_t(inc, 63);
    }
    if (lane == 0) a.refcnt[r] = carry - base;
  }
}

__global__ void __launch_bounds__(256) k_model_head(ModelArgs a) {
  __shared__ uint32_t l_tlen[MD_TLEN_LDS];
  __shared__ uint32_t l_cnt[MD_NCNT], l_wref[4][MD_REF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool tlen_lds = a.max_tlen <= MD_TLEN_LDS;
  if (tlen_lds)
    for (int i = threadIdx.x; i < a.max_tlen; i += 256) l_tlen[i] = 0;
  if (threadIdx.x < MD_NCNT) l_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tiles = (a.n + 255) / 256;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t = tile * 256 + threadIdx.x;
    // ---- the record's ordinal among the records of its refID (step 2), all flags counted
    unsigned long long ord = 0;
    if (a.every > 1) {   // (uniform)
      __syncthreads();
      if (threadIdx.x < 4 * MD_REF) (&l_wref[0][0])[threadIdx.x] = 0;
      __syncthreads();
      const int32_t r = md_ref(a, t);
      uint32_t before = 0;
      uint64_t pend = __ballot(r >= 0);
      while (pend) {
        const int leader = __ffsll((unsigned long long)pend) - 1;
        const int32_t lr = __shfl(r, leader, 64);
        const uint64_t m = __ballot(r == lr);
        if (r == lr) before = (uint32_t)__popcll(m & (((uint64_t)1 << lane) - 1));
        if (lane == leader) l_wref[wave][lr] = (uint32_t)__popcll(m);
        pend &= ~m;
      }
      __syncthreads();
      if (r >= 0) {
        ord = a.tile_ord[tile * MD_REF + r] + before;
        for (int w = 0; w < wave; w++) ord += l_wref[w][r];
      }
    }
    // ---- steps 1-5
    int32_t kind = 0, tcell = -1, L = 0;
    int seen = 0, used = 0, sk_unpl = 0, sk_ref = 0, sk_every = 0, sk_flag = 0;
    ModelDesc d{-1, 0, 0};
    if (t < a.n) {
      int64_t s, size;
      seen = 1;
      if (!rec_span(a.roff, t, a.avail, &s, &size)) {
        kind = ME_STRUCT;
      } else {
        const uint8_t *p = a.recs + s;
        const int32_t tid = (int32_t)le32(p + 4);
        const int32_t mapq = p[13], flag = (int32_t)le16(p + 18);
        if (tid < 0) {
          sk_unpl = 1;   // fetch(reference=SN) never yields these
        } else if (tid >= a.n_refs) {
          kind = ME_TID;
        } else if (tid >= MD_REF) {
          sk_ref = 1;    // refs[:24]
        } else if (a.every > 1 && ord % (unsigned long long)a.every != 0) {
          sk_every = 1;
        } else if (flag > 255) {
          sk_flag = 1;
        } else {
          const int64_t l_seq = (int64_t)le32(p + 20);
          const int64_t qoff = 36 + (int64_t)p[12] + 4 * (int64_t)le16(p + 16) + (l_seq + 1) / 2;
          if (l_seq == 0) kind = ME_EMPTY;           // query_qualities is None
          else if (l_seq > a.max_bp) kind = ME_LONG;  // bq_mat's second index
          else if (qoff + l_seq > size) kind = ME_STRUCT;
          else {
            used = 1;
            L = (int32_t)l_seq;
            d.q = s + qoff;
            d.len = L;
            d.bits = (a.by_ref ? tid : ((flag & 0x40) ? 0 : 1)) << 1 | ((flag & 0x10) ? 1 : 0);
            int64_t T = (int64_t)(int32_t)le32(p + 32);
            if (T < 0) T = -T;
            if (mapq >= a.min_mq && mapq != 255 && (flag & 0x80) && T < a.max_tlen) tcell = (int32_t)T;
          }
        }
      }
      if (kind) rec_fail(a.err, a.base_rec + t, kind);
      a.desc[t] = d;
    }
    {
      const uint64_t b[6] = {__ballot(seen), __ballot(used), __ballot(sk_unpl),
                             __ballot(sk_ref), __ballot(sk_every), __ballot(sk_flag)};
      if (lane < 6 && b[lane]) atomicAdd(&l_cnt[lane], (uint32_t)__popcll(b[lane]));
      int32_t lo = used ? INT32_MAX - L : 0, hi = L;   // both are maxima
#pragma unroll
      for (int dlt = 32; dlt >= 1; dlt >>= 1) {
        lo = max(lo, __shfl_xor(lo, dlt, 64));
        hi = max(hi, __shfl_xor(hi, dlt, 64));
      }
      if (lane == 0 && hi > 0) {
        atomicMax(&l_cnt[6], (uint32_t)lo);
        atomicMax(&l_cnt[7], (uint32_t)hi);
      }
    }
    if (tlen_lds) {
      if (tcell >= 0) atomicAdd(&l_tlen[tcell], 1u);
    } else {   // one global add per distinct template length among the wave's lanes
      wave_distinct(tcell, lane, [&](int32_t lc, uint32_t c) { atomicAdd(&a.tlen[lc], (unsigned long long)c); });
    }
  }
  __syncthreads();
  if (tlen_lds)
    for (int i = threadIdx.x; i < a.max_tlen; i += 256)
      if (l_tlen[i]) atomicAdd(&a.tlen[i], (unsigned long long)l_tlen[i]);
  if (threadIdx.x < 6 && l_cnt[threadIdx.x]) atomicAdd(&a.cnt[threadIdx.x], (unsigned long long)l_cnt[threadIdx.x]);
  if ((threadIdx.x == 6 || threadIdx.x == 7) && l_cnt[threadIdx.x])
    atomicMax(&a.cnt[threadIdx.x], (unsigned long long)l_cnt[threadIdx.x]);
}

// blockIdx.x = part * wg_per_part + g; part = table * n_slab + slab.  The part's workgroups share the chunk's records in
// batches of 64 descriptors per wave.
__global__ void __launch_bounds__(1024) k_model_hist(ModelArgs a) {
  __shared__ uint32_t tab[MD_LDS_CELLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int part = blockIdx.x / a.wg_per_part, g = blockIdx.x - part * a.wg_per_part;
  const int tsel = part / a.n_slab, slab = part - tsel * a.n_slab;
  const int32_t p0 = slab * a.slab_bp, p1 = min(p0 + a.slab_bp, a.max_bp);
  const int32_t cells = (p1 - p0) * a.max_bq;   // <= MD_LDS_CELLS (model_begin)
  for (int i = threadIdx.x; i < cells; i += 1024) tab[i] = 0;
  __syncthreads();
  const int64_t batches = (a.n + 63) / 64;
  for (int64_t batch = (int64_t)g * 16 + wave; batch < batches; batch += (int64_t)a.wg_per_part * 16) {
    const int64_t r = batch * 64 + lane;
    ModelDesc d{-1, 0, 0};
    if (r < a.n) d = a.desc[r];
    uint64_t pend = __ballot(d.q >= 0 && (d.bits >> 1) == tsel && d.len > p0);
    while (pend) {
      const int j = __ffsll((unsigned long long)pend) - 1;
      pend &= pend - 1;
      const int64_t q = __shfl(d.q, j, 64);
      const int32_t len = __shfl(d.len, j, 64), rev = __shfl(d.bits, j, 64) & 1;
      const int32_t hi = min(len, p1);
      for (int32_t i0 = p0 + lane; i0 < hi; i0 += 256) {   // (no barrier or shuffle inside: lanes past the end leave)
        uint32_t b[4];   // up to 256 positions' bytes in flight before the first add
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int32_t i = i0 + 64 * k;
          b[k] = i < hi ? (uint32_t)a.recs[q + (rev ? len - 1 - i : i)] : 0x100u;   // 0x100: no position
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (b[k] == 0x100u) continue;
          if (b[k] >= (uint32_t)a.max_bq)   // bq_mat's third index (0xff: the record carries no qualities)
            rec_fail(a.err, a.base_rec + batch * 64 + j, ME_QUAL);
          else
            atomicAdd(&tab[(i0 + 64 * k - p0) * a.max_bq + (int32_t)b[k]], 1u);
        }
      }
    }
  }
  __syncthreads();
  unsigned long long *out = a.bq + ((int64_t)tsel * a.max_bp + p0) * a.max_bq;
  for (int i = threadIdx.x; i < cells; i += 1024)
    if (tab[i]) atomicAdd(&out[i], (unsigned long long)tab[i]);
}

// the chunk's sums zeroed, the passes over the records, the sums committed; all queued on the context's stream
int32_t model_launch(mh_ctx *ctx, ModelState &S, const RecChunk &c) {
  hipStream_t st = ctx->stream;
  const int64_t n = c.n;
  const int32_t n_refs = c.store ? (int32_t)c.store->ref_names.size() : S.n_refs;
  const int64_t tiles = (n + 255) / 256;
  MH_TRY(ensure(ctx, S.desc, sizeof(ModelDesc) * (size_t)n));
  if (S.every > 1) MH_TRY(ensure(ctx, S.tile_ord, sizeof(uint64_t) * MD_REF * (size_t)tiles));
  HIPCHK(ctx, hipMemsetAsync(S.delta.p, 0, sizeof(uint64_t) * S.n_all, st));
  unsigned long long *d = (unsigned long long *)S.delta.p;
  const int64_t o_tlen = S.n_bq, o_cnt = o_tlen + S.max_tlen, o_ref = o_cnt + MD_NCNT;
  const int parts = S.n_tab * S.n_slab;
  // a part's workgroups: enough for every CU, no more than there are 16-wave loads of 64 records; 32-bit LDS counters
  // gain 1 per record at the most, so fewer than 2^32 records per workgroup
  // by_ref: a chunk's records sit on one or two contigs (a sorted file, a one-contig store), so a table's share is
  // sized as if it had the device alone; the other tables' workgroups find no record of theirs and flush nothing
  const int64_t batches = (n + 63) / 64;
  const int busy = S.by_ref ? S.n_slab : parts;
  int64_t wgp = std::min<int64_t>((batches + 15) / 16, std::max<int64_t>(1, (ctx->max_cu + busy - 1) / busy));
  wgp = std::max<int64_t>(wgp, (n >> 31) + 1);
  ModelArgs a{c.recs, c.roff, n, c.avail, n_refs, S.every, S.min_mq, S.max_bq, S.max_bp, S.max_tlen, S.slab_bp, S.n_slab,
              (int32_t)wgp, S.by_ref ? 1 : 0, d, d + o_tlen, d + o_cnt, d + o_ref,
              (const unsigned long long *)S.acc.p + o_ref, (unsigned long long *)S.tile_ord.p,
              (ModelDesc *)S.desc.p, (unsigned long long *)S.ses.err.p, c.base_rec};
  const int64_t grid = std::min<int64_t>(tiles, std::max<int64_t>(8 * (int64_t)ctx->max_cu, (tiles + 4095) / 4096));
  if (S.every > 1) {
    hipLaunchKernelGGL(k_model_refcount, dim3((unsigned)grid), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_model_refscan, dim3(1), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(k_model_head, dim3((unsigned)grid), dim3(256), 0, st, a);
  HIPCHK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_model_hist, dim3((unsigned)(wgp * parts)), dim3(1024), 0, st, a);
  HIPCHK(ctx, hipGetLastError());
  // cells o_cnt + 6 and + 7 are maxima (INT32_MAX - min l_seq, max l_seq), every other cell is a sum
  return session_commit(ctx, S.ses, S.delta, S.acc, S.n_all, o_cnt + 6);
}

int32_t model_clear(mh_ctx *ctx, ModelState &S) {
  MH_TRY(session_clear(ctx, S.ses));
  HIPCHK(ctx, hipMemsetAsync(S.acc.p, 0, sizeof(uint64_t) * S.n_all, ctx->stream));
  SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

}  // namespace

int32_t model_begin(mh_ctx *ctx, ModelState &S, int32_t n_refs, int32_t every, int32_t min_mq, int32_t max_bq,
                    int32_t max_bp, int32_t max_tlen, bool by_ref) {
  const int32_t n_tab = by_ref ? MD_REF : 2;
  if (n_refs < 0) return arg_fail(ctx, MH_E_ARG, "bad reference count");
  if (every < 1) return arg_fail(ctx, MH_E_ARG, "every must be at least 1");
  if (max_bq < 1 || max_bq > 256) return arg_fail(ctx, MH_E_ARG, "max_bq must be 1..256");
  if (max_bp < 1 || max_tlen < 1) return arg_fail(ctx, MH_E_ARG, "max_bp and max_tlen must be positive");
  if (n_tab * (int64_t)max_bp * max_bq >= INT32_MAX) return arg_fail(ctx, MH_E_ARG, "bq_mat of 2^31 cells or more");
  if (max_tlen == INT32_MAX) return arg_fail(ctx, MH_E_ARG, "tlen histogram of 2^31 cells or more");
  S.ses.begun = false;
  S.n_refs = n_refs;
  S.every = every;
  S.min_mq = min_mq;
  S.max_bq = max_bq;
  S.max_bp = max_bp;
  S.max_tlen = max_tlen;
  S.n_tab = n_tab;
  S.by_ref = by_ref;
  S.slab_bp = std::min(max_bp, MD_LDS_CELLS / max_bq);
  S.n_slab = (max_bp + S.slab_bp - 1) / S.slab_bp;
  S.n_bq = n_tab * (int64_t)max_bp * max_bq;
  S.n_all = S.n_bq + max_tlen + MD_NCNT + MD_REF;
  MH_TRY(ensure(ctx, S.acc, sizeof(uint64_t) * S.n_all));
  MH_TRY(ensure(ctx, S.delta, sizeof(uint64_t) * S.n_all));
  MH_TRY(model_clear(ctx, S));
  S.ses.begun = true;
  return MH_OK;
}

int32_t model_add_records(mh_ctx *ctx, ModelState &S, const uint8_t *recs, int64_t len, const int64_t *roff,
                          int64_t n) {
  return session_add_records(ctx, S.ses, recs, len, roff, n,
                             [ctx, &S](const RecChunk &c) { return model_launch(ctx, S, c); });
}

// (the store's own order stands for the file's)
int32_t model_add_store(mh_ctx *ctx, ModelState &S) {
  return session_add_store(ctx, S.ses, [ctx, &S](const RecChunk &c) { return model_launch(ctx, S, c); });
}

// the session's work waited for; the first failing record, if any, as MH_E_ARG
static int32_t model_wait(mh_ctx *ctx, ModelState &S) {
  MH_TRY(session_begun(ctx, S.ses));
  std::string failed;
  MH_TRY(session_failed(ctx, S.ses, &failed));
  return failed.empty() ? MH_OK : arg_fail(ctx, MH_E_ARG, failed);
}

int32_t model_result(mh_ctx *ctx, ModelState &S, uint64_t *bq_mat, uint64_t *tlen_mat, int64_t *counts) {
  MH_TRY(model_wait(ctx, S));
  const uint64_t *acc = (const uint64_t *)S.acc.p;
  if (bq_mat) HIPCHK(ctx, hipMemcpyAsync(bq_mat, acc, 8 * S.n_bq, hipMemcpyDeviceToHost, ctx->stream));
  if (tlen_mat)
    HIPCHK(ctx, hipMemcpyAsync(tlen_mat, acc + S.n_bq, 8 * (size_t)S.max_tlen, hipMemcpyDeviceToHost, ctx->stream));
  if (counts)
    HIPCHK(ctx, hipMemcpyAsync(counts, acc + S.n_bq + S.max_tlen, 8 * MD_NCNT, hipMemcpyDeviceToHost, ctx->stream));
  SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (counts) counts[6] = counts[6] ? (int64_t)INT32_MAX - counts[6] : MH_MODEL_NO_RLEN;
  return MH_OK;
}

// one table (a contig's matrix of a by_ref session) and the counts
int32_t model_result_table(mh_ctx *ctx, ModelState &S, int32_t tab, uint64_t *mat, int64_t *counts) {
  MH_TRY(model_wait(ctx, S));
  if (tab < 0 || tab >= S.n_tab || (S.by_ref && tab >= S.n_refs))
    return arg_fail(ctx, MH_E_ARG, "no such table in the session");
  const uint64_t *acc = (const uint64_t *)S.acc.p;
  const int64_t cells = (int64_t)S.max_bp * S.max_bq;
  if (mat) HIPCHK(ctx, hipMemcpyAsync(mat, acc + tab * cells, 8 * cells, hipMemcpyDeviceToHost, ctx->stream));
  if (counts)
    HIPCHK(ctx, hipMemcpyAsync(counts, acc + S.n_bq + S.max_tlen, 8 * MD_NCNT, hipMemcpyDeviceToHost, ctx->stream));
  SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (counts) counts[6] = counts[6] ? (int64_t)INT32_MAX - counts[6] : MH_MODEL_NO_RLEN;
  return MH_OK;
}

int32_t model_reset(mh_ctx *ctx, ModelState &S) {
  MH_TRY(session_begun(ctx, S.ses));
  return model_clear(ctx, S);
}

void model_release(ModelState &S) {
  release(S.acc); release(S.delta); release(S.desc); release(S.tile_ord);
  session_release(S.ses);
}

}  // namespace mh
