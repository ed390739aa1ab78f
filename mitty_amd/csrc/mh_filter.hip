// mh_filter.hip — filter-bam: a BAM's records kept or dropped by their alignment error, on the device, and the kept ones
// written as a new BAM.  The score is mh_scorerec.h's (the one k_score counts by), so the records kept by default are
// exactly those mq-plot counts outside its d_err = 0 column.
//
//   a chunk of BAM records in HBM (uploaded from the host reader by the session core, mh_recs.hip)
//     -> k_filter_mark    thread per record, heads staged in LDS as k_score stages them: the verdict, the record's kept
//                         bytes (0 or its size) and the eight counts
//     -> look-back scan   exclusive sums of (kept bytes, kept records): each kept record's destination, and the compact
//                         list of kept records (source offset, destination offset) the gather searches
//     -> k_filter_gather  a wave per 4 KiB of output, a lane per 16-byte destination word: the kept records, input
//                         order, behind the carry of the earlier chunks
//     -> bgzf_device      the whole 0xff00-byte blocks of [carry | kept bytes]; the rest is the next chunk's carry
//     -> the session's BgzfSink (mh_bgzfsink.hip): its thread copies the blocks out and writes them while the next
//                         chunk's kernels run
//
// The blocks are cut at fixed multiples of 0xff00 of the kept stream, so the file does not depend on how the input was
// cut into chunks.  Once a record fails, nothing of its chunk or of a later one is written, and finish removes the file.
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>

#include "mh_bgzf.h"
#include "mh_internal.h"
#include "mh_scan.h"
#include "mh_scorerec.h"

namespace mh {

const RecTexts FILTER_TEXTS = {
    "filtering", "call mh_filter_begin first", nullptr,
    {SCORE_KIND_TEXT[0], SCORE_KIND_TEXT[1], SCORE_KIND_TEXT[2], SCORE_KIND_TEXT[3], SCORE_KIND_TEXT[4], nullptr}};

namespace {

constexpr int FG_WAVE_BYTES = 4096;            // output bytes a wave of the gather owns: 4 rounds of 64 x 16 bytes
constexpr int FG_TILE = 4 * FG_WAVE_BYTES;     // ... and a workgroup
constexpr int FG_MIN_REC = 36;                 // a kept record's least size (k_filter_mark keeps nothing smaller)

enum { FC_SEEN = 0, FC_KEPT, FC_DROP_SCORE, FC_DROP_MAPQ, FC_SKIP_TID, FC_SKIP_SMP, FC_BYTES_IN, FC_BYTES_KEPT, FC_N };

struct MarkArgs {
  const uint8_t *recs;
  const int64_t *roff;
  int64_t n, avail;
  ScoreRule rule;
  int32_t d_lo, d_hi, mq_lo, mq_hi, keep_unscored;
  uint32_t *ksz;               // per record: its kept bytes (0: dropped)
  unsigned long long *cnt;     // the chunk's eight counts
  unsigned long long *err;
  int64_t base_rec;
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ void __launch_bounds__(256) k_filter_mark(MarkArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t rows[256 * SC_ROW];
  __shared__ unsigned long long l_cnt[FC_N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < FC_N) l_cnt[threadIdx.x] = 0;
  const int64_t tiles = (a.n + 255) / 256;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();   // the counters are zero / the previous tile's rows are no longer read
    sc_stage_heads(rows, a.recs, a.roff, a.n, a.avail, tile, wave, lane);
    __syncthreads();
    const int64_t t = tile * 256 + threadIdx.x;
    int seen = 0, keep = 0, drop_d = 0, drop_mq = 0, skip_tid = 0, skip_smp = 0;
    int64_t size = 0;
    if (t < a.n) {
      const int64_t s = a.roff[t], e = a.roff[t + 1];
      int32_t kind = 0;
      size = e - s;
      seen = 1;
      if (size < FG_MIN_REC || size > (int64_t)0x7fffffff || s < 0 || e > a.avail) {
        kind = SE_STRUCT;
        size = 0;
      } else {
        const uint8_t *lp = sc_head(rows, a.recs, s, e, a.avail);
        const ScoreRec r = score_record(lp, size, (int32_t)le16(lp + 18), (int32_t)le32(lp + 4),
                                        (int32_t)le32(lp + 8), a.rule);
        kind = r.kind;
        skip_tid = r.skip_tid;
        skip_smp = r.skip_smp;
        if (skip_tid | skip_smp) {
          keep = a.keep_unscored;
        } else if (r.scored) {
          const int32_t ad = r.d_err < 0 ? -r.d_err : r.d_err;
          if (ad < a.d_lo || ad > a.d_hi) drop_d = 1;
          else if (r.mapq < a.mq_lo || r.mapq > a.mq_hi) drop_mq = 1;
          else keep = 1;
        }
      }
      if (kind) rec_fail(a.err, a.base_rec + t, kind);
      a.ksz[t] = keep ? (uint32_t)size : 0u;
    }
    {   // the counts: one LDS add per wave each
      const uint64_t b[6] = {__ballot(seen),     __ballot(keep),     __ballot(drop_d),
                             __ballot(drop_mq), __ballot(skip_tid), __ballot(skip_smp)};
      if (lane < 6 && b[lane]) atomicAdd(&l_cnt[lane], (unsigned long long)__popcll(b[lane]));
      const unsigned long long bi = wave_sum((unsigned long long)size), bk = wave_sum(keep ? (unsigned long long)size : 0);
      if (lane == 0 && bi) atomicAdd(&l_cnt[FC_BYTES_IN], bi);
      if (lane == 1 && bk) atomicAdd(&l_cnt[FC_BYTES_KEPT], bk);
    }
  }
  __syncthreads();
  if (threadIdx.x < FC_N && l_cnt[threadIdx.x]) atomicAdd(&a.cnt[threadIdx.x], l_cnt[threadIdx.x]);
}

// The scan's element: kept bytes and kept records, both summed
struct KB {
  int64_t bytes, recs;
  __host__ __device__ KB operator+(const KB &o) const { return KB{bytes + o.bytes, recs + o.recs}; }
};
struct LoadKept {
  const uint32_t *ksz;
  __device__ KB operator()(int64_t i) const {
    const int64_t b = ksz[i];
    return KB{b, b > 0 ? 1 : 0};
  }
};
// kept record number k (its exclusive record sum) enters the compact list: ksrc[k] its offset in the chunk, kdst[k] its
// offset among the chunk's kept bytes; the last record closes the list with the totals
struct StoreKept {
  const uint32_t *ksz;
  const int64_t *roff;
  int64_t *ksrc, *kdst;
  int64_t n;
  __device__ void operator()(int64_t i, const KB &incl, const KB &excl) const {
    if (ksz[i]) {
      ksrc[excl.recs] = roff[i];
      kdst[excl.recs] = excl.bytes;
    }
    if (i == n - 1) kdst[incl.recs] = incl.bytes;
  }
};

struct GatherArgs {
  const uint8_t *recs;
  int64_t avail;               // bytes readable at recs
  const int64_t *ksrc, *kdst;  // the compact list: kdst has one entry more, the total
  const KB *tot;
  uint8_t *out;                // 16-byte aligned; the chunk's kept bytes go to [carry, carry + tot->bytes)
  int64_t carry;
  const unsigned long long *err;
};

// A wave owns FG_WAVE_BYTES of `out` from a 16-byte boundary and goes over them in rounds of 64 destination-aligned
// 16-byte words, one per lane.  It finds the record under its first byte by a binary search of the compact list, once;
// a lane then finds its own record among the few that can follow inside one round (records are >= 36 bytes): the wave
// loads those list entries once, a lane each, and every lane searches them with shuffles.  A word
// wholly inside one record and inside the chunk's bytes is one 16-byte store, filled from the two aligned 16-byte
// source words under it; the words over a record boundary and the ends of the chunk's bytes are written bytewise.
__global__ void __launch_bounds__(256) k_filter_gather(GatherArgs a) {
  if (*a.err != ~0ull) return;   // a record failed: the chunk is not written
  const int64_t total = a.tot->bytes;
  const int32_t cnt = (int32_t)a.tot->recs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t lo = a.carry, hi = a.carry + total;
  const int64_t p0 = (int64_t)blockIdx.x * FG_TILE + (int64_t)wave * FG_WAVE_BYTES;
  if (cnt <= 0 || p0 + FG_WAVE_BYTES <= lo || p0 >= hi) return;
  int32_t k;   // the record under the wave's first byte: the last with kdst[k] <= that byte (kdst[0] = 0)
  {
    const int64_t d0 = (p0 > lo ? p0 : lo) - lo;
    int32_t l = 0, h = cnt;
    while (h - l > 1) {
      const int32_t mid = l + ((h - l) >> 1);
      if (a.kdst[mid] <= d0) l = mid; else h = mid;
    }
    k = l;
  }
  const uint8_t *const src_end = a.recs + a.avail;
  for (int round = 0; round < FG_WAVE_BYTES / 1024; round++) {
    const int64_t pr = p0 + 1024 * round;   // (wave-uniform)
    if (pr >= hi) break;
    const int64_t p = pr + 16 * lane;
    const bool mine = p + 16 > lo && p < hi;                    // the word holds bytes of this chunk
    const int64_t d = mine ? (p > lo ? p : lo) - lo : 0;        // the lane's first byte among the chunk's kept bytes
    // the list entries the round can need, one per lane (its 1 KiB starts inside record k and meets at most 1040 / 36
    // more): a lane finds its record in them with shuffles, no load waiting on the one before
    const int32_t wi = k + lane < cnt ? k + lane : cnt;
    const int64_t wd = a.kdst[wi], ws = a.ksrc[wi < cnt ? wi : cnt - 1];
    int j = 0;   // the last entry of the window with kdst <= d
#pragma unroll
    for (int step = 16; step >= 1; step >>= 1) {
      const int64_t v = __shfl(wd, j + step, 64);
      if (k + j + step < cnt && v <= d) j += step;
    }
    const int64_t rs = __shfl(wd, j, 64), re = __shfl(wd, j + 1, 64), so = __shfl(ws, j, 64);
    const int32_t kk = k + j;
    if (mine) {
      if (p >= lo && p + 16 <= hi && d + 16 <= re) {
        const uint8_t *sp = a.recs + so + (d - rs);   // [sp, sp + 16) is inside the record
        const uint32_t sh = (uint32_t)((uintptr_t)sp & 15);
        const uint8_t *ap = sp - sh;
        uint4 v;
        if (sh == 0) {
          v = *(const uint4 *)ap;
        } else if (ap >= a.recs && ap + 32 <= src_end) {
          const uint4 A = *(const uint4 *)ap, B = *(const uint4 *)(ap + 16);
          uint64_t x0 = (uint64_t)A.x | (uint64_t)A.y << 32, x1 = (uint64_t)A.z | (uint64_t)A.w << 32;
          uint64_t x2 = (uint64_t)B.x | (uint64_t)B.y << 32;
          const uint64_t x3 = (uint64_t)B.z | (uint64_t)B.w << 32;
          if (sh & 8) { x0 = x1; x1 = x2; x2 = x3; }
          const uint32_t r = (sh & 7) * 8;
          if (r) {
            x0 = x0 >> r | x1 << (64 - r);
            x1 = x1 >> r | x2 << (64 - r);
          }
          v = make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32));
        } else {   // the aligned words would leave [recs, recs + avail)
          uint32_t w[4] = {0, 0, 0, 0};
          for (int i = 0; i < 16; i++) w[i >> 2] |= (uint32_t)sp[i] << (8 * (i & 3));
          v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4 *)(a.out + p) = v;
      } else {
        const int64_t q1 = p + 16 < hi ? p + 16 : hi;
        int32_t kb = kk;
        for (int64_t q = p > lo ? p : lo; q < q1; q++) {
          const int64_t dd = q - lo;
          while (dd >= a.kdst[kb + 1]) kb++;   // (dd < total = kdst[cnt])
          a.out[q] = a.recs[a.ksrc[kb] + (dd - a.kdst[kb])];
        }
      }
    }
    k = __shfl(kk, 63, 64);   // the next round starts at or behind the last lane's record
  }
}

// the sink's failure as a call's result: a failed copy, or a failed write naming the path (MH_OK: neither)
int32_t sink_failed(mh_ctx *ctx, FilterState &F) {
  if (F.sink.hip_error() != hipSuccess) return hip_fail(ctx, F.sink.hip_error(), "filter-bam D2H", __FILE__, __LINE__);
  if (!F.sink.failed()) return MH_OK;
  const char *what = F.sink.close_failed ? "filter-bam: close failed: " : "filter-bam: write failed: ";
  return arg_fail(ctx, MH_E_IO, what + F.sink.path);
}

// out[cur][0, n) (whole blocks, or the last carry) deflated into z and pushed to the sink, once the sink has copied the
// previous chunk's blocks out of z.  A failed sink takes nothing more (the add call and finish report it)
int32_t deflate_out(mh_ctx *ctx, FilterState &F, int64_t n) {
  hipStream_t st = ctx->stream;
  int64_t used = 0;
  if (!F.sink.wait_copied(F.sink.mark())) return MH_OK;
  MH_TRY(ensure(ctx, F.z, (size_t)bgzf_device_bound(n)));
  {
    StageScope sc(ctx, "filter_deflate");
    MH_TRY(bgzf_device(ctx, st, (const uint8_t *)F.out[F.cur].p, n, (uint8_t *)F.z.p, (int64_t)F.z.cap, &used));
  }
  F.sink.push(F.z.p, used, st);
  return MH_OK;
}

int32_t filter_launch(mh_ctx *ctx, const RecChunk &c) {
  FilterState &F = ctx->filter;
  hipStream_t st = ctx->stream;
  if (F.failed || F.sink.failed()) return MH_OK;   // nothing of a later chunk is written
  const int64_t n = c.n;
  MH_TRY(ensure(ctx, F.ksz, sizeof(uint32_t) * (size_t)n + 64));
  MH_TRY(ensure(ctx, F.klist, sizeof(int64_t) * (size_t)(2 * n + 1) + 64));
  MH_TRY(ensure(ctx, F.scan, scan_lb_scratch_bytes<KB>(n)));
  // [carry | this chunk's kept bytes], and room for the last 16-byte word
  MH_TRY(ensure_keep(ctx, F.out[F.cur], (size_t)(F.carry + c.avail + 64), (size_t)F.carry));
  uint32_t *ksz = (uint32_t *)F.ksz.p;
  int64_t *kdst = (int64_t *)F.klist.p, *ksrc = kdst + n + 1;
  KB *tot = (KB *)F.tot.p;
  unsigned long long *err = (unsigned long long *)F.ses.err.p;
  HIPCHK(ctx, hipMemsetAsync(F.delta.p, 0, sizeof(uint64_t) * FC_N, st));
  HIPCHK(ctx, hipMemsetAsync(tot, 0, sizeof(KB), st));
  const int64_t tiles = (n + 255) / 256;
  {
    StageScope sc(ctx, "filter_mark");
    MarkArgs a{c.recs, c.roff, n, c.avail, F.refs.rule(F.max_d, F.strict), F.d_lo, F.d_hi, F.mq_lo, F.mq_hi,
               F.keep_unscored, ksz, (unsigned long long *)F.delta.p, err, c.base_rec};
    const int64_t grid = std::min<int64_t>(tiles, 8 * (int64_t)ctx->max_cu);
    hipLaunchKernelGGL(k_filter_mark, dim3((unsigned)grid), dim3(256), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
  }
  {
    StageScope sc(ctx, "filter_scan");
    HIPCHK(ctx, device_scan_sum<KB>(st, n, LoadKept{ksz}, StoreKept{ksz, c.roff, ksrc, kdst, n}, F.scan.p, tot));
  }
  {
    StageScope sc(ctx, "filter_gather");
    // (the kept bytes are known on the device only: workgroups past them return)
    const int64_t grid = (F.carry + c.avail + FG_TILE - 1) / FG_TILE;
    GatherArgs g{c.recs, c.avail, ksrc, kdst, tot, (uint8_t *)F.out[F.cur].p, F.carry, err};
    hipLaunchKernelGGL(k_filter_gather, dim3((unsigned)grid), dim3(256), 0, st, g);
    HIPCHK(ctx, hipGetLastError());
  }
  MH_TRY(session_commit(ctx, F.ses, F.delta, F.acc, FC_N, FC_N));
  HIPCHK(ctx, hipMemcpyAsync(F.h_rb, tot, sizeof(KB), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(F.h_rb + 2, err, 8, hipMemcpyDeviceToHost, st));
  // (the sink's thread writes the previous chunk's compressed bytes while the device works on this one)
  SYNCCHK(ctx, hipStreamSynchronize(st));
  if ((uint64_t)F.h_rb[2] != ~(uint64_t)0) {
    F.failed = true;
    return MH_OK;
  }
  const int64_t T = F.carry + F.h_rb[0];
  const int64_t whole = T / BGZF_BLOCK * BGZF_BLOCK;
  if (whole == 0) {
    F.carry = T;
    return MH_OK;
  }
  MH_TRY(deflate_out(ctx, F, whole));
  // what is left starts the other buffer: the next chunk's carry
  const int64_t rem = T - whole;
  MH_TRY(ensure(ctx, F.out[F.cur ^ 1], (size_t)rem + 64));
  if (rem > 0)
    HIPCHK(ctx, hipMemcpyAsync(F.out[F.cur ^ 1].p, (const uint8_t *)F.out[F.cur].p + whole, (size_t)rem,
                               hipMemcpyDeviceToDevice, st));
  F.cur ^= 1;
  F.carry = rem;
  return MH_OK;
}

// the sink stopped, the session's unfinished file closed and removed (when it is a regular file): the state a new
// begin starts from
void filter_drop(FilterState &F) {
  F.sink.abort();
  struct stat sb;
  if (F.unfinished && stat(F.sink.path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) (void)unlink(F.sink.path.c_str());
  F.unfinished = false;
  F.ses.begun = false;
}

}  // namespace

int32_t filter_begin(mh_ctx *ctx, int32_t n_refs, const char *names, const int64_t *lengths, const char *header_text,
                     int64_t header_len, const char *out_path, int32_t max_d, int32_t strict,
                     const char *sample_prefix, int32_t d_lo, int32_t d_hi, int32_t mq_lo, int32_t mq_hi,
                     int32_t keep_unscored) {
  FilterState &F = ctx->filter;
  if (!out_path || !*out_path || header_len < 0 || (header_len > 0 && !header_text))
    return arg_fail(ctx, MH_E_ARG, "null argument");
  if (n_refs < 0 || (n_refs > 0 && (!names || !lengths))) return arg_fail(ctx, MH_E_ARG, "bad reference list");
  if (max_d < 0 || max_d > (1 << 20)) return arg_fail(ctx, MH_E_ARG, "max_d must be 0..2^20");
  if (d_lo < 0 || d_lo > d_hi || d_hi > max_d) return arg_fail(ctx, MH_E_ARG, "need 0 <= d_lo <= d_hi <= max_d");
  if (mq_lo < 0 || mq_lo > mq_hi || mq_hi > 255) return arg_fail(ctx, MH_E_ARG, "need 0 <= mq_lo <= mq_hi <= 255");
  filter_drop(F);   // a session left open: as mh_filter_abort
  std::vector<std::string> ref_names;
  std::vector<int64_t> ref_len;
  const char *p = names;
  for (int32_t i = 0; i < n_refs; i++) {
    ref_names.emplace_back(p);
    ref_len.push_back(lengths[i]);
    p += ref_names.back().size() + 1;
  }
  F.max_d = max_d;
  F.strict = strict ? 1 : 0;
  F.d_lo = d_lo;
  F.d_hi = d_hi;
  F.mq_lo = mq_lo;
  F.mq_hi = mq_hi;
  F.keep_unscored = keep_unscored ? 1 : 0;
  F.failed = false;
  F.carry = 0;
  F.cur = 0;
  hipStream_t st = ctx->stream;
  if (!F.h_rb) HIPCHK(ctx, hipHostMalloc((void **)&F.h_rb, 64, hipHostMallocDefault));
  MH_TRY(ensure(ctx, F.acc, sizeof(uint64_t) * FC_N));
  MH_TRY(ensure(ctx, F.delta, sizeof(uint64_t) * FC_N));
  MH_TRY(ensure(ctx, F.tot, 64));
  MH_TRY(F.refs.upload(ctx, n_refs, names, sample_prefix));
  MH_TRY(session_clear(ctx, F.ses));
  HIPCHK(ctx, hipMemsetAsync(F.acc.p, 0, sizeof(uint64_t) * FC_N, st));
  SYNCCHK(ctx, hipStreamSynchronize(st));   // (the session's cleared state is in place before a file is made)
  // the header, deflated by the sink in its own block(s); the records start a fresh block behind it
  const std::string hdr = bam_header_bytes(std::string(header_text ? header_text : "", (size_t)header_len), ref_names,
                                           ref_len);
  int64_t data_pos = 0;
  F.unfinished = true;   // (a file the open created and could not write is removed as well)
  if (!F.sink.open(ctx, out_path, &hdr, 6, &data_pos)) {
    const int32_t rc = F.sink.hip_error() != hipSuccess
                           ? sink_failed(ctx, F)
                           : arg_fail(ctx, MH_E_IO, "filter-bam: cannot write " + F.sink.path + ": " + F.sink.io_error());
    filter_drop(F);
    return rc;
  }
  F.ses.begun = true;
  return MH_OK;
}

int32_t filter_add_records(mh_ctx *ctx, const uint8_t *recs, int64_t len, const int64_t *roff, int64_t n) {
  FilterState &F = ctx->filter;
  MH_TRY(session_add_records(ctx, F.ses, recs, len, roff, n, [ctx](const RecChunk &c) { return filter_launch(ctx, c); }));
  return sink_failed(ctx, F);
}

int32_t filter_finish(mh_ctx *ctx, int64_t *counts) {
  FilterState &F = ctx->filter;
  MH_TRY(session_begun(ctx, F.ses));
  int32_t rc = MH_OK;
  if (!F.failed && !F.sink.failed()) {
    if (F.carry > 0) rc = deflate_out(ctx, F, F.carry);   // the carry is the last block
    if (rc == MH_OK && F.sink.finish(true, nullptr) && ctx->timing) {
      ctx->last_times.emplace_back("filter_d2h", F.sink.d2h_ms);
      ctx->last_times.emplace_back("filter_write", F.sink.write_ms);
    }
  }
  std::string failed;
  const int32_t rc_s = session_failed(ctx, F.ses, &failed);   // (waits for the stream)
  if (rc == MH_OK) rc = rc_s;
  if (rc == MH_OK) rc = sink_failed(ctx, F);
  if (rc == MH_OK && !failed.empty()) rc = arg_fail(ctx, MH_E_ARG, failed);
  if (rc == MH_OK && counts) {
    if (hipMemcpyAsync(counts, F.acc.p, sizeof(int64_t) * FC_N, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
      rc = hip_fail(ctx, hipGetLastError(), "filter counts D2H", __FILE__, __LINE__);
  }
  if (rc != MH_OK) {
    filter_drop(F);
    return rc;
  }
  F.unfinished = false;
  F.ses.begun = false;
  return MH_OK;
}

int32_t filter_abort(mh_ctx *ctx) {
  FilterState &F = ctx->filter;
  SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
  filter_drop(F);
  return MH_OK;
}

void filter_release(FilterState &F) {
  filter_drop(F);   // (a session still open when its context goes: aborted)
  F.sink.release();
  release(F.acc); release(F.delta); release(F.ksz); release(F.klist); release(F.scan); release(F.tot); release(F.z);
  F.refs.release();
  for (DevBuf &b : F.out) release(b);
  if (F.h_rb) (void)hipHostFree(F.h_rb);
  F.h_rb = nullptr;
  session_release(F.ses);
}

}  // namespace mh
