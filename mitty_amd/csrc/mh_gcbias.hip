// mh_gcbias.hip — GC-bias thinning of a unit's sampled templates (generate-reads --gc-bias; mitty_hip.h mh_gc_thin).
//
//   k_gc_flag    per template the 'G' / 'C' bytes (upper case only, as gc-cov counts) of the haplotype bytes it spans,
//                a quarter wave per template: 16-byte loads over the aligned middle of the span, bytes at its ragged
//                ends, SWAR byte compares (count_eq4, as k_cov_gc) and a shuffle reduction inside the 16 lanes;
//                then the bin, the Philox draw of the template's index and a one-byte keep flag.  Templates seen and
//                kept per bin in 2 x 101 LDS cells per workgroup, flushed with 64-bit global atomic adds.
//   compaction   one device_scan over the flags whose Store moves fo0 / pos0 / pos1 / n0 to fresh buffers at the
//                exclusive index (out of place: the kept templates keep their relative order).
// The haplotype bytes are read where they are (Hap::hap); nothing is added to the slot.
#include <utility>

#include "mh_corrupt.h"
#include "mh_device.h"
#include "mh_internal.h"
#include "mh_scan.h"

using namespace mh;

namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_GROUP = 16;                        // lanes per template (a quarter wave)
constexpr int GC_PER_BLOCK = GC_THREADS / GC_GROUP;   // templates a workgroup counts at a time

struct GcKey {
  uint32_t k0, k1, c3;
};

// acc: seen[MH_GC_BINS] | kept[MH_GC_BINS].  Every read of hap is inside [0, hap_len): the span is clamped to it.
__global__ void __launch_bounds__(GC_THREADS) k_gc_flag(const uint8_t *hap, int64_t hap_len, int64_t p_min, int64_t n,
                                                        const int64_t *pos0, const int64_t *pos1, int64_t rlen,
                                                        const uint64_t *accept, GcKey key, uint8_t *keep,
                                                        unsigned long long *acc) {
  __shared__ uint32_t s_hist[2 * MH_GC_BINS];
  __shared__ uint64_t s_acc[MH_GC_BINS];
  for (int i = threadIdx.x; i < 2 * MH_GC_BINS; i += GC_THREADS) s_hist[i] = 0;
  for (int i = threadIdx.x; i < MH_GC_BINS; i += GC_THREADS) s_acc[i] = accept[i];
  __syncthreads();
  const int gl = threadIdx.x & (GC_GROUP - 1);
  const int64_t grp = (int64_t)blockIdx.x * GC_PER_BLOCK + (threadIdx.x / GC_GROUP);
  const int64_t ngrp = (int64_t)gridDim.x * GC_PER_BLOCK;
  for (int64_t t = grp; t < n; t += ngrp) {   // (uniform over the 16 lanes of a group)
    int64_t s = pos0[t] - p_min, e = pos1[t] + rlen - p_min;
    s = s < 0 ? 0 : s > hap_len ? hap_len : s;
    e = e < s ? s : e > hap_len ? hap_len : e;
    const uint8_t *b = hap + s;
    const int64_t len = e - s;
    // 16-byte pieces on the buffer's own alignment: piece j covers span bytes [16 j - mis, 16 j - mis + 16)
    const int64_t mis = (int64_t)((uintptr_t)b & 15);
    int g = 0;
    for (int64_t lo = 16 * (int64_t)gl - mis; lo < len; lo += 16 * GC_GROUP) {
      if (lo >= 0 && lo + 16 <= len) {
        const uint4 v = *reinterpret_cast<const uint4 *>(b + lo);
        g += count_eq4(v.x, 'G') + count_eq4(v.x, 'C') + count_eq4(v.y, 'G') + count_eq4(v.y, 'C') +
             count_eq4(v.z, 'G') + count_eq4(v.z, 'C') + count_eq4(v.w, 'G') + count_eq4(v.w, 'C');
      } else {
        const int64_t x1 = lo + 16 < len ? lo + 16 : len;
        for (int64_t x = lo < 0 ? 0 : lo; x < x1; x++) {
          const uint8_t ch = b[x];
          g += ch == 'G' || ch == 'C';
        }
      }
    }
#pragma unroll
    for (int d = GC_GROUP / 2; d >= 1; d >>= 1) g += __shfl_xor(g, d, 64);   // (partners stay inside the group)
    if (gl == 0) {
      const int bin = len > 0 ? (int)((100 * (int64_t)g) / len) : 0;
      const uint32_t u = philox4x32_10(make_uint4((uint32_t)t, (uint32_t)((uint64_t)t >> 32), 0u, key.c3),
                                       make_uint2(key.k0, key.k1)).x;
      const bool k = (uint64_t)u < s_acc[bin];
      keep[t] = k ? 1 : 0;
      atomicAdd(&s_hist[bin], 1u);
      if (k) atomicAdd(&s_hist[MH_GC_BINS + bin], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * MH_GC_BINS; i += GC_THREADS)
    if (s_hist[i]) atomicAdd(&acc[i], (unsigned long long)s_hist[i]);
}

struct LoadFlag {
  const uint8_t *keep;
  __device__ int64_t operator()(int64_t i) const { return keep[i]; }
};
struct StoreThin {
  const uint8_t *keep;
  const int8_t *fo0;
  const int64_t *pos0, *pos1;
  const int32_t *n0;   // null: the set carries no start nodes
  int8_t *o_fo0;
  int64_t *o_pos0, *o_pos1;
  int32_t *o_n0;
  __device__ void operator()(int64_t i, int64_t, int64_t ex) const {
    if (!keep[i]) return;
    o_fo0[ex] = fo0[i];
    o_pos0[ex] = pos0[i];
    o_pos1[ex] = pos1[i];
    if (n0) o_n0[ex] = n0[i];
  }
};

}  // namespace

int32_t mh_gc_thin(mh_ctx *ctx, int32_t tpl_id, int32_t slot, const uint64_t *accept, uint64_t seed,
                   uint64_t unit_key, int64_t *out_n, int64_t *bin_seen, int64_t *bin_kept) {
  if (!ctx) return MH_E_ARG;
  scan_fault_slot = ctx->fault_slot;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  auto it = ctx->tsets.find(tpl_id);
  if (it == ctx->tsets.end()) return arg_fail(ctx, MH_E_STATE, "unknown template set");
  TplSet &ts = it->second;
  MH_TRY(tpl_resolve(ctx, ts));
  if (!ts.valid) return arg_fail(ctx, MH_E_STATE, "unknown template set");
  auto hit = ctx->haps.find(slot);
  if (hit != ctx->haps.end() && hit->second.prefetched) MH_TRY(join_prefetch(ctx));
  if (hit == ctx->haps.end() || !hit->second.valid) return arg_fail(ctx, MH_E_STATE, "empty haplotype slot");
  const Hap &h = hit->second;
  if (!accept) return arg_fail(ctx, MH_E_ARG, "null argument");
  for (int b = 0; b < MH_GC_BINS; b++)
    if (accept[b] > ((uint64_t)1 << 32)) return arg_fail(ctx, MH_E_ARG, "gc-bias threshold above 2^32");
  // once, before any emission of the set: a measure pass made for it, or a writer still queued on it (the sampling
  // or import that filled the set already waited for every earlier writer), would read the arrays replaced here
  if (ts.prep.valid || (ts.used_set && hipEventQuery(ts.used) != hipSuccess))
    return arg_fail(ctx, MH_E_STATE, "mh_gc_thin: the template set is already being emitted");

  hipStream_t st = ctx->stream;
  const int64_t n = ts.n;
  int64_t hist[2 * MH_GC_BINS] = {0};
  int64_t kept = 0;
  if (n > 0) {
    // [seen | kept | total | accept] then the flags
    constexpr size_t HDR = 8 * (2 * MH_GC_BINS + 1 + MH_GC_BINS) + 8;
    MH_TRY(ensure(ctx, ctx->gc_buf, HDR + (size_t)n + 16));
    MH_TRY(ensure(ctx, ctx->scan_partials, 8 * (size_t)scan_partials_count(n) + 64));
    // the arrays compacted into, with the slack the other producers leave; grown as an import grows a set's arrays
    DevBuf &nf = ctx->gc_out[0], &np0 = ctx->gc_out[1], &np1 = ctx->gc_out[2], &nn0 = ctx->gc_out[3];
    MH_TRY(ensure(ctx, nf, (size_t)n + 16));
    MH_TRY(ensure(ctx, np0, 8 * ((size_t)n + 16)));
    MH_TRY(ensure(ctx, np1, 8 * ((size_t)n + 16)));
    if (ts.has_n0) MH_TRY(ensure(ctx, nn0, 4 * ((size_t)n + 16)));
    unsigned long long *d_hist = (unsigned long long *)ctx->gc_buf.p;
    int64_t *d_tot = (int64_t *)(d_hist + 2 * MH_GC_BINS);
    uint64_t *d_acc = (uint64_t *)(d_tot + 1);
    uint8_t *d_keep = (uint8_t *)ctx->gc_buf.p + HDR;
    const GcKey key{(uint32_t)seed, (uint32_t)unit_key,
                    (uint32_t)(seed >> 32) ^ (uint32_t)(unit_key >> 32) ^ 0x67636269u};
    hipError_t e = hipMemsetAsync(d_hist, 0, 8 * (2 * MH_GC_BINS + 1), st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_acc, accept, 8 * MH_GC_BINS, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
      StageScope stage(ctx, "gc_flag");
      hipLaunchKernelGGL(k_gc_flag, dim3(grid_for(n, GC_PER_BLOCK, 8 * (int64_t)ctx->max_cu)), dim3(GC_THREADS), 0, st,
                         (const uint8_t *)h.hap.p, h.hap_len, h.p_min, n, (const int64_t *)ts.pos0.p,
                         (const int64_t *)ts.pos1.p, (int64_t)ts.rlen, (const uint64_t *)d_acc, key, d_keep, d_hist);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      StageScope stage(ctx, "gc_compact");
      e = device_scan<int64_t>(st, n, LoadFlag{d_keep},
                               StoreThin{d_keep, (const int8_t *)ts.fo0.p, (const int64_t *)ts.pos0.p,
                                         (const int64_t *)ts.pos1.p, ts.has_n0 ? (const int32_t *)ts.n0.p : nullptr,
                                         (int8_t *)nf.p, (int64_t *)np0.p, (int64_t *)np1.p, (int32_t *)nn0.p},
                               OpSum{}, (int64_t)0, (int64_t *)ctx->scan_partials.p, d_tot);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hist, d_hist, 8 * 2 * MH_GC_BINS, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&kept, d_tot, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(ctx, e, "mh_gc_thin", __FILE__, __LINE__);
    if (scan_fault_pending(ctx)) return scan_fault_fail(ctx);
    // the stream is drained and no writer reads the set's old arrays: they take the next call's compaction
    std::swap(ts.fo0, nf);
    std::swap(ts.pos0, np0);
    std::swap(ts.pos1, np1);
    if (ts.has_n0) std::swap(ts.n0, nn0);
    ts.n = kept;
  }
  if (out_n) *out_n = kept;
  for (int b = 0; b < MH_GC_BINS; b++) {
    if (bin_seen) bin_seen[b] = hist[b];
    if (bin_kept) bin_kept[b] = hist[MH_GC_BINS + b];
  }
  return MH_OK;
}
