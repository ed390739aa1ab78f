// mh_recs.hip — the host side of the record sessions' shared core (mh_recs.h): host records staged through two
// page-locked buffers, the session envelope around a consumer's kernels, and the commit of a chunk's sums.
#include <cstring>

#include "mh_bamread.h"
#include "mh_internal.h"

namespace mh {
namespace {

struct StagedRecs {
  const uint8_t *recs;         // device: the records, 64 zero bytes behind them
  const int64_t *roff;         // device: n + 1 offsets from recs
  int64_t avail;               // bytes readable at recs
  int slot;
};

// its events exist; the chunks in flight are done
int32_t stage_init(mh_ctx *ctx, RecStage &G) {
  for (int k = 0; k < 2; k++) {
    if (!G.ev[k]) HIPCHK(ctx, hipEventCreateWithFlags(&G.ev[k], hipEventDisableTiming));
    if (G.ev_set[k]) {
      HIPCHK(ctx, hipEventSynchronize(G.ev[k]));
      G.ev_set[k] = false;
    }
  }
  return MH_OK;
}

// the n records checked (a failure names record base_rec + i), copied with their offsets into the free page-locked
// buffer and queued for upload; the caller queues its kernels on ctx->stream, then calls stage_queued(out->slot)
int32_t stage_records(mh_ctx *ctx, RecStage &G, const uint8_t *recs, int64_t len, const int64_t *roff, int64_t n,
                      int64_t base_rec, StagedRecs *out) {
  // the same structural check the reader applies: nothing malformed reaches the device
  if (roff[0] < 0 || roff[n] > len) return arg_fail(ctx, MH_E_ARG, "record offsets outside the buffer");
  for (int64_t i = 0; i < n; i++) {
    std::string why;
    if (roff[i + 1] < roff[i] || roff[i + 1] > len || !bam_record_ok(recs + roff[i], roff[i + 1] - roff[i], &why))
      return arg_fail(ctx, MH_E_ARG, "malformed BAM record " + std::to_string(base_rec + i) + ": " +
                                         (why.empty() ? "record offsets decrease" : why));
  }
  const int k = G.cur;
  if (G.ev_set[k]) {   // the chunk staged here two calls ago has been worked through
    HIPCHK(ctx, hipEventSynchronize(G.ev[k]));
    G.ev_set[k] = false;
  }
  const int64_t bytes = roff[n] - roff[0];
  const size_t o_recs = ((size_t)(n + 1) * 8 + 15) & ~(size_t)15, need = o_recs + (size_t)bytes + 64;
  if (G.pin_cap[k] < need) {
    if (G.pin[k]) (void)hipHostFree(G.pin[k]);
    G.pin[k] = nullptr;
    G.pin_cap[k] = 0;
    const size_t cap = need + need / 4;
    HIPCHK(ctx, hipHostMalloc((void **)&G.pin[k], cap, hipHostMallocDefault));
    G.pin_cap[k] = cap;
  }
  int64_t *po = (int64_t *)G.pin[k];
  for (int64_t i = 0; i <= n; i++) po[i] = roff[i] - roff[0];
  memcpy(G.pin[k] + o_recs, recs + roff[0], (size_t)bytes);
  memset(G.pin[k] + o_recs + bytes, 0, 64);
  MH_TRY(ensure(ctx, G.in[k], need));
  HIPCHK(ctx, hipMemcpyAsync(G.in[k].p, G.pin[k], need, hipMemcpyHostToDevice, ctx->stream));
  *out = StagedRecs{(const uint8_t *)G.in[k].p + o_recs, (const int64_t *)G.in[k].p, bytes + 64, k};
  return MH_OK;
}

int32_t stage_queued(mh_ctx *ctx, RecStage &G, int slot) {
  HIPCHK(ctx, hipEventRecord(G.ev[slot], ctx->stream));
  G.ev_set[slot] = true;
  G.cur = slot ^ 1;
  return MH_OK;
}

void stage_release(RecStage &G) {
  for (int k = 0; k < 2; k++) {
    release(G.in[k]);
    if (G.pin[k]) (void)hipHostFree(G.pin[k]);
    if (G.ev[k]) (void)hipEventDestroy(G.ev[k]);
    G.pin[k] = nullptr;
    G.pin_cap[k] = 0;
    G.ev[k] = nullptr;
    G.ev_set[k] = false;
  }
}

__global__ void k_commit(const unsigned long long *delta, unsigned long long *acc, int64_t n, int64_t i_max,
                         const unsigned long long *err) {
  if (*err != ~0ull) return;   // a record failed: nothing of this chunk, or of any later one, is kept
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!delta[i]) continue;
    if (i == i_max || i == i_max + 1) acc[i] = max(acc[i], delta[i]);
    else acc[i] += delta[i];
  }
}

}  // namespace

int32_t session_begun(mh_ctx *ctx, const RecSession &S) {
  return S.begun ? MH_OK : arg_fail(ctx, MH_E_STATE, S.texts->begin_first);
}

int32_t session_clear(mh_ctx *ctx, RecSession &S) {
  MH_TRY(stage_init(ctx, S.stage));
  MH_TRY(ensure(ctx, S.err, 64));
  HIPCHK(ctx, hipMemsetAsync(S.err.p, 0xff, 8, ctx->stream));
  S.base_rec = 0;
  return MH_OK;
}

int32_t session_add_records(mh_ctx *ctx, RecSession &S, const uint8_t *recs, int64_t len, const int64_t *roff,
                            int64_t n, const RecLaunch &launch) {
  MH_TRY(session_begun(ctx, S));
  if (n == 0) return MH_OK;
  StagedRecs d;
  MH_TRY(stage_records(ctx, S.stage, recs, len, roff, n, S.base_rec, &d));
  MH_TRY(launch(RecChunk{d.recs, d.roff, n, d.avail, S.base_rec, nullptr}));
  S.base_rec += n;
  return stage_queued(ctx, S.stage, d.slot);
}

int32_t session_add_store(mh_ctx *ctx, RecSession &S, const RecLaunch &launch) {
  const BamStore &B = ctx->bam;
  MH_TRY(session_begun(ctx, S));
  if (!B.refs_set) return arg_fail(ctx, MH_E_STATE, "call mh_bam_set_refs first");
  if (B.n_rec == 0) return MH_OK;
  if (B.spilled > 0) return arg_fail(ctx, MH_E_STATE, S.texts->spilled);
  // a direct sorted write keeps the records in coordinate order only
  const uint8_t *recs = (const uint8_t *)(B.direct ? B.srecs.p : B.recs.p);
  const int64_t *roff = (const int64_t *)(B.direct ? B.soff.p : B.roff.p);
  MH_TRY(launch(RecChunk{recs, roff, B.n_rec, B.bytes, S.base_rec, &B}));
  S.base_rec += B.n_rec;
  SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

int32_t session_commit(mh_ctx *ctx, const RecSession &S, const DevBuf &delta, DevBuf &acc, int64_t n, int64_t i_max) {
  hipLaunchKernelGGL(k_commit, dim3(grid_for(n, 256, 1024)), dim3(256), 0, ctx->stream,
                     (const unsigned long long *)delta.p, (unsigned long long *)acc.p, n, i_max,
                     (const unsigned long long *)S.err.p);
  HIPCHK(ctx, hipGetLastError());
  return MH_OK;
}

int32_t session_failed(mh_ctx *ctx, const RecSession &S, std::string *msg) {
  uint64_t herr = 0;
  HIPCHK(ctx, hipMemcpyAsync(&herr, S.err.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  SYNCCHK(ctx, hipStreamSynchronize(ctx->stream));
  msg->clear();
  if (herr != ~(uint64_t)0) {
    const int kind = (int)(herr & 15);
    *msg = std::string(S.texts->label) + ": record " + std::to_string(herr >> 4) + ": " +
           (kind >= 1 && kind <= 5 && S.texts->kind[kind] ? S.texts->kind[kind] : "unknown failure");
  }
  return MH_OK;
}

void session_release(RecSession &S) {
  release(S.err);
  stage_release(S.stage);
  S.begun = false;
}

int32_t RefNames::upload(mh_ctx *ctx, int32_t n, const char *ref_names, const char *sample_prefix) {
  std::vector<int32_t> off(1, 0);
  std::string cat;
  const char *p = ref_names;
  for (int32_t i = 0; i < n; i++) {
    const size_t l = strlen(p);
    cat.append(p, l);
    p += l + 1;
    off.push_back((int32_t)cat.size());
  }
  const std::string pre = sample_prefix ? sample_prefix : "";
  n_refs = n;
  plen = (int32_t)pre.size();
  hipStream_t st = ctx->stream;
  MH_TRY(ensure(ctx, names, cat.size() + 16));
  MH_TRY(ensure(ctx, name_off, sizeof(int32_t) * off.size()));
  MH_TRY(ensure(ctx, prefix, pre.size() + 16));
  if (!cat.empty()) HIPCHK(ctx, hipMemcpyAsync(names.p, cat.data(), cat.size(), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(name_off.p, off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice, st));
  if (!pre.empty()) HIPCHK(ctx, hipMemcpyAsync(prefix.p, pre.data(), pre.size(), hipMemcpyHostToDevice, st));
  SYNCCHK(ctx, hipStreamSynchronize(st));   // (the host strings above are done with)
  return MH_OK;
}

void RefNames::release() {
  mh::release(names);
  mh::release(name_off);
  mh::release(prefix);
}

}  // namespace mh
