// mh_recs.h — what the sessions that consume BAM records (mh_score.hip, mh_model.hip, mh_cov.hip) share: the envelope
// of a session (begun, the records counted so far, the first failing record, the staging of host records) and the
// device helpers of their record kernels.  Included by mh_internal.h, after DevBuf and BamStore and before the
// sessions' states, which embed a RecSession; sources include mh_internal.h.
#pragma once

namespace mh {

// Host BAM records on their way to the device: two page-locked buffers, so chunk k + 1 is checked and copied while
// chunk k is worked on (stage_records in mh_recs.hip).
struct RecStage {
  DevBuf in[2];                // the chunk on the device: record offsets, then the records
  uint8_t *pin[2] = {nullptr, nullptr};   // page-locked staging, one per chunk in flight
  size_t pin_cap[2] = {0, 0};
  hipEvent_t ev[2] = {nullptr, nullptr};  // after the kernels of the chunk staged in pin[k]
  bool ev_set[2] = {false, false};
  int cur = 0;
};

// A session's words: they differ between the sessions and are part of their interface.
struct RecTexts {
  const char *label;           // "<label>: record N: <what>"
  const char *begin_first;     // a call before the session's begin
  const char *spilled;         // add_store on a store whose records have left HBM
  const char *kind[6];         // <what>, by the kind a kernel gave rec_fail (1 .. 5; unused ones null)
};

struct RecSession {
  const RecTexts *texts;
  bool begun = false;
  int64_t base_rec = 0;        // records given to earlier calls (names a failing record)
  DevBuf err;                  // u64: min over failing records of (record index << 4 | kind), ~0 = none
  RecStage stage;
  explicit RecSession(const RecTexts &t) : texts(&t) {}
};

// Records at a device address, from some source: a staged host chunk (store null) or the god-aligner store.
struct RecChunk {
  const uint8_t *recs;
  const int64_t *roff;         // n + 1 offsets from recs
  int64_t n, avail, base_rec;  // records; bytes readable at recs; the session's index of record 0
  const BamStore *store;
};
using RecLaunch = std::function<int32_t(const RecChunk &)>;   // the consumer's kernels over a chunk, on ctx->stream

// What the sessions that score records (mh_score.hip, mh_filter.hip) keep of the header on the device: the reference
// names, concatenated with their offsets, and the sample prefix
struct ScoreRule;   // mh_scorerec.h, where rule() is defined
struct RefNames {
  DevBuf names, name_off, prefix;
  int32_t n_refs = 0, plen = 0;
  // names: n_refs strings, each ending in NUL; sample_prefix may be null.  Returns with the copies done
  int32_t upload(mh_ctx *ctx, int32_t n_refs, const char *names, const char *sample_prefix);
  ScoreRule rule(int32_t max_d, int32_t strict) const;
  void release();
};

int32_t session_begun(mh_ctx *ctx, const RecSession &S);   // MH_E_STATE with the session's text when it is not
// the chunks in flight done, no failing record, no records counted; queued on ctx->stream (the caller synchronises)
int32_t session_clear(mh_ctx *ctx, RecSession &S);
// host records checked as the reader checks them (bam_record_ok; a failure names the session's record index), staged
// and launched; returns with the kernels queued
int32_t session_add_records(mh_ctx *ctx, RecSession &S, const uint8_t *recs, int64_t len, const int64_t *roff,
                            int64_t n, const RecLaunch &launch);
// the context's record store launched where it lies (input order, or coordinate order after a direct sorted write),
// then waited for
int32_t session_add_store(mh_ctx *ctx, RecSession &S, const RecLaunch &launch);
// the chunk's sums join the session's unless a record of this or an earlier chunk failed: acc[i] += delta[i], but
// cells i_max and i_max + 1 are maxima (i_max = n: no such cells)
int32_t session_commit(mh_ctx *ctx, const RecSession &S, const DevBuf &delta, DevBuf &acc, int64_t n, int64_t i_max);
// the session's work waited for; *msg = "<label>: record N: <what>" of the first failing record, or empty
int32_t session_failed(mh_ctx *ctx, const RecSession &S, std::string *msg);
void session_release(RecSession &S);

// ---- device side of the record kernels ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t le32(const uint8_t *p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// record t of a chunk: *s its offset, *size its bytes; true when its 36 fixed bytes lie inside [roff[t], roff[t + 1])
// and inside `avail`
__device__ __forceinline__ bool rec_span(const int64_t *roff, int64_t t, int64_t avail, int64_t *s, int64_t *size) {
  const int64_t e = roff[t + 1];
  *s = roff[t];
  *size = e - *s;
  return !(*size < 36 || *s < 0 || e > avail);
}

// the session's error word keeps the first failing record
__device__ __forceinline__ void rec_fail(unsigned long long *err, int64_t rec, int32_t kind) {
  atomicMin(err, ((unsigned long long)rec << 4) | (unsigned long long)kind);
}

// add(cell, lanes holding it) once per distinct cell among the wave's lanes (cell < 0: none), on the first such lane.
// Called by every lane of the wave.
template <class F>
__device__ __forceinline__ void wave_distinct(int32_t cell, int lane, F add) {
  uint64_t pend = __ballot(cell >= 0);
  while (pend) {
    const int leader = __ffsll((unsigned long long)pend) - 1;
    const int32_t lc = __shfl(cell, leader, 64);
    const uint64_t m = __ballot(cell == lc);
    if (lane == leader) add(lc, (uint32_t)__popcll(m));
    pend &= ~m;
  }
}

}  // namespace mh
