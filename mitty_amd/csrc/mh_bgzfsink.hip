// mh_bgzfsink.hip — BgzfSink (mh_internal.h): BGZF blocks deflated in HBM on their way into a file, for the device BAM
// writers (mh_bamwrite.hip) and filter-bam (mh_filter.hip).  The bookkeeping between the owner and the thread is the
// piece queue's (mh_piecequeue.h); what is here is the file, the two page-locked slots and the copies.
#include <chrono>

#include "mh_bgzf.h"
#include "mh_internal.h"

namespace mh {

namespace {
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
}  // namespace

bool BgzfSink::open(mh_ctx *ctx, const char *out_path, const std::string *header, int level, int64_t *data_pos) {
  abort();
  path = out_path;
  device = ctx->device;
  copy_stream = ctx->stream2;
  herr = (int)hipSuccess;
  ioerr = open_failed = close_failed = false;
  d2h_ms = write_ms = 0;
  n_piece = 0;
  q.reset();
  fp = fopen(out_path, "wb");
  if (!fp) {
    ioerr = open_failed = true;
    return false;
  }
  std::string hz;
  if ((header && !bgzf_header_blocks(*header, level, hz)) || fwrite(hz.data(), 1, hz.size(), fp) != hz.size() ||
      fflush(fp) != 0) {   // (flushed: a path on which every write fails is reported here)
    ioerr = true;
    abort();
    return false;
  }
  *data_pos = pos = (int64_t)hz.size();
  th = std::thread([this] { run(); });
  return true;
}

void BgzfSink::push(const void *d, int64_t bytes, hipStream_t st) {
  if (n_piece == ev_piece.size()) {
    hipEvent_t ev = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) {
      herr = (int)e;
      return;
    }
    ev_piece.push_back(ev);
  }
  hipEvent_t ev = ev_piece[n_piece];
  const hipError_t e = hipEventRecord(ev, st);
  if (e != hipSuccess) {
    herr = (int)e;
    return;
  }
  n_piece++;
  q.push((int64_t)(uintptr_t)d, bytes, ev);
}

bool BgzfSink::wait_copied(int64_t mark) { return q.wait_copied(mark) && !failed(); }

// the next sub-piece's copy into slot s queued on the copy stream, behind its piece's event (wait false: only if a
// sub-piece is ready now)
bool BgzfSink::issue(int s, PieceQueue::Sub *sub, bool wait) {
  if (!q.take(sub, wait)) return false;
  hipError_t e = hipSuccess;
  if (!pin[s]) e = hipHostMalloc((void **)&pin[s], (size_t)SLOT_BYTES, hipHostMallocDefault);
  if (e == hipSuccess && !ev_copy[s]) e = hipEventCreateWithFlags(&ev_copy[s], hipEventDisableTiming);
  if (e == hipSuccess) e = hipStreamWaitEvent(copy_stream, (hipEvent_t)sub->token, 0);
  if (e == hipSuccess)
    e = hipMemcpyAsync(pin[s], (const void *)(uintptr_t)sub->off, (size_t)sub->len, hipMemcpyDeviceToHost, copy_stream);
  if (e == hipSuccess) e = hipEventRecord(ev_copy[s], copy_stream);
  if (e != hipSuccess) {
    herr = (int)e;
    return false;
  }
  in_flight[s] = true;
  return true;
}

void BgzfSink::run() {
  (void)hipSetDevice(device);
  PieceQueue::Sub sub[2];
  bool have = issue(0, &sub[0], true);
  for (int s = 0; have && !failed(); s ^= 1) {
    Clock::time_point t0 = Clock::now();
    const hipError_t e = hipEventSynchronize(ev_copy[s]);   // (its own copy only: the stream may carry other work)
    in_flight[s] = false;
    d2h_ms += ms_since(t0);
    if (e != hipSuccess) {
      herr = (int)e;
      break;
    }
    if (sub[s].ends >= 0) q.copied(sub[s].ends);   // that piece's device bytes may be overwritten
    // the following sub-piece, when one is ready, into the other slot while this one is written
    const bool next = issue(s ^ 1, &sub[s ^ 1], false);
    t0 = Clock::now();
    const bool ok = fwrite(pin[s], 1, (size_t)sub[s].len, fp) == (size_t)sub[s].len;
    write_ms += ms_since(t0);
    if (!ok) {
      ioerr = true;
      break;
    }
    pos += sub[s].len;
    have = next || (!failed() && issue(s ^ 1, &sub[s ^ 1], true));
  }
  for (int s = 0; s < 2; s++) {   // what is in flight is drained before the slots go
    if (in_flight[s]) (void)hipEventSynchronize(ev_copy[s]);
    in_flight[s] = false;
  }
  q.stop();
}

bool BgzfSink::finish(bool eof, int64_t *end_pos) {
  if (!fp) {   // (not open: a caller's mistake, reported as a failed write)
    ioerr = true;
    return false;
  }
  q.close();
  if (th.joinable()) th.join();
  FILE *f = fp;
  fp = nullptr;
  if (end_pos) *end_pos = pos;
  char marker[28];
  (void)mh_bgzf_eof(marker);
  if (!failed() && eof && fwrite(marker, 1, 28, f) != 28) ioerr = true;
  if (fclose(f) != 0) ioerr = close_failed = true;
  return !failed();
}

void BgzfSink::abort() {
  if (th.joinable()) {
    q.stop();
    th.join();
  }
  if (fp) (void)fclose(fp);
  fp = nullptr;
}

std::string BgzfSink::io_error() const {
  if (!ioerr.load()) return std::string();
  return (open_failed ? "cannot open " : "BGZF write failed: ") + path;
}

void BgzfSink::release() {
  abort();
  for (int s = 0; s < 2; s++) {
    if (pin[s]) (void)hipHostFree(pin[s]);
    if (ev_copy[s]) (void)hipEventDestroy(ev_copy[s]);
    pin[s] = nullptr;
    ev_copy[s] = nullptr;
  }
  for (hipEvent_t ev : ev_piece) (void)hipEventDestroy(ev);
  ev_piece.clear();
}

}  // namespace mh
