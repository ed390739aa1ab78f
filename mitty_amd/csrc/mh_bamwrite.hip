// mh_bamwrite.hip — the god-aligner store written as a BAM from the device: the sorted record stream deflated in HBM
// (bgzf_device, mh_deflate.hip), its blocks handed to the context's BgzfSink (mh_bgzfsink.hip) as they are packed, and
// the BAI from the device plan (mh_bam.hip).  Behind mh_bam_write_gpu and mh_bam_write_part (mh_api.hip).
#include <algorithm>
#include <condition_variable>
#include <cstring>

#include "mh_bgzf.h"
#include "mh_internal.h"

namespace mh {

namespace {

// Window of a spilled store's deflate: a quarter of the store's capacity (two staging windows in HBM and two ring
// slots of compressed output, each about a window: together about the capacity), whole BGZF blocks, at most 8192
// blocks (535 MB)
int64_t spill_window(const BamStore &B) {
  const int64_t cap_blocks = B.cap > 0 ? B.cap / 4 / BGZF_BLOCK : 8192;
  return std::max<int64_t>(1, std::min<int64_t>(8192, cap_blocks)) * BGZF_BLOCK;
}

// A spilled store's sorted record stream deflated on the device window by window: the host assembles window i + 1
// (bam_assemble, a thread of its own) while window i goes H2D and through bgzf_device into ring slot i & 1 of
// ctx->gz_out (ring bytes per slot), whose pieces go to the sink; the block offsets in `boff` are the stream's.
// Window i may overwrite its slot once window i - 2's pieces have left the device: a mark of the sink per window, waited
// for two windows later.  Windows are whole numbers of BGZF blocks, so the blocks — and the file — are the ones one
// deflate of the whole stream makes.  The stream deflated is the sorted stream from byte `skip`, then `tail` (a range's
// part of a file, mh_bam_write_part).
int32_t bam_deflate_spilled(mh_ctx *ctx, BgzfSink &sink, int64_t ring, int64_t skip, const uint8_t *tail,
                            int64_t tail_len, int64_t *nz, std::vector<int64_t> *boff) {
  BamStore &B = ctx->bam;
  MH_TRY(bam_spill(ctx));   // (the records still in HBM: every record is then on the host)
  MH_TRY(bam_sort(ctx));    // (a no-op unless the spill undid a direct write's order)
  BamHostOrder o;
  MH_TRY(bam_host_order(ctx, o));
  const int64_t W = spill_window(B);
  const int64_t nb = B.bytes - skip, L = nb + tail_len;   // the stream: sorted [skip, bytes), then the tail
  const int64_t n_win = (L + W - 1) / W;
  uint8_t *pin[2] = {nullptr, nullptr};
  struct PinGuard {
    uint8_t **p;
    ~PinGuard() {
      for (int s = 0; s < 2; s++)
        if (p[s]) (void)hipHostFree(p[s]);
    }
  } pguard{pin};
  for (int s = 0; s < 2; s++) HIPCHK(ctx, hipHostMalloc((void **)&pin[s], (size_t)W, hipHostMallocDefault));
  MH_TRY(ensure(ctx, B.in1, (size_t)W + 64));
  MH_TRY(ensure(ctx, B.in2, (size_t)W + 64));
  uint8_t *dwin[2] = {(uint8_t *)B.in1.p, (uint8_t *)B.in2.p};
  std::mutex mu;
  std::condition_variable cv;
  int64_t ready = 0;            // windows assembled
  int64_t freed = 2;            // windows whose staging slot may be refilled (slot of window i: i & 1)
  bool stop = false;
  std::thread asm_th([&]() {
    for (int64_t i = 0; i < n_win; i++) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || i < freed; });
        if (stop) return;
      }
      const int64_t v0 = i * W, v1 = std::min(L, v0 + W);
      if (std::min(v1, nb) > v0) bam_assemble(B, o, skip + v0, skip + std::min(v1, nb), pin[i & 1], 16);
      if (v1 > nb) {
        const int64_t t0 = std::max(v0, nb);
        std::memcpy(pin[i & 1] + (t0 - v0), tail + (t0 - nb), (size_t)(v1 - t0));
      }
      std::lock_guard<std::mutex> lk(mu);
      ready = i + 1;
      cv.notify_all();
    }
  });
  struct Join {
    std::thread *t;
    std::mutex *m;
    std::condition_variable *c;
    bool *stop;
    ~Join() {
      {
        std::lock_guard<std::mutex> lk(*m);
        *stop = true;
        c->notify_all();
      }
      t->join();
    }
  } join{&asm_th, &mu, &cv, &stop};
  boff->assign(1, 0);
  int64_t zpos = 0;
  std::vector<int64_t> bw;
  std::vector<int64_t> marks;   // marks[i]: the sink's pieces once window i's are all pushed
  for (int64_t i = 0; i < n_win; i++) {
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return ready > i; });
    }
    const int s = (int)(i & 1);
    const int64_t len = std::min(L, (i + 1) * W) - i * W;
    HIPCHK(ctx, hipMemcpyAsync(dwin[s], pin[s], (size_t)len, hipMemcpyHostToDevice, ctx->stream));
    if (i >= 2 && !sink.wait_copied(marks[(size_t)i - 2]))   // ring slot s: window i - 2's compressed pieces copied out
      return arg_fail(ctx, MH_E_STATE, "BAM writer stopped before the deflate ring drained");
    uint8_t *const zs = (uint8_t *)ctx->gz_out.p + s * ring;
    const std::function<void(int64_t, int64_t)> piece = [&](int64_t off, int64_t bytes) {
      sink.push(zs + off, bytes, ctx->stream);
    };
    int64_t used = 0;
    MH_TRY(bgzf_device(ctx, ctx->stream, dwin[s], len, zs, ring, &used, &bw, &piece));   // (returns with the stream drained)
    marks.push_back(sink.mark());
    {
      std::lock_guard<std::mutex> lk(mu);
      freed = i + 3;   // slot s (its H2D is done) takes window i + 2
      cv.notify_all();
    }
    boff->pop_back();
    for (int64_t x : bw) boff->push_back(zpos + x);
    zpos += used;
  }
  *nz = zpos;
  return MH_OK;
}

// The sorted store's record stream deflated on the device and written to `path`: the header's block(s) first (hdr
// null: none), the stream from byte `skip` followed by `tail` (tail_len bytes, host memory) cut into 0xff00-byte BGZF
// blocks, the EOF marker when `eof`.  The context's sink copies each packed piece out and writes it while the next
// piece deflates.  boff: the data blocks' offsets from data_pos (nblocks + 1).
struct BamPart {
  int64_t data_pos = 0, end_pos = 0, nz = 0;
  std::vector<int64_t> boff;
};
int32_t bam_write_stream(mh_ctx *ctx, const char *path, const std::string *hdr, int64_t skip, const uint8_t *tail,
                         int64_t tail_len, bool eof, BamPart &P) {
  BamStore &B = ctx->bam;
  BgzfSink &sink = ctx->bam_sink;
  MH_TRY(bam_sort(ctx));
  if (skip < 0 || skip > B.bytes || tail_len < 0 || (tail_len > 0 && !tail))
    return arg_fail(ctx, MH_E_ARG, "BAM part: skip or tail out of range");
  // gz_out is sized for the whole BAM (GBs): released on every exit into the device block cache (the next job's
  // buffers, or the next file's gz_out, take it from there), once the sink's thread no longer reads it
  struct Guard {
    mh_ctx *c;
    ~Guard() {
      c->bam_sink.abort();
      release(c->gz_out);
    }
  } guard{ctx};
  MH_TRY(gz_drain(ctx));
  const int64_t L = B.bytes - skip + tail_len;
  // a spilled (bounded) store deflates window by window into two ring slots; otherwise one buffer for the whole file
  const int64_t ring = B.spilled > 0 ? bgzf_device_bound(spill_window(B)) : 0;
  MH_TRY(ensure(ctx, ctx->gz_out, (size_t)(ring ? 2 * ring : bgzf_device_bound(L))));
  if (!sink.open(ctx, path, hdr, 6, &P.data_pos)) return arg_fail(ctx, MH_E_ARG, sink.io_error());
  int32_t rc = MH_OK;
  if (B.spilled > 0) {
    rc = bam_deflate_spilled(ctx, sink, ring, skip, tail, tail_len, &P.nz, &P.boff);
  } else {
    // the tail after the sorted records (srecs keeps its bytes), then one deflate of [skip, bytes + tail_len)
    if (tail_len > 0) {
      MH_TRY(ensure_keep(ctx, B.srecs, (size_t)(B.bytes + tail_len + 64), (size_t)B.bytes));
      HIPCHK(ctx, hipMemcpyAsync((uint8_t *)B.srecs.p + B.bytes, tail, (size_t)tail_len, hipMemcpyHostToDevice,
                                 ctx->stream));
    }
    uint8_t *const z = (uint8_t *)ctx->gz_out.p;
    const std::function<void(int64_t, int64_t)> piece = [&](int64_t off, int64_t bytes) {
      sink.push(z + off, bytes, ctx->stream);
    };
    rc = bgzf_device(ctx, ctx->stream, (const uint8_t *)B.srecs.p + skip, L, z, (int64_t)ctx->gz_out.cap, &P.nz, &P.boff,
                     &piece);
  }
  if (rc != MH_OK) return rc;
  if (!sink.finish(eof, &P.end_pos)) {
    if (sink.hip_error() != hipSuccess) return hip_fail(ctx, sink.hip_error(), "BAM D2H", __FILE__, __LINE__);
    return arg_fail(ctx, MH_E_ARG, sink.io_error());
  }
  if (P.end_pos - P.data_pos != P.nz) return arg_fail(ctx, MH_E_STATE, "BAM: compressed bytes written differ (internal)");
  return MH_OK;
}

}  // namespace

int32_t bam_write_gpu(mh_ctx *ctx, const char *bam_path, const char *header_text, int64_t header_len,
                      const char *bai_path, int64_t *out_records, int64_t *out_bytes, int64_t *out_file_bytes) {
  BamStore &B = ctx->bam;
  MH_TRY(bam_sort(ctx));
  const int64_t n = B.n_rec;
  // the BAI's per-record half on the device (chunks and linear windows; only their offsets cross PCIe)
  BaiPlan plan;
  std::vector<int64_t> offs;
  bool dev_plan = false;
  if (bai_path) MH_TRY(bam_bai_plan(ctx, plan, offs, &dev_plan));
  const std::string hdr = bam_header_bytes(std::string(header_text ? header_text : "", (size_t)header_len),
                                           B.ref_names, B.ref_len);
  BamPart P;
  MH_TRY(bam_write_stream(ctx, bam_path, &hdr, 0, nullptr, 0, true, P));
  std::vector<int64_t> coff(P.boff.size());
  for (size_t b = 0; b < P.boff.size(); b++) coff[b] = P.data_pos + P.boff[b];
  std::string err;
  if (bai_path) {
    if (dev_plan) {
      if (!bai_emit(bai_path, plan, offs.data(), coff, err)) return arg_fail(ctx, MH_E_ARG, err);
    } else {   // outside the device plan's checks: the host plan (and its errors)
      std::vector<int64_t> soff((size_t)n + 1, 0);
      std::vector<BaiRec> info((size_t)n + 1);
      MH_TRY(bam_fetch_sorted(ctx, nullptr, soff.data(), (int32_t *)info.data()));
      if (!bai_write(bai_path, (int32_t)B.ref_names.size(), n, info.data(), soff.data(), coff, err))
        return arg_fail(ctx, MH_E_ARG, err);
    }
  }
  if (out_records) *out_records = n;
  if (out_bytes) *out_bytes = B.bytes;
  if (out_file_bytes) *out_file_bytes = P.end_pos + 28;
  return MH_OK;
}

int32_t bam_write_part(mh_ctx *ctx, const char *path, const char *header_text, int64_t header_len, int64_t skip,
                       const uint8_t *tail, int64_t tail_len, int32_t eof, int64_t *out_blocks, int64_t *out_data_pos,
                       int64_t *out_bytes, int64_t *boff, int64_t boff_cap) {
  BamStore &B = ctx->bam;
  std::string hdr;
  if (header_len >= 0)
    hdr = bam_header_bytes(std::string(header_text ? header_text : "", (size_t)header_len), B.ref_names, B.ref_len);
  BamPart P;
  MH_TRY(bam_write_stream(ctx, path, header_len >= 0 ? &hdr : nullptr, skip, tail, tail_len, eof != 0, P));
  const int64_t nb = (int64_t)P.boff.size() - 1;
  *out_blocks = nb;
  *out_data_pos = P.data_pos;
  *out_bytes = P.end_pos + (eof ? 28 : 0);
  if (boff) {
    if (boff_cap < nb + 1) return arg_fail(ctx, MH_E_CAPACITY, "block offset array too small");
    std::memcpy(boff, P.boff.data(), 8 * (size_t)(nb + 1));
  }
  return MH_OK;
}

}  // namespace mh
