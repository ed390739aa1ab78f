// mh_inflate.hip — BGZF inflate on the device: one launch inflates and CRC-checks a batch of members (mh_inflate.h
// holds the decoder; mh_deflate.hip is the other direction).
//
//   k_inflate: one wave64 workgroup per member, a grid-stride loop over the batch's descriptors.  The member's output
//   window (ISIZE <= 64 KiB, so no back-reference ever leaves it), the Huffman tables, the CRC table and 8 KiB of the
//   payload at a time (the bit reader's refill is a dependent load per symbol: from LDS, not from HBM) live in LDS:
//   77 KiB a workgroup, two workgroups per CU.  The serial symbol decode runs on every lane with the same values
//   (readfirstlane keeps the bit buffer and the walk in scalar registers):
//   in effect one lane decodes.  All 64 lanes fill the first-level tables, carry out the match copies and stored
//   blocks, compute the CRC-32 (a slice per lane, joined by x^(8 len) mod P) and store the finished window to HBM, in
//   16-byte stores: the window sits in LDS at the destination's offset from a 16-byte boundary.
//   A match reads only bytes written before it began (position - distance + i mod distance for distance < length),
//   which is the byte-serial result without any order among its own bytes.
//   Per member the kernel writes a status word (inf::ST_*); nothing goes through a context's fault slot.
//
//   mh::Inflater: the host side, used by mh_bamread.cpp through mh_inflate.h.  No mh_ctx: its own stream, two
//   page-locked staging buffers and device buffers, hipSetDevice in the calling thread.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mitty_hip.h"
#include "mh_inflate.h"

namespace mh {

namespace {

using namespace inf;

constexpr int INF_LANES = 64;
constexpr int IN_BYTES = 8192, IN_WORDS = IN_BYTES / 8;   // the payload bytes staged in LDS at a time

struct DevMember {
  uint64_t src, dst;   // offsets into the launch's compressed and output buffers
  uint32_t clen, isize, crc, pad;
};

struct InfLds {
  alignas(16) uint8_t win[MAX_ISIZE + 16];
  Tables T;
  uint32_t crc_tab[256];
  uint64_t in[IN_WORDS];
};
static_assert(2 * sizeof(InfLds) <= 160 * 1024, "two workgroups per CU");

__constant__ CrcPowers kInfCrcPow = make_crc_powers();

// The policies the decoder's templates take on the device.  They are instantiated from k_inflate only; the members are
// __host__ __device__ (with the device's builtins compiled for the device alone) because the templates are.
struct DevPolicy {
  int ln;
  __host__ __device__ int lane() const { return ln; }
  __host__ __device__ int lanes() const { return INF_LANES; }
  __host__ __device__ uint32_t uni(uint32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
  }
  __host__ __device__ void sync() const {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
  }
};

// The payload through LDS: in[base, base + IN_BYTES) staged by all lanes (zeros past the payload's end), restaged
// from the reader's position when a load comes within 16 bytes of its end.  `in` is 8-byte aligned.
struct DevSource {
  const uint8_t *in;
  int64_t n, base;
  uint64_t *buf;
  int ln;
  __host__ __device__ void stage(int64_t pos) {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
    base = pos & ~(int64_t)7;
    for (int w = ln; w < IN_WORDS; w += INF_LANES) {
      const int64_t o = base + 8 * (int64_t)w;
      uint64_t v = 0;
      if (o + 8 <= n) {
        v = *(const uint64_t *)(in + o);
      } else {
        for (int b = 0; b < 8; b++)
          if (o + b < n) v |= (uint64_t)in[o + b] << (8 * b);
      }
      buf[w] = v;
    }
    __syncthreads();
#endif
  }
  __host__ __device__ uint64_t load64(int64_t pos) {
    if (pos < base || pos + 16 > base + IN_BYTES) stage(pos);
    const int r = (int)(pos - base), w = r >> 3, s = (r & 7) * 8;   // w + 1 < IN_WORDS
    const uint64_t a = buf[w], b = buf[w + 1];
    const uint64_t v = s ? (a >> s) | (b << (64 - s)) : a;
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32 |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
#else
    return v;
#endif
  }
  __host__ __device__ uint32_t byte(int64_t pos) { return (uint32_t)load64(pos) & 0xffu; }
};

// The member's window in LDS.  The core has checked pos + len <= ISIZE and dist <= pos before each call.
struct DevOut {
  uint8_t *win;
  int ln;
  __host__ __device__ void lit(uint32_t pos, uint8_t b) { win[pos] = b; }   // every lane, the same byte
  __host__ __device__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();   // the literals and copies before this one are in the window
#endif
    const uint8_t *src = win + pos - dist;
    if (dist >= len) {
      for (uint32_t i = (uint32_t)ln; i < len; i += INF_LANES) win[pos + i] = src[i];
    } else {
      for (uint32_t i = (uint32_t)ln; i < len; i += INF_LANES) win[pos + i] = src[i % dist];
    }
  }
  __host__ __device__ void store(uint32_t pos, const uint8_t *s, uint32_t len) {
    for (uint32_t i = (uint32_t)ln; i < len; i += INF_LANES) win[pos + i] = s[i];
  }
};

__device__ inline uint64_t uni64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}

__global__ void __launch_bounds__(INF_LANES) k_inflate(const uint8_t *__restrict__ comp, int64_t comp_bytes,
                                                       const DevMember *__restrict__ mem, int n_mem,
                                                       uint8_t *__restrict__ out, int64_t out_bytes,
                                                       uint32_t *__restrict__ status) {
  __shared__ InfLds L;
  const int lane = (int)threadIdx.x;
  DevPolicy pol{lane};
  for (int i = lane; i < 256; i += INF_LANES) L.crc_tab[i] = crc_table_entry((uint32_t)i);
  __syncthreads();
  for (int k = (int)blockIdx.x; k < n_mem; k += (int)gridDim.x) {
    const uint64_t src = uni64(mem[k].src), dst = uni64(mem[k].dst);
    const uint32_t clen = pol.uni(mem[k].clen), isize = pol.uni(mem[k].isize), want = pol.uni(mem[k].crc);
    int32_t st = ST_BAD_STREAM;
    // (the host builds the descriptors from checked headers; a descriptor outside the buffers is refused all the same)
    const bool inside = isize <= (uint32_t)MAX_ISIZE && (src & 7) == 0 && src <= (uint64_t)comp_bytes &&
                        clen <= (uint64_t)comp_bytes - src && dst <= (uint64_t)out_bytes &&
                        isize <= (uint64_t)out_bytes - dst;
    if (inside) {
      const uint32_t shift = (uint32_t)dst & 15u;
      DevOut o{L.win + shift, lane};
      uint32_t produced = 0;
      DevSource in{comp + src, (int64_t)clen, -4 * (int64_t)IN_BYTES, L.in, lane};
      st = inflate_raw(in, comp + src, (int64_t)clen, isize, o, L.T, pol, &produced);
      __syncthreads();
      if (st == ST_OK) {
        uint32_t acc, tail;
        crc_slices(o.win, (int)isize, kInfCrcPow, L.crc_tab, lane, INF_LANES, &acc, &tail);
        for (int d = INF_LANES / 2; d > 0; d >>= 1) {
          acc ^= (uint32_t)__shfl_xor((int)acc, d, INF_LANES);
          tail ^= (uint32_t)__shfl_xor((int)tail, d, INF_LANES);
        }
        if (pol.uni(crc_finish(acc, tail, (int)isize, kInfCrcPow)) != want) st = ST_CRC;
      }
      if (st == ST_OK) {   // window -> HBM: bytes up to the first 16-byte boundary, 16-byte stores, the rest
        uint8_t *g = out + dst;
        const uint8_t *w = o.win;
        const uint32_t head = std::min<uint32_t>(isize, (16u - shift) & 15u), nb = (isize - head) >> 4;
        for (uint32_t i = (uint32_t)lane; i < head; i += INF_LANES) g[i] = w[i];
        const uint4 *ws = (const uint4 *)(w + head);
        uint4 *gs = (uint4 *)(g + head);
        for (uint32_t i = (uint32_t)lane; i < nb; i += INF_LANES) gs[i] = ws[i];
        for (uint32_t i = head + 16u * nb + (uint32_t)lane; i < isize; i += INF_LANES) g[i] = w[i];
      }
    }
    if (lane == 0) status[k] = (uint32_t)st;
    __syncthreads();   // the window is read out before the next member writes it
  }
}

}  // namespace

class Inflater {
 public:
  int device = 0, cus = 1;
  hipStream_t stream = nullptr;
  uint8_t *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
  size_t h_in_cap = 0, h_out_cap = 0, d_in_cap = 0, d_out_cap = 0;
};

namespace {

int32_t hip_err(std::string *err, hipError_t e, const char *what) {
  if (err) *err = std::string("device inflate: ") + what + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? MH_E_OOM : MH_E_HIP;
}

#define INF_CHK(call, what)                         \
  do {                                              \
    const hipError_t _e = (call);                   \
    if (_e != hipSuccess) return hip_err(err, _e, what); \
  } while (0)

size_t grown(size_t need) { return (need + need / 4 + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1); }

int32_t reserve_host(uint8_t **p, size_t *cap, size_t need, std::string *err) {
  if (need <= *cap) return MH_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t c = grown(need);
  INF_CHK(hipHostMalloc((void **)p, c, hipHostMallocDefault), "hipHostMalloc");
  *cap = c;
  return MH_OK;
}

int32_t reserve_dev(uint8_t **p, size_t *cap, size_t need, std::string *err) {
  if (need <= *cap) return MH_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t c = grown(need);
  INF_CHK(hipMalloc((void **)p, c), "hipMalloc");
  *cap = c;
  return MH_OK;
}

// f(k) for k in [0, n) on up to `threads` threads, in contiguous shares
template <class F>
void shared_among(size_t n, int threads, F f) {
  const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), n / 16));
  auto work = [&](size_t t) {
    for (size_t k = n * t / nt; k < n * (t + 1) / nt; k++) f(k);
  };
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nt; t++) pool.emplace_back(work, t);
  work(0);
  for (auto &t : pool) t.join();
}

}  // namespace

int32_t inflater_create(int device, Inflater **out, std::string *err) {
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
    if (err) *err = "device inflate: no HIP device";
    return MH_E_NO_DEVICE;
  }
  if (device < 0 || device >= n) {
    if (err) *err = "device inflate: no device " + std::to_string(device);
    return MH_E_ARG;
  }
  INF_CHK(hipSetDevice(device), "hipSetDevice");
  Inflater *f = new Inflater();
  f->device = device;
  hipError_t e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);
  int cus = 0;
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  if (e != hipSuccess) {
    inflater_destroy(f);
    return hip_err(err, e, "stream");
  }
  f->cus = std::max(1, cus);
  *out = f;
  return MH_OK;
}

void inflater_destroy(Inflater *f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->stream) {
    (void)hipStreamSynchronize(f->stream);
    (void)hipStreamDestroy(f->stream);
  }
  if (f->h_in) (void)hipHostFree(f->h_in);
  if (f->h_out) (void)hipHostFree(f->h_out);
  if (f->d_in) (void)hipFree(f->d_in);
  if (f->d_out) (void)hipFree(f->d_out);
  delete f;
}

int32_t inflater_run(Inflater *f, const uint8_t *base, InflateMember *m, size_t n, uint8_t *out, int64_t out_bytes,
                     int threads, std::string *err) {
  if (!f || !m || out_bytes < 0 || n > (size_t)INT32_MAX) return MH_E_ARG;
  if (n == 0) return MH_OK;
  INF_CHK(hipSetDevice(f->device), "hipSetDevice");
  // in: the descriptors, then the payloads, each at a multiple of 8 bytes; out: the inflated bytes, then a status word per member
  const size_t desc = (n * sizeof(DevMember) + 15) & ~(size_t)15;
  size_t comp = 0;
  for (size_t k = 0; k < n; k++) {
    if (m[k].isize > (uint32_t)MAX_ISIZE || m[k].dst < 0 || m[k].dst > out_bytes ||
        (int64_t)m[k].isize > out_bytes - m[k].dst)
      return MH_E_ARG;
    comp += ((size_t)m[k].clen + 7) & ~(size_t)7;
  }
  const size_t st_off = ((size_t)out_bytes + 15) & ~(size_t)15, out_all = st_off + 4 * n;
  int32_t rc = reserve_host(&f->h_in, &f->h_in_cap, desc + comp, err);
  if (rc == MH_OK) rc = reserve_host(&f->h_out, &f->h_out_cap, out_all, err);
  if (rc == MH_OK) rc = reserve_dev(&f->d_in, &f->d_in_cap, desc + comp, err);
  if (rc == MH_OK) rc = reserve_dev(&f->d_out, &f->d_out_cap, out_all, err);
  if (rc != MH_OK) return rc;
  DevMember *dm = (DevMember *)f->h_in;
  size_t at = 0;
  for (size_t k = 0; k < n; k++) {
    dm[k] = DevMember{(uint64_t)at, (uint64_t)m[k].dst, m[k].clen, m[k].isize, m[k].crc, 0};
    at += ((size_t)m[k].clen + 7) & ~(size_t)7;
  }
  shared_among(n, threads, [&](size_t k) {
    if (m[k].clen) memcpy(f->h_in + desc + dm[k].src, base + m[k].src, m[k].clen);
  });
  INF_CHK(hipMemcpyAsync(f->d_in, f->h_in, desc + comp, hipMemcpyHostToDevice, f->stream), "copy to the device");
  const int grid = (int)std::min<size_t>(n, (size_t)f->cus * 4);
  hipLaunchKernelGGL(k_inflate, dim3(grid), dim3(INF_LANES), 0, f->stream, f->d_in + desc, (int64_t)comp,
                     (const DevMember *)f->d_in, (int)n, f->d_out, out_bytes, (uint32_t *)(f->d_out + st_off));
  INF_CHK(hipGetLastError(), "launch");
  INF_CHK(hipMemcpyAsync(f->h_out, f->d_out, out_all, hipMemcpyDeviceToHost, f->stream), "copy from the device");
  INF_CHK(hipStreamSynchronize(f->stream), "inflate kernel");
  const uint32_t *st = (const uint32_t *)(f->h_out + st_off);
  shared_among(n, threads, [&](size_t k) {
    m[k].status = st[k];
    if (st[k] == (uint32_t)ST_OK && m[k].isize) memcpy(out + m[k].dst, f->h_out + m[k].dst, m[k].isize);
  });
  return MH_OK;
}

}  // namespace mh
