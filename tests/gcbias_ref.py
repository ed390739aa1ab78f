"""NumPy restatement of the GC-bias thinning rule (test infrastructure; mitty_hip.h mh_gc_thin, mh_gcbias.hip).

There is no reference behaviour for GC bias (the reference's sampler only marks the place, illumina.py:67), so the
rule is this project's own specification and this restatement is the yardstick:

  T[b] = min(2^32, floor(w[b] * 2^32)) for the curve's 101 weights (simulation.gcbias.thresholds)
  template t (its index in the unit's set before thinning):
    start = clamp(pos0[t] - p_min, 0, hap_len), end = clamp(pos1[t] + rlen - p_min, start, hap_len), L = end - start
    g   = bytes of hap[start:end] equal to 'G' or 'C' (upper case only)
    bin = (100 * g) // L, 0 when L == 0
    u   = word 0 of philox4x32_10((t & 0xffffffff, t >> 32, 0, c3), (k0, k1)) with keys(seed, unit_key)
    kept iff u < T[bin]
Nothing here touches the GPU."""
import numpy as np

from tests.philox_ref import philox4x32_10

N_BINS = 101


def keys(seed, unit_key):
  return seed & 0xffffffff, unit_key & 0xffffffff, ((seed >> 32) ^ (unit_key >> 32) ^ 0x67636269) & 0xffffffff


def draws(n, seed, unit_key, t0=0):
  """u of templates t0 .. t0 + n - 1, as uint64."""
  k0, k1, c3 = keys(seed, unit_key)
  t = np.arange(t0, t0 + n, dtype=np.uint64)
  return philox4x32_10(t & np.uint64(0xffffffff), t >> np.uint64(32), np.zeros(n, np.uint64),
                       np.full(n, c3, np.uint64), k0, k1)[0]


def bins(hap, p_min, pos0, pos1, rlen):
  """The GC bin of every template: a prefix sum of the 'G' / 'C' bytes of hap, then the clamped span's count."""
  h = np.frombuffer(bytes(hap), np.uint8)
  hap_len = len(h)
  cum = np.concatenate(([0], np.cumsum((h == ord('G')) | (h == ord('C'))))).astype(np.int64)
  pos0, pos1 = np.asarray(pos0, np.int64), np.asarray(pos1, np.int64)
  start = np.clip(pos0 - p_min, 0, hap_len)
  end = np.minimum(np.maximum(pos1 + rlen - p_min, start), hap_len)
  L = end - start
  g = cum[end] - cum[start]
  return np.where(L > 0, (100 * g) // np.maximum(L, 1), 0).astype(np.int64)


def thin(hap, p_min, fo0, pos0, pos1, rlen, T, seed, unit_key, n0=None, t0=0):
  """-> (kept index array, bins, seen[101], kept[101]).  T: uint64[101] thresholds; t0: the index of the first
  template handed in inside the set it is thinned as a part of (0: the whole set).  fo0 and n0 ride along."""
  n = len(pos0)
  assert len(fo0) == n and len(pos1) == n and (n0 is None or len(n0) == n)
  T = np.asarray(T, np.uint64)
  assert T.shape == (N_BINS,) and int(T.max(initial=0)) <= 1 << 32
  b = bins(hap, p_min, pos0, pos1, rlen)
  keep = draws(n, seed, unit_key, t0) < T[b]
  seen = np.bincount(b, minlength=N_BINS).astype(np.int64)
  kept = np.bincount(b[keep], minlength=N_BINS).astype(np.int64)
  return np.flatnonzero(keep), b, seen, kept
