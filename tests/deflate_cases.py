"""Shared pieces of the deflate tests (tests/test_deflate_cpu.py, tests/test_gpu_deflate.py, tests/test_gpu_parity.py):
the BGZF member walk, the host restatement of the device parse (tests/deflate_host.cpp, built with hipcc) as a
reference, and the generators of the inputs whose shape (codes used, Huffman folds, token widths) the reference's
report proves.  Every generator is seeded: the same bytes on every run."""
import json
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 0xff00                   # input bytes per BGZF block
SLICE = BLOCK // 8               # input bytes per wave: one deflate block each
MIN_MATCH, MAX_MATCH = 7, 258


def bgzf_members(z):
  """The BGZF members of z: (BSIZE, ISIZE) each, checking the gzip header and the BC extra field."""
  out, o = [], 0
  while o < len(z):
    assert z[o:o + 4] == b'\x1f\x8b\x08\x04' and z[o + 12:o + 16] == b'BC\x02\x00', o
    bsize = int.from_bytes(z[o + 16:o + 18], 'little') + 1
    isize = int.from_bytes(z[o + bsize - 4:o + bsize], 'little')
    assert isize <= 0xff00
    out.append((bsize, isize))
    o += bsize
  assert o == len(z)
  return out


def bgzf_bound(n):
  """mh_deflate.hip bgzf_device_bound: every block stored."""
  return n + ((n + BLOCK - 1) // BLOCK + 1) * 31 + 64


def build_tool(tmp_path_factory):
  out = str(tmp_path_factory.mktemp('df') / 'deflate_host')
  subprocess.check_call(['/opt/rocm/bin/hipcc', '-O2', '-std=c++17', '-x', 'hip', '--offload-arch=gfx950',
                         '-include', 'algorithm', '-o', out, os.path.join(HERE, 'deflate_host.cpp')])
  return out


class Reference:
  """deflate_host --device-rules on byte strings: (members, report), remembered per input."""

  def __init__(self, tool, tmp):
    self.tool, self.tmp, self.memo = tool, str(tmp), {}

  def __call__(self, data):
    data = bytes(data)
    key = (len(data), hash(data))
    if key not in self.memo:
      src, dst = os.path.join(self.tmp, 'in'), os.path.join(self.tmp, 'out')
      with open(src, 'wb') as f:
        f.write(data)
      p = subprocess.run([self.tool, '--device-rules', src, dst], stderr=subprocess.PIPE, check=True)
      with open(dst, 'rb') as f:
        z = f.read()
      self.memo[key] = (z, json.loads(p.stderr.decode().strip().splitlines()[-1]))
    return self.memo[key]


# ---- deflate's code tables (RFC 1951 3.2.5), restated for the expectations ---------------------------------------
def len_base(c):
  return c + 3 if c < 8 else 258 if c == 28 else 3 + ((4 + (c & 3)) << (c // 4 - 1))


def len_extra(c):
  return 0 if c < 8 or c == 28 else c // 4 - 1


def dist_base(c):
  return c + 1 if c < 4 else 1 + ((2 + (c & 1)) << (c // 2 - 1))


def dist_extra(c):
  return 0 if c < 4 else c // 2 - 1


# the farthest match inside a slice: MIN_MATCH bytes at its end copied from its start
MAX_SLICE_DIST = SLICE - MIN_MATCH
# per code with extra bits: (lowest, highest) extra value a slice can hold
LEN_EXTREMES = {c: (0, 30 if c == 27 else (1 << len_extra(c)) - 1) for c in range(8, 28)}
DIST_EXTREMES = {c: (0, min((1 << dist_extra(c)) - 1, MAX_SLICE_DIST - dist_base(c))) for c in range(4, 26)}


# ---- inputs ---------------------------------------------------------------------------------------------------------
_WORDS = [b'read', b'model', b'haplotype', b'variant', b'GATTACA', b'ACGTACGTTGCA', b'quality', b'the', b'of',
          b'and', b'sample', b'offset', b'@S1:0:0', b'+', b'FFFFFFFFFFFF', b'insertion', b'deletion', b'chromosome',
          b'a', b'is']


def text(n, seed=1):
  """n bytes of compressible text: seeded draws from a small vocabulary."""
  rng = np.random.default_rng(seed)
  out, size = [], 0
  while size < n:
    w = _WORDS[int(rng.integers(0, len(_WORDS)))] + (b'\n' if rng.integers(0, 12) == 0 else b' ')
    out.append(w)
    size += len(w)
  return b''.join(out)[:n]


_TEXT = text(2 * BLOCK + 1)

SIZES = (list(range(1, 9)) + [131, 132, 133, 263, 264, 265, 255, 256, 257, 8159, 8160, 8161, 8166, 8167] +
         [SLICE * k + d for k in range(2, 8) for d in (-1, 0, 1)] + [7 * SLICE + 6, 7 * SLICE + 7, 65208,
                                                                     65279, 65280, 65281, 65280 + 8163,
                                                                     2 * 65280, 2 * 65280 + 1])


def sized(n):
  return _TEXT[:n]


PERIODS = list(range(1, 10)) + [63, 64, 65] + list(range(255, 261)) + [511, 512, 513, 1000, 4096, 8153, 8159]


def periodic(p):
  """A random base of p bytes repeated over one block plus 777 bytes."""
  base = np.random.default_rng(7000 + p).integers(0, 256, p, dtype=np.uint8).tobytes()
  n = BLOCK + 777
  return (base * (n // p + 1))[:n]


def _rand_without(rng, n, avoid):
  """n random bytes, none equal to `avoid`."""
  x = rng.integers(0, 255, n, dtype=np.uint8)
  return np.where(x >= avoid, x + 1, x).astype(np.uint8)


FILL = 0x5a


def _pad_slice(parts):
  b = b''.join(parts)
  assert len(b) <= SLICE, len(b)
  return b + bytes([FILL]) * (SLICE - len(b))


def lengths_slice(seed, literals=True):
  """One slice whose matches have every length the length codes' extremes need: a random source of 300 bytes, then
  its prefixes of those lengths, longest first (each finds the previous, longer copy and stops at its own end: the
  byte after a copy differs from the source's next byte), then all 256 byte values."""
  rng = np.random.default_rng(seed)
  src = _rand_without(rng, 300, FILL)
  lens = sorted({7, 8, 9, 10, 258} | {len_base(c) + x for c, xs in LEN_EXTREMES.items() for x in xs}, reverse=True)
  parts = [src.tobytes()]
  # the byte before a copy differs from copy to copy (and from the source's first): else the match would start on it
  before = [int(v) for v in rng.permutation(256) if v not in (FILL, int(src[0]), int(src[299]))]
  for i, L in enumerate(lens):
    sep0 = int(_rand_without(rng, 1, FILL)[0])
    while sep0 == src[L]:
      sep0 = int(_rand_without(rng, 1, FILL)[0])
    parts += [bytes([sep0, before[i]]), src[:L].tobytes()]
  if literals:
    parts.append(rng.permutation(256).astype(np.uint8).tobytes())
  return _pad_slice(parts)


FAR_DISTS = sorted({dist_base(c) + x for c in range(18, 26) for x in DIST_EXTREMES[c]})
NEAR_DISTS = [2, 3, 4] + sorted({dist_base(c) + x for c in range(4, 18) for x in DIST_EXTREMES[c]})


def _hashes(s):
  """mh_deflate.hip hash4 of every position's four bytes (2^11 entries)."""
  x = s.astype(np.uint64)
  w = x[:-3] | x[1:-2] << np.uint64(8) | x[2:-1] << np.uint64(16) | x[3:] << np.uint64(24)
  return ((w * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(32 - 11)


def far_slice(seed):
  """One slice with a 7-byte match at each of FAR_DISTS (513 .. 8153): short random sources at the start, a filler of
  one byte (runs at distance 1; its positions hash to one table entry), and each source copied at its distance.  The
  table keeps the latest position per entry, so the sources are redrawn until no position between a source and its
  copy shares the source's entry."""
  rng = np.random.default_rng(seed)
  n = len(FAR_DISTS)
  ds = FAR_DISTS[::-1]                       # the farthest from position 0
  assert ds[0] == MAX_SLICE_DIST
  while True:
    s = np.full(SLICE, FILL, np.uint8)
    s[:16 * n] = _rand_without(rng, 16 * n, FILL)
    pairs = []
    for i, d in enumerate(ds):
      j = 0 if i == 0 else 16 * (n - i)      # ascending distances get ascending sources: copies do not overlap
      q = j + d
      assert q + MIN_MATCH <= SLICE
      s[q:q + MIN_MATCH] = s[j:j + MIN_MATCH]
      pairs.append((q, j))
    pairs.sort()
    assert all(a[0] + MIN_MATCH < b[0] for a, b in zip(pairs, pairs[1:])) and pairs[0][0] >= 16 * n + 256
    h = _hashes(s)
    if all(not np.any(h[j + 1:q] == h[j]) for q, j in pairs):
      return s.tobytes()


def near_slices(seed):
  """Slices of periodic segments, one per distance of NEAR_DISTS (2 .. 512): a random base of d bytes repeated over
  d + 520 bytes, so some step starts inside the segment with its first period already in the table and takes matches
  at distance d."""
  rng = np.random.default_rng(seed)
  slices, parts, size = [], [], 0
  for d in NEAR_DISTS:
    base = _rand_without(rng, d, FILL)
    while d > 1 and len(set(base.tolist())) < 2:
      base = _rand_without(rng, d, FILL)
    seg = np.resize(base, d + 520).tobytes()
    if size + len(seg) > SLICE:
      slices.append(_pad_slice(parts))
      parts, size = [], 0
    parts.append(seg)
    size += len(seg)
  slices.append(_pad_slice(parts))
  return slices


def grid(seed=0):
  """One block whose slices together use every length code 4..28 and distance code 0..25 at both ends of their extra
  bits (the highest that fits a slice)."""
  return lengths_slice(101 + seed) + far_slice(200 + seed) + b''.join(near_slices(300 + seed))


def many_symbols(seed=0):
  return lengths_slice(101 + seed)


def cl_profile(seed):
  """A slice of literals whose code lengths make the code-length code deep: an alphabet of 40..250 bytes with weights
  max(1, g^i mod 2000), g in 1.15..1.9, scaled to at most 7000 bytes, symbols permuted, bytes shuffled."""
  rng = np.random.default_rng(seed)
  k = int(rng.integers(40, 251))
  g = float(rng.uniform(1.15, 1.9))
  w = np.array([max(1, int((g ** i) % 2000)) for i in range(k)], np.int64)
  if w.sum() > 7000:
    w = np.maximum(1, w * 7000 // w.sum())
    while w.sum() > 7000:
      w[int(np.argmax(w))] -= int(w.sum() - 7000)
  syms = rng.permutation(256)[:k].astype(np.uint8)
  data = np.repeat(syms, w)
  rng.shuffle(data)
  return data.tobytes()


def de_bruijn(k, n):
  """The de Bruijn sequence B(k, n) over 0..k-1 (Lyndon words): no n-gram occurs twice, so the parse finds no match
  of n bytes in any stretch of it."""
  a, seq = [0] * (k * n), []

  def db(t, p):
    if t > n:
      if n % p == 0:
        seq.extend(a[1:p + 1])
    else:
      a[t] = a[t - p]
      db(t + 1, p)
      for j in range(a[t - p] + 1, k):
        a[t] = j
        db(t + 1, t)
  db(1, 1)
  return np.array(seq, np.uint8)


_DB4 = de_bruijn(4, MIN_MATCH) + 0x30      # 16384 bytes of '0'..'3' without a repeated 7-gram: 2-bit literals


def wide_slice(seed):
  """A slice of rare, wide matches among thousands of cheap tokens: random sources (4 of 131..257 bytes, then 16
  short), a zero filler (a run: one table entry, so the sources stay in the table), then each source copied once
  (the long ones last, beyond distance 4096: 5 + 11 extra bits) between stretches of a four-symbol sequence without
  repeated 7-grams (2-bit literals, no matches) and short zero runs (many matches at distance 1).  The length and
  distance codes used once each are then deep."""
  rng = np.random.default_rng(seed)
  lens = [int(rng.integers(a, a + 32)) for a in (131, 163, 195, 226)] + [MIN_MATCH + 1] * 16   # a length code each
  parts, srcs, o = [], [], 0
  for L in lens:
    parts.append(rng.integers(0x40, 0x100, L, dtype=np.uint8))
    srcs.append(len(parts) - 1)
    o += L
  parts.append(np.zeros(300, np.uint8))
  o += 300
  t = int(rng.integers(0, 4000))                                # the stretches: successive pieces of _DB4
  zeros = np.zeros(9, np.uint8)
  for k in srcs[4:] + srcs[:4]:
    L = len(parts[k])
    for _ in range(4):
      g = int(rng.integers(20, 40))
      parts += [_DB4[t:t + g], zeros]
      t += g
      o += g + 9
    g = int(rng.integers(20, 52))
    parts += [_DB4[t:t + g], parts[k]]
    t += g
    o += g + L
  assert o <= SLICE, o
  parts.append(_DB4[t:t + SLICE - o])
  out = np.concatenate(parts).tobytes()
  assert len(out) == SLICE
  return out


def wide_tokens(seed=0):
  """One block of eight wide_slice()s."""
  return b''.join(wide_slice(8 * seed + k) for k in range(8))


def _hash4(b0, b1, b2, b3):
  return (((b0 | b1 << 8 | b2 << 16 | b3 << 24) * 2654435761) & 0xffffffff) >> (32 - 11)


def fibonacci_literals(seed=0):
  """A slice of 4179 literals and no match at all, whose 16 byte values occur 1, 2, 3, 5, ... 1597 times: with the
  end of block (once) the Huffman tree is a chain 16 deep, one more than deflate allows, so the 15-bit limiter folds
  it.  The bytes are placed one by one following the parse: a byte that would complete a 7-byte match against the
  position the hash table holds at that step's start (or a run of 8) is not taken."""
  rng = np.random.default_rng(seed)
  fib = [1, 2]
  while len(fib) < 16:
    fib.append(fib[-1] + fib[-2])
  syms = [int(v) for v in rng.permutation(256)[:16]]
  left = dict(zip(syms, fib))
  n = sum(fib)
  s, table = [], {}
  for i in range(n):
    p = i - (MIN_MATCH - 1)                 # the position whose 7 bytes this byte completes
    bad = set()
    if p >= 0:
      if p % 256 == 0:                      # a new step: the positions of the step before are in the table
        for k in range(max(0, p - 256), p):
          table[_hash4(*s[k:k + 4])] = k
      j = table.get(_hash4(*s[p:p + 4]))
      if j is not None and s[j:j + MIN_MATCH - 1] == s[p:p + MIN_MATCH - 1]:
        bad.add(s[j + MIN_MATCH - 1])
      if p >= 1 and len(set(s[p - 1:i])) == 1:
        bad.add(s[p])                       # bytes p-1 .. p+5 are equal: one more is a run candidate
    ok = [v for v in syms if left[v] > 0 and v not in bad]
    if not ok:
      return None
    w = np.array([left[v] for v in ok], np.float64)
    v = ok[int(rng.choice(len(ok), p=w / w.sum()))]
    left[v] -= 1
    s.append(v)
  return bytes(s)
