"""Shared pieces of the inflate tests (tests/test_inflate_cpu.py, tests/test_gpu_inflate.py): BGZF members from zlib at
a chosen level, strategy and block size, a bit writer that emits hand-made DEFLATE streams (fixed Huffman and given
dynamic tables: shapes zlib's compressor never writes), zlib's verdict on a member, the named valid and malformed cases,
and the host run of the decoder core (tests/inflate_host.cpp, built with the sanitizers)."""
import heapq
import os
import struct
import subprocess
import zlib

import numpy as np

from tests import deflate_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
ST_OK, ST_BAD_STREAM, ST_LENGTH, ST_CRC = 0, 1, 2, 3


# ---- BGZF framing ---------------------------------------------------------------------------------------------------
def member(raw, isize, crc):
  """One BGZF member around the raw deflate stream `raw` with the given trailer."""
  bsize = 18 + len(raw) + 8
  assert bsize <= 65536, bsize
  return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', bsize - 1) + raw +
          struct.pack('<II', crc & 0xffffffff, isize & 0xffffffff))


def member_of(raw, data):
  return member(raw, len(data), zlib.crc32(data))


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
  c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
  return c.compress(data) + c.flush()


def bgzf(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, block=D.BLOCK):
  """BGZF members of `data`, `block` input bytes each (an empty input gives one empty member)."""
  out = []
  for o in range(0, max(len(data), 1), block):
    part = data[o:o + block]
    out.append(member_of(raw_deflate(part, level, strategy), part))
  return b''.join(out)


def split(z):
  """The members of a BGZF byte string: (file offset, raw deflate, isize, crc) each."""
  out, o = [], 0
  while o < len(z):
    assert z[o:o + 4] == b'\x1f\x8b\x08\x04'
    xlen = int.from_bytes(z[o + 10:o + 12], 'little')
    assert z[o + 12:o + 16] == b'BC\x02\x00'
    bsize = int.from_bytes(z[o + 16:o + 18], 'little') + 1
    crc, isize = struct.unpack('<II', z[o + bsize - 8:o + bsize])
    out.append((o, z[o + 12 + xlen:o + bsize - 8], isize, crc))
    o += bsize
  assert o == len(z)
  return out


def zlib_verdict(raw, isize, crc):
  """(good, bytes) as the reader's zlib path decides: the stream ends, gives exactly isize bytes, and the CRC-32
  matches.  (max_length isize + 1: one byte over shows as a wrong length, and 0 would mean no limit.)"""
  d = zlib.decompressobj(-15)
  try:
    out = d.decompress(raw, isize + 1)
  except zlib.error:
    return False, b''
  good = d.eof and len(out) == isize and zlib.crc32(out) == crc
  return good, out if good else b''


# ---- a DEFLATE writer -----------------------------------------------------------------------------------------------
class Bits:
  """LSB-first bit sink (RFC 1951 3.1.1); Huffman codes go in most significant bit first."""

  def __init__(self):
    self.acc, self.n, self.out = 0, 0, bytearray()

  def put(self, v, n):
    assert 0 <= v < (1 << n) or n == 0
    self.acc |= v << self.n
    self.n += n
    while self.n >= 8:
      self.out.append(self.acc & 255)
      self.acc >>= 8
      self.n -= 8

  def code(self, c, n):
    self.put(int('{:0{}b}'.format(c, n)[::-1], 2) if n else 0, n)

  def align(self):
    if self.n:
      self.put(0, 8 - self.n)

  def bytes(self):
    self.align()
    return bytes(self.out)


def canonical(lens):
  """{symbol: (code, length)} of the canonical Huffman code with these lengths (3.2.2)."""
  codes, code = {}, 0
  for n in range(1, 16):
    for s, l in enumerate(lens):
      if l == n:
        codes[s] = (code, n)
        code += 1
    code <<= 1
  return codes


def huffman_lengths(freq, n):
  """Code lengths (n entries) of a Huffman code for the used symbols of freq {symbol: count}; one used symbol gets
  length 1.  (The test alphabets are small: no length passes 15.)"""
  lens = [0] * n
  if len(freq) == 1:
    lens[next(iter(freq))] = 1
    return lens
  heap = [(f, s, [s]) for s, f in sorted(freq.items())]
  heapq.heapify(heap)
  while len(heap) > 1:
    a, b = heapq.heappop(heap), heapq.heappop(heap)
    for s in a[2] + b[2]:
      lens[s] += 1
    heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
  assert max(lens) <= 15
  return lens


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def len_symbol(length):
  """(code 0..28, extra bits, extra value) of a match length."""
  if length == 258:
    return 28, 0, 0
  for c in range(27, -1, -1):
    if D.len_base(c) <= length:
      assert length - D.len_base(c) < (1 << D.len_extra(c))
      return c, D.len_extra(c), length - D.len_base(c)
  raise ValueError(length)


def dist_symbol(dist):
  for c in range(29, -1, -1):
    if D.dist_base(c) <= dist:
      assert dist - D.dist_base(c) < (1 << D.dist_extra(c))
      return c, D.dist_extra(c), dist - D.dist_base(c)
  raise ValueError(dist)


def symbols(tokens):
  """Tokens -> [(literal/length symbol, extra bits, extra value, None | (distance code, extra bits, extra value))].
  A token is an int (a literal byte), ('m', length, distance), ('l284', extra, distance): length symbol 284 with a
  given extra value, ('sym', s): a bare literal/length symbol, or ('md', length, distance code, extra value): a match
  with a raw distance code."""
  out = []
  for t in tokens:
    if isinstance(t, int):
      out.append((t, 0, 0, None))
    elif t[0] == 'm':
      c, xb, xv = len_symbol(t[1])
      out.append((257 + c, xb, xv, dist_symbol(t[2])))
    elif t[0] == 'l284':
      out.append((284, 5, t[1], dist_symbol(t[2])))
    elif t[0] == 'sym':
      out.append((t[1], 0, 0, None))
    elif t[0] == 'md':
      c, xb, xv = len_symbol(t[1])
      out.append((257 + c, xb, xv, (t[2], D.dist_extra(min(t[2], 29)), t[3])))
    else:
      raise ValueError(t)
  return out


def expand(tokens):
  """The bytes a token list of literals, 'm' and 'l284' tokens stands for."""
  out = bytearray()
  for t in tokens:
    if isinstance(t, int):
      out.append(t)
    else:
      length, dist = (t[1], t[2]) if t[0] == 'm' else (227 + t[1], t[2])
      assert 1 <= dist <= len(out)
      for _ in range(length):
        out.append(out[-dist])
  return bytes(out)


def _put_symbols(bw, syms, lcodes, dcodes):
  for s, xb, xv, d in syms + [(256, 0, 0, None)]:
    bw.code(*lcodes[s])
    bw.put(xv, xb)
    if d is not None:
      bw.code(*dcodes[d[0]])
      bw.put(d[2], d[1])


def fixed_block(bw, tokens, final=True):
  bw.put(1 if final else 0, 1)
  bw.put(1, 2)
  _put_symbols(bw, symbols(tokens), canonical(FIXED_LIT), canonical(FIXED_DIST))


def stored_block(bw, data, final=True, nlen=None):
  bw.put(1 if final else 0, 1)
  bw.put(0, 2)
  bw.align()
  bw.put(len(data), 16)
  bw.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
  for b in data:
    bw.put(b, 8)


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_PLAIN = [4] * 16 + [0, 0, 0]      # a complete code-length code: every length 0..15 in 4 bits, no repeat codes


def dynamic_header(bw, llens, dlens, final=True, hlit=None, hdist=None, cl_lens=None, cl_syms=None):
  """BFINAL, BTYPE 2 and the header of 3.2.7.  llens / dlens: the lengths sent (>= 257 and >= 1 of them); hlit, hdist:
  the raw 5-bit fields when they should not match; cl_lens: the code-length code's lengths (default CL_PLAIN); cl_syms:
  [(symbol, extra value)] sent instead of one plain symbol per length."""
  bw.put(1 if final else 0, 1)
  bw.put(2, 2)
  bw.put(len(llens) - 257 if hlit is None else hlit, 5)
  bw.put(len(dlens) - 1 if hdist is None else hdist, 5)
  cl = CL_PLAIN if cl_lens is None else cl_lens
  bw.put(19 - 4, 4)
  for s in CL_ORDER:
    bw.put(cl[s], 3)
  cc = canonical(cl)
  for s, x in (cl_syms if cl_syms is not None else [(l, 0) for l in list(llens) + list(dlens)]):
    bw.code(*cc[s])
    bw.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))


def dynamic_block(bw, tokens, final=True):
  """A dynamic block with Huffman codes made for its own tokens; returns (llens, dlens)."""
  syms = symbols(tokens)
  lf, df = {256: 1}, {}
  for s, _, _, d in syms:
    lf[s] = lf.get(s, 0) + 1
    if d is not None:
      df[d[0]] = df.get(d[0], 0) + 1
  llens = huffman_lengths(lf, 286)
  dlens = huffman_lengths(df, 30) if df else [0] * 30
  while len(llens) > 257 and llens[-1] == 0:
    llens.pop()
  while len(dlens) > 1 and dlens[-1] == 0:
    dlens.pop()
  dynamic_header(bw, llens, dlens, final)
  _put_symbols(bw, syms, canonical(llens), canonical(dlens))
  return llens, dlens


# ---- the named cases ------------------------------------------------------------------------------------------------
def _far_tokens():
  """32768 literals, a match at distance 32768 exactly (distance code 29, all 13 extra bits set), literals, and a longer
  one at the same distance."""
  lits = list(np.random.default_rng(5).integers(0x41, 0x5b, 32768, dtype=np.uint8).tolist())
  return lits + [('m', 3, 32768)] + [0x61, 0x62] + [('m', 200, 32768)]


def valid_cases(ref=None):
  """{name: (BGZF bytes, the bytes they inflate to)}.  ref: deflate_cases.Reference (the host restatement of the device
  deflate) for the eight-block members; without it those cases are left out."""
  text = D.text(70000, seed=3)
  cases = {
    'stored': (bgzf(text[:3000], 0), text[:3000]),
    'fixed': (bgzf(text[:20000], 6, zlib.Z_FIXED), text[:20000]),
    'dynamic1': (bgzf(text, 1), text),
    'dynamic6': (bgzf(text, 6), text),
    'dynamic9': (bgzf(text, 9), text),
    'zeros': (bgzf(bytes(65280), 6), bytes(65280)),
    'one_byte': (bgzf(b'x', 6), b'x'),
    'empty': (bgzf(b'', 6), b''),
    'eof_marker': (EOF, b''),
    'full_64k': (bgzf(text[:65536], 6, block=65536), text[:65536]),
    'small_blocks': (bgzf(text[:20000], 6, block=997), text[:20000]),
  }

  def hand(build):
    bw = Bits()
    data = build(bw)
    return member_of(bw.bytes(), data), data

  def far(bw):
    fixed_block(bw, _far_tokens())
    return expand(_far_tokens())
  cases['far_distance'] = hand(far)

  def len285(bw):
    t = list(b'abcdefg') + [('m', 258, 7), ('m', 258, 1), 0x7a]
    fixed_block(bw, t)
    return expand(t)
  cases['len_285'] = hand(len285)

  def len284(bw):   # symbol 284 with extra 30 (length 257) and with all five extra bits set (258: zlib takes it)
    t = list(b'0123456789') + [('l284', 30, 10), ('l284', 31, 3), ('l284', 0, 1)]
    dynamic_block(bw, t)
    return expand(t)
  cases['len_284_max_extra'] = hand(len284)

  def stored_after_dynamic(bw):
    t = list(b'mississippi river ') + [('m', 11, 18), ('m', 5, 4)]
    dynamic_block(bw, t, final=False)
    stored_block(bw, b'stored tail \x00\xff', final=False)
    fixed_block(bw, [0x21, ('m', 4, 1)], final=False)
    stored_block(bw, b'', final=True)
    return expand(t) + b'stored tail \x00\xff' + b'!!!!!'
  cases['stored_after_dynamic'] = hand(stored_after_dynamic)

  def single_distance(bw):   # every match at one distance code: the distance set is one code of length 1
    t = list(b'abcabc') + [('m', 9, 3), 0x58, ('m', 4, 3)]
    llens, dlens = dynamic_block(bw, t)
    assert sorted(l for l in dlens if l) == [1]
    return expand(t)
  cases['single_distance_code'] = hand(single_distance)

  if ref is not None:
    for name, data in (('device_grid', D.grid()), ('device_wide_tokens', D.wide_tokens()),
                       ('device_fibonacci', D.fibonacci_literals(0))):
      z, rep = ref(data)
      assert rep['stored_blocks'] == 0, name
      cases[name] = (z, data)
  return cases


def malformed_cases():
  """{name: (raw deflate, isize, crc)}: each refused by zlib (test_inflate_cpu.py asserts that first)."""
  data = D.text(5000, seed=9)
  good = raw_deflate(data, 6)
  crc = zlib.crc32(data)
  cases = {}

  def hand(name, build, out=b''):
    bw = Bits()
    build(bw)
    cases[name] = (bw.bytes(), len(out), zlib.crc32(out))

  def btype3(bw):
    bw.put(1, 1)
    bw.put(3, 2)
  hand('btype3', btype3)
  hand('len_nlen_mismatch', lambda bw: stored_block(bw, b'abc', nlen=0x1234), b'abc')

  def oversubscribed(bw):
    llens = [0] * 257
    llens[65] = llens[66] = llens[256] = 1
    dynamic_header(bw, llens, [1])
    bw.put(0, 8)
  hand('oversubscribed_litlen', oversubscribed)

  def incomplete(bw):
    llens = [0] * 257
    llens[65], llens[256] = 1, 2
    dynamic_header(bw, llens, [1])
    bw.code(0, 1)      # 'A'
    bw.code(2, 2)      # end of block
  hand('incomplete_litlen', incomplete, b'A')

  def repeat_first(bw):
    cl = [0] * 19
    cl[16], cl[1], cl[2] = 1, 2, 2
    dynamic_header(bw, [0] * 257, [1], cl_lens=cl, cl_syms=[(16, 0)] + [(1, 0)] * 255)
    bw.put(0, 8)
  hand('repeat16_first', repeat_first)

  def hlit287(bw):
    llens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 7      # 287 lengths
    dynamic_header(bw, llens, [5] * 30, hlit=30)
    bw.put(0, 16)
  hand('hlit_287', hlit287)
  hand('symbol_286', lambda bw: fixed_block(bw, [0x41, ('sym', 286)]), b'A')
  hand('distance_code_30', lambda bw: fixed_block(bw, [0x41, 0x42, 0x43, ('md', 3, 30, 0)]), b'ABCABC')
  hand('distance_too_far', lambda bw: fixed_block(bw, [0x41, ('m', 3, 2)]), b'AAAA')
  cases['cut_mid_symbol'] = (good[:len(good) // 2], len(data), crc)
  cases['one_byte_short'] = (raw_deflate(data[:-1], 6), len(data), crc)
  cases['one_byte_more'] = (raw_deflate(data + b'x', 6), len(data), crc)
  cases['crc_bit_flipped'] = (good, len(data), crc ^ 0x00010000)
  cases['wrong_isize'] = (good, len(data) + 7, crc)
  return cases


# ---- the decoder core on the host -------------------------------------------------------------------------------------
def build_tool(tmp_path_factory):
  """tests/inflate_host.cpp built the way deflate_cases.build_tool builds its tool, with the address and undefined
  behaviour sanitizers on the host side (a stand-alone program: it is run directly)."""
  out = str(tmp_path_factory.mktemp('inf') / 'inflate_host')
  subprocess.check_call(['/opt/rocm/bin/hipcc', '-O1', '-g', '-std=c++17', '-x', 'hip', '--offload-arch=gfx950',
                         '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                         '-Xarch_host', '-fno-omit-frame-pointer',
                         '-o', out, os.path.join(HERE, 'inflate_host.cpp')])
  return out


def run_core(tool, tmp, members):
  """The core's (status, bytes) for each (raw, isize, crc); any sanitizer report fails the run (exit status)."""
  src, dst = os.path.join(str(tmp), 'members'), os.path.join(str(tmp), 'inflated')
  with open(src, 'wb') as f:
    for raw, isize, crc in members:
      f.write(struct.pack('<III', len(raw), isize, crc & 0xffffffff) + raw)
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1')
  p = subprocess.run([tool, src, dst], stderr=subprocess.PIPE, env=env)
  assert p.returncode == 0, p.stderr.decode(errors='replace')[-4000:]
  out, o = [], 0
  with open(dst, 'rb') as f:
    z = f.read()
  while o < len(z):
    st, n = struct.unpack('<II', z[o:o + 8])
    out.append((st, z[o + 8:o + 8 + n]))
    o += 8 + n
  assert len(out) == len(members)
  return out
