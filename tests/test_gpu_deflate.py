"""The device BGZF compressor (mitty_amd/csrc/mh_deflate.hip) byte for byte against its host restatement
(tests/deflate_host.cpp --device-rules: the same parse, restated sequentially, with the same Huffman / header / CRC
code and the kernel's "store instead" rule).  The device's hash table is order-independent and every match is
extended to its true end, so the members must be identical — "it inflates" would not notice a dropped match, a
position never hashed in, or a path FASTQ never takes.  Every case also asserts, from the restatement's own report,
that its input has the shape it is named for (tests/deflate_cases.py builds the inputs).

Shapes the restatement reported for the committed seeds: grid — 5 slices, 199+ matches, length codes 4..28 and
distance codes 0..25 each at both ends of their extra bits; many symbols — 282 literal/length symbols in one slice;
code-length limiter — seeds 1134, 1262, 1339, 1360, 1370 each fold (unlimited depth 8 > 7); literal/length limiter —
4179 literals, no match, 17 symbols, unlimited depth 16 > 15; wide tokens — widest token 34 bits, 3 tokens over three
staging words, 2 of them with a bit set there."""
import ctypes
import gzip

import numpy as np
import pytest

from tests import deflate_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def native():
  from mitty_amd import _native
  if _native.device_count() == 0:
    pytest.fail('no HIP device: GPU tests must run on an MI355X')
  return _native


@pytest.fixture(scope='module')
def ctx(native):
  c = native.Context(0)
  yield c
  c.close()


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
  return C.Reference(C.build_tool(tmp_path_factory), tmp_path_factory.mktemp('ref'))


def _first_diff(a, b):
  n = min(len(a), len(b))
  d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
  return int(d[0]) if len(d) else n


def _stored_flags(z):
  """Per member: stored (one stored deflate block) or deflated."""
  out, o = [], 0
  for bsize, isize in C.bgzf_members(z):
    out.append(bsize == 18 + 5 + isize + 8 and z[o + 18] == 1)
    o += bsize
  return out


def _identity(native, z, data, ref, what):
  """The oracle of every case: z (the device's members for data) equals the restatement's; returns its report."""
  want, rep = ref(data)
  assert z == want, '{}: {} device bytes, {} reference bytes, first difference at byte {}'.format(
    what, len(z), len(want), _first_diff(z, want))
  assert gzip.decompress(z + native.bgzf_eof()) == data, what
  members = C.bgzf_members(z)
  assert sum(m[1] for m in members) == len(data) and len(members) == (len(data) + C.BLOCK - 1) // C.BLOCK, what
  assert len(z) <= C.bgzf_bound(len(data)), what
  assert rep['blocks'] == len(members) and rep['stored_blocks'] == sum(_stored_flags(z)), what
  return rep


def _check(native, ctx, ref, data, what):
  return _identity(native, ctx.selftest_bgzf(data), data, ref, what)


# ---- sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', C.SIZES)
def test_sizes(native, ctx, ref, n):
  """Compressible text of n bytes: the CRC with no whole segment, no partial one, a partial one that is no multiple
  of 4; a last slice of 1..6 bytes (no position long enough to match); the final-block flag when n is a multiple of
  the slice; tiny blocks the store rule catches."""
  rep = _check(native, ctx, ref, C.sized(n), 'text[:{}]'.format(n))
  if n >= 264:
    assert rep['stored_blocks'] < rep['blocks'] and rep['matches'] > 0


def test_sizes_cover_stored_and_deflated_last_blocks(ref):
  last = {n: _stored_flags(ref(C.sized(n))[0])[-1] for n in C.SIZES}
  assert any(last.values()) and not all(last.values())
  assert all(last[n] for n in range(1, 9)), last                     # tot >= 5 + n
  assert not last[2 * C.BLOCK] and last[2 * C.BLOCK + 1], last       # a whole second block | one byte of it


# ---- periodic -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', C.PERIODS)
def test_periodic(native, ctx, ref, p):
  """A random base of period p over one block plus 777 bytes: chains of 258-byte matches at distance p (the
  positions inside a long match must be hashed in for the next one to be found at that distance)."""
  rep = _check(native, ctx, ref, C.periodic(p), 'period {}'.format(p))
  if p >= 8153:
    assert rep['stored_blocks'] == 2          # a slice holds at most 7 bytes of repeat: nothing gained
  else:
    assert 28 in rep['len_codes'] and rep['matches'] >= 100
    # the matches are at distance p wherever the base's first period is in the table
    dc = [c for c in range(30) if C.dist_base(c) <= p < C.dist_base(c) + (1 << C.dist_extra(c))][0]
    assert dc in rep['dist_codes']


def test_periodic_family_has_steps_over_two_windows(ref):
  """Somewhere in the family a step's last token starts near the end of its 256 positions and runs on for a whole
  match: a span of 500 or more (hash_in's second loop over the positions past the window)."""
  assert max(ref(C.periodic(p))[1]['max_step_span'] for p in C.PERIODS) >= 500


# ---- the code tables ------------------------------------------------------------------------------------------------
def test_length_and_distance_grid(native, ctx, ref):
  """Every length code 4..28 and distance code 0..25, each code with extra bits at its lowest value and at its
  highest that fits a slice (lengths 257 and 258 both; the farthest match a slice can hold)."""
  rep = _check(native, ctx, ref, C.grid(), 'grid')
  assert set(rep['len_codes']) >= set(range(4, 29)) and set(rep['dist_codes']) >= set(range(26))
  for c, ext in C.LEN_EXTREMES.items():
    assert rep['len_extra'][str(c)] == list(ext), ('length code', c)
  for c, ext in C.DIST_EXTREMES.items():
    assert rep['dist_extra'][str(c)] == list(ext), ('distance code', c)
  assert C.LEN_EXTREMES[27] == (0, 30) and C.DIST_EXTREMES[25] == (0, C.SLICE - 7 - 6145)
  assert rep['stored_blocks'] == 0


def test_many_symbols(native, ctx, ref):
  """One slice with all 256 literals, the end of block and all 25 length codes: wave_sort over 512 slots and
  wave_huffman's compaction over five rounds of 64 symbols."""
  rep = _check(native, ctx, ref, C.many_symbols(), 'many symbols')
  assert rep['slices'] == 1 and rep['max_lit_syms'] >= 280 and rep['stored_blocks'] == 0


CL_SEEDS = [1134, 1262, 1339, 1360, 1370]


@pytest.mark.parametrize('seed', CL_SEEDS)
def test_code_length_limiter(native, ctx, ref, seed):
  """Literal profiles whose code-length code is deeper than 7 bits before the limiter folds it (lane 0 of the wave
  runs huffman_from_sorted's fold; the header then carries the folded code)."""
  rep = _check(native, ctx, ref, C.cl_profile(seed), 'code-length profile {}'.format(seed))
  assert rep['slices'] == 1 and rep['fold_cl'] == 1 and rep['max_depth_cl'] > 7 and rep['stored_blocks'] == 0


@pytest.mark.parametrize('seed', [0, 1])
def test_literal_length_limiter(native, ctx, ref, seed):
  """Fibonacci literal counts and not one match: the literal/length tree is a chain 16 deep and the 15-bit limiter
  folds it on the device."""
  rep = _check(native, ctx, ref, C.fibonacci_literals(seed), 'fibonacci literals {}'.format(seed))
  assert rep['matches'] == 0 and rep['fold_lit'] == 1 and rep['max_depth_lit'] > 15 and rep['stored_blocks'] == 0


WIDE_SEEDS = [23, 33]   # (blocks whose report shows a third-word token with a bit set past the second word)


def test_wide_tokens(native, ctx, ref):
  """Rare far matches with 5 + 11 extra bits and deep codes among thousands of 2-bit literals: tokens of 34 bits and
  more, some starting so late in a staging word that they reach a third one (stage_or's last OR)."""
  data = b''.join(C.wide_tokens(s) for s in WIDE_SEEDS)
  rep = _check(native, ctx, ref, data, 'wide tokens')
  assert rep['max_token_bits'] >= 34 and rep['third_word_tokens'] >= 1 and rep['stored_blocks'] == 0
  assert rep['third_word_set'] >= 1   # ... with a 1 among the bits that land in the third word


# ---- members, alignment, scratch reuse ----------------------------------------------------------------------------
def _mixed():
  rng = np.random.default_rng(99)
  return C.sized(C.BLOCK) + rng.integers(0, 256, C.BLOCK, dtype=np.uint8).tobytes() + b'tail\n'


def test_mixed_members(native, ctx, ref):
  """A deflated, a stored and a 5-byte member in one call: every offset from the scan of the members' sizes."""
  data = _mixed()
  rep = _check(native, ctx, ref, data, 'mixed')
  assert _stored_flags(ref(data)[0]) == [False, True, True] and rep['blocks'] == 3


def _two_blocks():
  rng = np.random.default_rng(98)
  return C.sized(C.BLOCK - 3000) + rng.integers(0, 256, 3000, dtype=np.uint8).tobytes() + C.grid()[:30011]


@pytest.mark.parametrize('misalign', range(1, 16))
def test_misaligned_source(native, ctx, ref, misalign):
  """The block staged byte by byte (a source that is not 16-byte aligned: BAM windows, odd arena offsets) gives the
  bytes of the aligned staging."""
  data = _two_blocks()
  z = ctx.selftest_bgzf(data, misalign)
  assert z == ctx.selftest_bgzf(data, 0)
  rep = _identity(native, z, data, ref, 'misalign {}'.format(misalign))
  assert rep['blocks'] == 2 and rep['stored_blocks'] == 0


def _all_cases():
  return ([C.sized(n) for n in C.SIZES] + [C.periodic(p) for p in C.PERIODS] +
          [C.grid(), C.many_symbols(), _mixed(), _two_blocks()] + [C.cl_profile(s) for s in CL_SEEDS] +
          [C.fibonacci_literals(0), b''.join(C.wide_tokens(s) for s in WIDE_SEEDS)])


def test_stale_scratch(native, ctx, ref):
  """Every case forward and then reversed in one context: the slots, the token area and the block info are reused
  (a larger case's leftovers under a smaller one), and the bytes are the reference's each time."""
  cases = _all_cases()
  for i, data in enumerate(cases + cases[::-1]):
    want = ref(data)[0]
    z = ctx.selftest_bgzf(data, i % 16 if i % 3 == 0 else 0)
    assert z == want, 'case {} of the sequence: first difference at byte {}'.format(i, _first_diff(z, want))


def test_arena_range_at_odd_offset(native, ref):
  """mh_output_bgzf_range at an odd offset and odd length into a unit's FASTQ arena: the reference's members of
  d1[off:off + n]."""
  from mitty_amd import synth
  from mitty_amd.engine import Engine
  from tests import golden_io as G
  mdl = G.model('hiseq-X-v2.5-Garvan')
  p, _ = native.read_model_params(mdl['mean_rlen'], 10.0)
  seq = synth.contig(100_000, 5)
  copies = synth.copies_soa(synth.variants(seq, 6), 0, len(seq))
  eng = Engine(0)
  pin = native.PinnedBuffer()
  try:
    eng.load_region(0, ('7', 0, len(seq)), seq)
    eng.ctx.reset_output()
    eng.run_unit(0, 0, 0, 99, copies[0], p, mdl['mean_rlen'], mdl['cum_tlen'], 'SYN')
    d1, _ = eng.ctx.fetch_output()
    off, n = 12345, C.BLOCK + 4321
    assert len(d1) >= off + n and off % 2 == 1 and n % 2 == 1
    z = eng.ctx.bgzf_range(0, off, n, pin)
    rep = _identity(native, z, bytes(d1[off:off + n]), ref, 'arena range')
    assert rep['blocks'] == 2 and rep['stored_blocks'] == 0
  finally:
    pin.free()
    eng.close()


def test_capacity(native, ctx, ref):
  """mh_bgzf_compress_gpu: one byte short is MH_E_CAPACITY with the needed size reported; the exact size succeeds."""
  data = _mixed()
  want = ref(data)[0]
  src = np.frombuffer(data, np.uint8)
  out = np.zeros(len(want) + 16, np.uint8)
  used = ctypes.c_int64()
  rc = ctx._L.mh_bgzf_compress_gpu(ctx._h, src.ctypes.data, len(data), out.ctypes.data, len(want) - 1,
                                   ctypes.byref(used))
  assert rc == native.MH_E_CAPACITY and used.value == len(want)
  rc = ctx._L.mh_bgzf_compress_gpu(ctx._h, src.ctypes.data, len(data), out.ctypes.data, len(want), ctypes.byref(used))
  assert rc == native.MH_OK and used.value == len(want)
  assert out[:len(want)].tobytes() == want and not out[len(want):].any()
