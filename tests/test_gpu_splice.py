"""Known-answer tests of the haplotype splice (mh_splice.hip) on adversarial variant lists.

Every case builds one haplotype through the library and compares, by exact array equality, the node list (count, ps,
pr, op, oplen), the haplotype bytes, and what the splice derives from them and only emission otherwise sees — the
reverse complement, both sorted N-run lists, the node-search bucket table (mh_get_haplotype_aux) — and p_min / p_max
with a plain restatement from the oracle's node arrays (tests/splice_ref.py).  The lists sit where the kernels change
path: non-anchor runs across a 256-thread block and a 2048-element scan tile (k_resolve), more and fewer than 512
nodes per workgroup span and up to 32 nodes in one 16-byte chunk (k_hap_fill), insertions longer than a span, lengths
around every chunk size (k_hap_rc's tail, k_nrun_find's masks), N-run counts around the boundary capacity (4096), the
LDS sort's limit (8192) and beyond it.  Each case asserts on the CPU side that its list has the shape it claims, so it
cannot pass vacuously.  All inputs are valid per the API's contract, except in the two error-return tests."""
import numpy as np
import pytest

from tests import splice_ref as R
from tests.splice_ref import D, I, X

pytestmark = pytest.mark.gpu

RS = 5001                 # region start: region and contig coordinates differ
SPAN = R.FILL_SPAN
CID, VSET = 3, 11         # contig and variant-set ids (anything but 0)


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


# ---- build one haplotype and compare everything ------------------------------------------------------------------
SIDE_REF = R.contig(3000, 99)
SIDE_V = R.soa([40, 41, 900, 2000], [X, I, D, X], [0, 7, 30, 0], seed=98)


def _compare(ctx, slot, res, want, what, n_var):
  """The slot's contents against want (an R.Expect); res = (n_nodes, p_min, p_max) as the build returned them, or
  None for a prefetched build (which returns nothing: its node count is then read off the bucket table's last entry,
  the number of nodes keyed below a position past every key)."""
  cap = 2 * n_var + 1                        # the most nodes n_var variants make: the read-back buffers' size
  if res is not None:
    assert res[0] == want.n_nodes, '{}: {} nodes for {}'.format(what, res[0], want.n_nodes)
    assert (res[1], res[2]) == (want.p_min, want.p_max), '{}: p_min, p_max {} for {}'.format(
      what, res[1:], (want.p_min, want.p_max))
  ps, pr, op, ol, hap = ctx.get_nodes(slot, cap)
  rc, run_s, run_e, bkt = ctx.get_haplotype_aux(slot)
  n = want.n_nodes
  for name, got, exp in (('ps', ps, want.ps), ('pr', pr, want.pr), ('op', op, want.op), ('oplen', ol, want.oplen)):
    R.same(got[:n], exp, '{}: node {}'.format(what, name),
           lambda k: 'node {} {!r} of variant {}'.format(k, chr(want.op[k]), want.variant_of_node(k)))
  assert len(hap) == len(want.hap), '{}: haplotype of {} bytes for {}'.format(what, len(hap), len(want.hap))
  R.same(hap, want.hap, what + ': haplotype bytes', R.span_of)
  R.same(rc, want.rc, what + ': reverse complement', R.span_of)
  assert len(run_s) == len(want.run_start), '{}: {} N runs for {}'.format(what, len(run_s), len(want.run_start))
  where = lambda r: 'run at offset {}, {}'.format(want.run_start[r], R.span_of(int(want.run_start[r])))
  R.same(run_s, want.run_start, what + ': N-run starts', where)
  R.same(run_e, want.run_end, what + ': N-run ends', where)
  R.same(bkt, want.bkt, what + ': bucket table', lambda k: 'bucket {}, {}'.format(k, R.span_of(k * R.BKT)))
  assert int(bkt[-1]) == want.n_nodes


def _check(ctx, ref, rs, v, what, slot=0, lane=0, want=None):
  """Build (ref, rs, v) in `slot` through one of the library's build paths and compare.  lane 0: mh_build_haplotype;
  'vset': resident variants, mh_build_haplotype_vset; 1: the second copy of mh_build_haplotypes_vset (its own stream,
  host thread and scratch); 2: mh_prefetch_haplotypes_vset (the prefetch thread's)."""
  want = want or R.Expect(ref, rs, v)
  n_var = len(v['pos'])
  ctx.upload_contig(CID, ref)
  if lane == 0:
    res = ctx.build_haplotype(slot, CID, rs, v)
  else:
    ctx.upload_variants(VSET, v)
    if lane == 'vset':
      res = ctx.build_haplotype_vset(slot, CID, rs, VSET)
    elif lane == 1:
      ctx.upload_contig(CID + 1, SIDE_REF)
      ctx.upload_variants(VSET + 1, SIDE_V)
      side, res = ctx.build_haplotypes_vset([slot + 1, slot], [CID + 1, CID], [7, rs], [VSET + 1, VSET])
      _compare(ctx, slot + 1, side, R.Expect(SIDE_REF, 7, SIDE_V), what + ' (the copy beside it)', 4)
    else:
      ctx.release_haplotype(slot)            # (a prefetch takes a free slot)
      ctx.prefetch_haplotypes_vset([slot], [CID], [rs], [VSET])
      res = None
  _compare(ctx, slot, res, want, what, n_var)
  return want


# ---- the accept chain (k_resolve) ----------------------------------------------------------------------------------
def shadowed_run(m, lead=0):
  """`lead` far-apart SNPs (anchors), then a deletion, then a long deletion that starts inside the first — rejected,
  but every later variant up to its end is a non-anchor — over m SNPs 3 bases apart, each accepted one by one."""
  p0 = RS + 10 + 20 * lead
  pos = np.concatenate((RS + 10 + 20 * np.arange(lead), [p0, p0 + 5], p0 + 11 + 3 * np.arange(m)))
  op = np.concatenate((np.full(lead, X), [D, D], np.full(m, X))).astype(np.uint8)
  oplen = np.concatenate((np.zeros(lead), [10, 3 * m + 10], np.zeros(m))).astype(np.int64)
  ref = R.contig(int(pos[-1]) - RS + 300, 1000 + m)
  return ref, RS, R.soa(pos, op, oplen, seed=m)


def _shadowed_pre(want, m, lead):
  runs = R.run_lengths(~want.anchor)
  assert int(want.anchor.sum()) == lead + 1 and list(runs) == [m + 1]
  assert int(np.flatnonzero(~want.anchor)[0]) == lead + 1          # the run's first variant
  assert int((want.accepted & ~want.anchor).sum()) == m and int((~want.accepted).sum()) == 1


@pytest.mark.parametrize('m', [1, 2, 255, 256, 257, 2047, 2048, 2049, 30000])
def test_shadowed_run(ctx, m):
  ref, rs, v = shadowed_run(m)
  want = R.Expect(ref, rs, v)
  _shadowed_pre(want, m, 0)
  _check(ctx, ref, rs, v, 'shadowed run of {}'.format(m), want=want)


@pytest.mark.parametrize('first', [255, 256, 2048])
def test_shadowed_run_starting_at(ctx, first):
  """The non-anchor run starts at variant index `first` (the last thread of a block, the first of the next, the first
  of a scan tile) and crosses several blocks."""
  ref, rs, v = shadowed_run(3000, first - 1)
  want = R.Expect(ref, rs, v)
  _shadowed_pre(want, 3000, first - 1)
  _check(ctx, ref, rs, v, 'shadowed run from variant {}'.format(first), want=want)


def dense_overlaps(seed, n=60000, length=300000):
  rng = np.random.default_rng(seed)
  pos = np.sort(rng.integers(RS, RS + length - 60, n))
  op = np.array([X, X, I, D], np.uint8)[rng.integers(0, 4, n)]
  oplen = np.minimum(rng.geometric(0.3, n), 50)
  return R.contig(length, seed + 1), RS, R.soa(pos, op, oplen, seed=seed + 2)


@pytest.mark.parametrize('seed', [11, 12, 13])
def test_dense_random_overlaps(ctx, seed):
  ref, rs, v = dense_overlaps(seed)
  want = R.Expect(ref, rs, v)
  na = ~want.anchor
  runs = R.run_lengths(na)
  print('anchors {} accepted non-anchors {} rejected {} longest non-anchor run {}'.format(
    int(want.anchor.sum()), int((want.accepted & na).sum()), int((~want.accepted).sum()), int(runs.max())))
  assert (want.accepted & na).sum() > 100 and (~want.accepted & na).sum() > 100 and runs.max() >= 4
  assert want.accepted[want.anchor].all()
  _check(ctx, ref, rs, v, 'dense overlaps, seed {}'.format(seed), want=want)


def test_first_variants_before_the_region(ctx):
  """Variants at rs - 3 .. rs - 1 are skipped (their position is before the ref cursor, which starts at rs), a
  deletion from before rs into the region included; none of them is an anchor, so the first thread of k_resolve
  walks them from a cursor of rs."""
  ref = R.contig(700, 5)
  lists = [
    [(RS - 1, 'X', 0, b'T')],
    [(RS - 3, 'X', 0, b'G'), (RS - 2, 'I', 2, b'ACC'), (RS - 1, 'D', 5, b'A'), (RS, 'X', 0, b'T'),
     (RS + 1, 'I', 3, b'AGGT'), (RS + 3, 'D', 2, b'C'), (RS + 10, 'X', 0, b'A'), (RS + 40, 'X', 0, b'C')],
    [(RS - 2, 'D', 1, b'A'), (RS, 'D', 4, b'T'), (RS + 2, 'X', 0, b'G'), (RS + 5, 'X', 0, b'G')],
    [(RS - 1, 'D', 300, b'A'), (RS + 100, 'X', 0, b'T'), (RS + 299, 'I', 1, b'AT'), (RS + 300, 'X', 0, b'T')],
  ]
  for k, vl in enumerate(lists):
    v = R.soa_of(vl)
    want = R.Expect(ref, RS, v)
    assert not want.anchor[0] and not want.accepted[0]
    assert not want.accepted[v['pos'] < RS].any() and (k == 0 or want.accepted.any())
    _check(ctx, ref, RS, v, 'variants before the region, list {}'.format(k), want=want)


def test_equal_positions(ctx):
  ref = R.contig(500, 6)
  p = RS + 100
  lists = [
    [(p, 'X', 0, b'T'), (p, 'I', 2, b'ACC')],
    [(p, 'I', 2, b'ACC'), (p, 'X', 0, b'T')],
    [(p, 'D', 3, b'A'), (p, 'X', 0, b'T')],
    [(p, 'D', 3, b'A'), (p + 3, 'I', 2, b'ACC')],        # on the deletion's last base: rejected
    [(p, 'D', 3, b'A'), (p + 4, 'I', 2, b'ACC')],        # directly after it: accepted
    [(p, 'X', 0, b'T'), (p, 'X', 0, b'G'), (p + 1, 'X', 0, b'G'), (p + 1, 'D', 2, b'C'), (p + 2, 'I', 1, b'AT')],
  ]
  n_acc = [1, 1, 1, 1, 2, 3]
  for k, vl in enumerate(lists):
    v = R.soa_of(vl)
    want = R.Expect(ref, RS, v)
    assert int(want.accepted.sum()) == n_acc[k]
    _check(ctx, ref, RS, v, 'equal positions, list {}'.format(k), want=want)


def test_empty_and_single(ctx):
  ref = R.contig(300, 7)
  for vl in ([], [(RS + 50, 'X', 0, b'T')], [(RS + 50, 'I', 4, b'ACCGT')], [(RS + 50, 'D', 4, b'A')],
             [(RS, 'X', 0, b'T')], [(RS, 'I', 1, b'AC')], [(RS, 'D', 1, b'A')], [(RS + 299, 'X', 0, b'T')]):
    v = R.soa_of(vl)
    want = R.Expect(ref, RS, v)
    assert want.n_nodes == (1 if not vl else 3 if vl[0][0] > RS or vl[0][1] != 'X' else 2)
    _check(ctx, ref, RS, v, 'list {}'.format(vl), want=want)


def test_deletion_to_and_past_the_region_end(ctx):
  """The last deletion ends exactly at the region's end (a trailing '=' node of no bases follows), then one base
  past it (no trailing node: the list ends with the 'D' node, from which p_max is taken)."""
  L = 1000
  ref = R.contig(L, 8)
  for past in (0, 1):
    v = R.soa_of([(RS + 200, 'X', 0, b'T'), (RS + 900, 'D', L - 901 + past, b'A')])
    want = R.Expect(ref, RS, v)
    assert chr(want.op[-1]) == ('D' if past else '=') and want.oplen[-1] == (L - 901 + past if past else 0)
    assert len(want.hap) == 901
    _check(ctx, ref, RS, v, 'deletion {} past the end'.format(past), want=want)


# ---- the byte fill (k_hap_fill) and the reverse complement -----------------------------------------------------------
def every_base(kind, n):
  if kind == 'X':
    return R.contig(n, 21), RS, R.soa(RS + np.arange(n), np.full(n, X), np.zeros(n), seed=22)
  if kind == 'D':      # one-base deletions at every other base
    return R.contig(n, 23), RS, R.soa(RS + 2 * np.arange(n // 2), np.full(n // 2, D), np.ones(n // 2), seed=24)
  return R.contig(n, 25), RS, R.soa(RS + np.arange(n), np.full(n, I), np.ones(n), seed=26)


@pytest.mark.parametrize('kind,n', [('X', 50001), ('D', 70000), ('I', 30001)])
def test_node_density_whole_contig(ctx, kind, n):
  """Every span needs far more than 512 nodes (searched in global memory); with deletions at every other base a
  16-byte chunk meets 32 nodes (16 '=' and 16 'D'), the most the chunk loop's bound of 40 has to cover: a 'D' node
  always follows an '=' node, so 16 positions hold at most 16 byte-holding nodes and 16 'D' nodes."""
  ref, rs, v = every_base(kind, n)
  want = R.Expect(ref, rs, v)
  spans, chunk = want.span_nodes(), want.chunk_nodes()
  print('nodes per span (max) {} per 16-byte chunk {} spans {}'.format(int(spans.max()), chunk, len(spans)))
  assert len(spans) >= 3 and spans.max() > R.FILL_NODES and want.accepted.all()
  assert chunk == {'X': 16, 'D': 32, 'I': 16}[kind] and spans.max() >= {'X': 16384, 'D': 32768, 'I': 16384}[kind]
  _check(ctx, ref, rs, v, 'an {} at every base'.format(kind), want=want)


def busy_staged():
  """One SNP per 2 kbp, and around haplotype offsets 16384 k - 8: 200 adjacent SNPs (k = 1, 2, 3), then one-base
  deletions at 100 alternate bases (k = 4, 5, 6; placed by the bases deleted before them)."""
  n = 8 * SPAN
  pos, op = [np.arange(700, n - 500, 2000)], [np.full(len(np.arange(700, n - 500, 2000)), X)]
  for k in (1, 2, 3):
    pos.append(SPAN * k - 8 - 100 + np.arange(200))
    op.append(np.full(200, X))
  for j, k in enumerate((4, 5, 6)):
    pos.append(SPAN * k - 8 - 50 + 100 * j + 2 * np.arange(100))
    op.append(np.full(100, D))
  pos, op = np.concatenate(pos), np.concatenate(op).astype(np.uint8)
  order = np.argsort(pos, kind='stable')
  pos, op = pos[order], op[order]
  keep = np.concatenate(([True], np.diff(pos) > 0))     # (a background SNP inside a cluster: dropped)
  pos, op = pos[keep], op[keep]
  return R.contig(n, 31), RS, R.soa(RS + pos, op, np.ones(len(pos)), seed=32)


def test_staged_path_with_busy_chunks(ctx):
  ref, rs, v = busy_staged()
  want = R.Expect(ref, rs, v)
  spans = want.span_nodes()
  print('nodes per span {} per 16-byte chunk {}'.format(spans.tolist(), want.chunk_nodes()))
  assert spans.max() <= R.FILL_NODES and spans.max() > 200 and want.accepted.all()
  assert want.chunk_nodes() >= 30
  off = want.keys - want.p_min
  for k in range(1, 7):      # each cluster has nodes on both sides of its span boundary, in the chunks beside it
    assert ((off >= SPAN * k - 16) & (off < SPAN * k)).sum() >= 8 and \
           ((off >= SPAN * k) & (off < SPAN * k + 16)).sum() >= 8, k
  _check(ctx, ref, rs, v, 'busy chunks on the staged path', want=want)


def test_long_insertions(ctx):
  """An insertion of 40000 bases (whole spans lie inside one node) and one of 16384 whose first base is the first
  byte of a span; an SNP directly follows each."""
  ref = R.contig(70000, 41)
  rng = np.random.default_rng(42)
  ins = [b'A' + R.ACGT[rng.integers(0, 4, n)].tobytes() for n in (40000, SPAN)]
  p2 = RS + (4 * SPAN - 40000) - 1
  v = R.soa_of([(RS + 1000, 'I', 40000, ins[0]), (RS + 1001, 'X', 0, b'T'), (p2, 'I', SPAN, ins[1]),
                (p2 + 1, 'X', 0, b'G')])
  want = R.Expect(ref, RS, v)
  isi = want.op == I
  assert want.accepted.all() and list(want.oplen[isi]) == [40000, SPAN]
  assert (want.ps[isi][1] - want.p_min) % SPAN == 0 and (want.ps[isi][0] - want.p_min) % 16 != 0
  assert want.span_nodes().max() <= R.FILL_NODES
  _check(ctx, ref, RS, v, 'long insertions', want=want)


LENGTHS = [1, 15, 16, 17, 63, 64, 65, 16383, 16384, 16385, 65537]


def test_length_sweep(ctx):
  """Haplotype lengths around a 16-byte chunk, a 64-position N-run word and a span: contigs of that length without
  variants, and with one 3-base insertion that moves the length off the multiple (k_hap_rc's tail, the last partial
  chunk of k_hap_fill, k_nrun_find's masks at the end).  Each contig ends in 'N' so the last run ends at hap_len."""
  for n in LENGTHS:
    ref = R.contig(n, 50 + n)[:-1] + b'N'
    for ins in (False, True):
      v = R.soa_of([(RS + (n - 1) // 2, 'I', 3, b'AGTN')] if ins else [])
      want = R.Expect(ref, RS, v)
      assert len(want.hap) == n + 3 * ins and want.run_end[-1] == len(want.hap)
      _check(ctx, ref, RS, v, 'length {}{}'.format(n, ' + 3' if ins else ''), want=want)


# ---- N runs ----------------------------------------------------------------------------------------------------------
def n_every_other(runs, tail=37):
  """A contig with `runs` single 'N's at odd offsets 1, 3, 5, ... and `tail` more bases."""
  a = np.frombuffer(R.contig(2 * runs + tail, 60 + runs), np.uint8).copy()
  a[1:2 * runs:2] = R.N
  return a.tobytes()


@pytest.mark.parametrize('runs', [0, 1, 3, 1000, 4095, 4096, 4097, 8191, 8192, 8193, 150000])
def test_n_run_counts(ctx, runs):
  """Run counts around the first boundary capacity (4096: one more is found again with room for all), the LDS
  bitonic sort's padding (counts that are no power of two) and limit (8192), and the radix sort beyond it."""
  ref = n_every_other(runs)
  v = R.soa_of([])
  want = R.Expect(ref, RS, v)
  assert len(want.run_start) == runs and (want.run_end - want.run_start == 1).all()
  # a fresh context: the capacity of the first attempt grows with the slot's N-run buffers
  from mitty_amd import _native
  c = _native.Context(0)
  try:
    _check(c, ref, RS, v, '{} N runs'.format(runs), want=want)
    if runs == 8193:    # and a second, smaller list into the same, larger buffers
      ref2 = n_every_other(4097)
      _check(c, ref2, RS, v, '4097 N runs after 8193')
  finally:
    c.close()


def test_n_run_placement(ctx):
  def with_n(n, runs, seed):
    a = np.frombuffer(R.contig(n, seed), np.uint8).copy()
    for s, e in runs:
      a[s:e] = R.N
    return a.tobytes()

  none = R.soa_of([])
  cases = [('a run at offset 0', with_n(200, [(0, 3)], 70), none, [(0, 3)])]
  for n in (128, 129, 191, 192, 64, 63):          # hap_len % 64 in {0, 1, 63}
    cases.append(('a run ending at hap_len = {}'.format(n), with_n(n, [(n - 5, n)], 71 + n), none, [(n - 5, n)]))
  cases.append(('all N, 64 bases', b'N' * 64, none, [(0, 64)]))
  cases.append(('all N, 1 base', b'N', none, [(0, 1)]))
  on64 = [(63, 64), (64 + 64, 192), (250, 256), (320, 330), (383, 385), (448, 449)]
  cases.append(('runs on multiples of 64', with_n(600, on64, 72), none, on64))
  ref = with_n(400, [(100, 106), (200, 203), (206, 209)], 73)
  cases.append(('an N inside an insertion', ref, R.soa_of([(RS + 50, 'I', 5, b'ACNNGN')]),
                [(52, 54), (55, 56), (105, 111), (205, 208), (211, 214)]))
  cases.append(('a run split by an insertion', ref, R.soa_of([(RS + 102, 'I', 3, b'NACG')]),
                [(100, 103), (106, 109), (203, 206), (209, 212)]))
  cases.append(('two runs joined by a deletion', ref, R.soa_of([(RS + 202, 'D', 3, b'N')]), [(100, 106), (200, 206)]))
  for what, ref, v, runs in cases:
    want = R.Expect(ref, RS, v)
    assert list(zip(want.run_start.tolist(), want.run_end.tolist())) == runs, what
    _check(ctx, ref, RS, v, what, want=want)


def test_stale_bytes_of_a_larger_buffer(native):
  """A 300 kbp haplotype with an 'N' at every other base, released; then a 1000-base haplotype without 'N' built into
  the same slot takes over its buffers: no run, and the bytes, of the second."""
  c = native.Context(0)
  try:
    ref = n_every_other(150000, tail=1)
    _check(c, ref, RS, R.soa_of([]), 'the larger haplotype', slot=5)
    c.release_haplotype(5)
    for n in (1000, 1001, 1023):
      ref2 = R.contig(n, 80)
      want = R.Expect(ref2, RS, R.soa_of([]))
      assert len(want.run_start) == 0 and R.N in ref[n:n + 2]      # (stale 'N's right behind the new end)
      _check(c, ref2, RS, R.soa_of([]), 'a {}-base haplotype in the larger one\'s buffers'.format(n), slot=5, want=want)
    # and with the stale 'N's at even offsets, under lengths that are a multiple of 16: the fill writes whole 16-byte
    # chunks (zeros past the end), so only then is the byte at hap_len itself, which k_nrun_find loads, a stale 'N'
    _check(c, ref[1:], RS, R.soa_of([]), 'the larger haplotype, shifted', slot=5)
    c.release_haplotype(5)
    for n in (1008, 1024):
      ref2 = R.contig(n, 81)
      want = R.Expect(ref2, RS, R.soa_of([]))
      assert len(want.run_start) == 0 and ref[1:][n] == R.N
      _check(c, ref2, RS, R.soa_of([]), 'a {}-base haplotype in the larger one\'s buffers'.format(n), slot=5, want=want)
  finally:
    c.close()


@pytest.fixture(scope='module')
def lane_cases():
  """Four of the lists above with their expectations, computed once for the three lanes (read-only)."""
  out = []
  for what, (ref, rs, v) in (('shadowed run of 30000', shadowed_run(30000)), ('dense overlaps', dense_overlaps(11)),
                             ('deletions at every other base', every_base('D', 70000)),
                             ('8193 N runs', (n_every_other(8193), RS, R.soa_of([])))):
    out.append((what, ref, rs, v, R.Expect(ref, rs, v)))
  return out


@pytest.mark.parametrize('lane', ['vset', 1, 2])
def test_build_lanes(native, lane_cases, lane):
  """The same lists through the other build paths, each with a stream and scratch buffers of its own: resident
  variants (mh_build_haplotype_vset), the second copy of mh_build_haplotypes_vset, mh_prefetch_haplotypes_vset."""
  c = native.Context(0)
  try:
    for what, ref, rs, v, want in lane_cases:
      _check(c, ref, rs, v, '{} (lane {})'.format(what, lane), slot=8, lane=lane, want=want)
  finally:
    c.close()


# ---- error returns -----------------------------------------------------------------------------------------------------
def _refused(ctx, native, ref, v, message):
  ctx.upload_contig(CID, ref)
  with pytest.raises((ValueError, native.NativeError), match=message):
    ctx.build_haplotype(0, CID, RS, v)
  good = R.soa_of([(RS + 10, 'X', 0, b'T'), (RS + 20, 'I', 2, b'ACC'), (RS + 30, 'D', 2, b'A')])
  _check(ctx, ref, RS, good, 'a valid build after the refused one')


def test_variant_beyond_the_region_is_refused(ctx, native):
  """A variant whose '=' node would run past the fetched region: refused (no byte of such a list is gathered), and the
  next build in the same context is right."""
  ref = R.contig(1000, 90)
  msg = 'variant beyond the end of the fetched reference region'
  _refused(ctx, native, ref, R.soa_of([(RS + 100, 'X', 0, b'T'), (RS + 1005, 'X', 0, b'G')]), msg)
  _refused(ctx, native, ref, R.soa_of([(RS + 1000, 'I', 2, b'ACC')]), msg)


def test_inconsistent_alt_length_is_refused(ctx, native):
  ref = R.contig(1000, 91)
  msg = 'SNP/INS alt length inconsistent with its op'
  _refused(ctx, native, ref, R.soa_of([(RS + 100, 'X', 0, b'TG')]), msg)
  _refused(ctx, native, ref, R.soa_of([(RS + 100, 'I', 3, b'ACC')]), msg)
  _refused(ctx, native, ref, R.soa_of([(RS + 100, 'X', 0, b'T'), (RS + 200, 'I', 2, b'ACCGT')]), msg)
