"""GPU tests of gc-cov and bq: the device passes (mh_cov.hip, mh_model.hip with a table per contig) against the
reference's golden results, edge shapes, contention, results and resets, the GC counts, the error returns, the
god-aligner store path and the command line.  Counts are compared by exact integer equality, floats bit for bit."""
import pickle
import struct

import numpy as np
import pytest

from oracle import god as OG
from tests import cov_util as CU
from tests import golden_io as G
from tests import score_util as SU

pytestmark = pytest.mark.gpu

SETS = ['bl100', 'bl37', 'bl1000']
COV_KEYS = ('covered', 'span_sum', 'min_pos', 'max_end')


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
def golden_files(tmp_path_factory):
  """The golden records as a BAM file (3000-byte BGZF blocks, so records straddle them), the same without records,
  and the golden FASTA."""
  g = CU.golden()
  d = tmp_path_factory.mktemp('cov')
  out = {'bam': str(d / 'g.bam'), 'empty': str(d / 'e.bam'), 'fasta': str(d / 'g.fa')}
  for key, recs in (('bam', g['recs']), ('empty', [])):
    with open(out[key], 'wb') as fp:
      fp.write(SU.bgzf_bytes(SU.bam_bytes(recs, g['sq'], CU.header_text(g)), block=3000))
  with open(out['fasta'], 'wb') as fp:
    fp.write(CU.fasta_text(g))
  return out


def _same(got, want, what):
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, what
  if not np.array_equal(got.astype(np.int64), want.astype(np.int64)):
    bad = np.argwhere(got.astype(np.int64) != want.astype(np.int64))
    raise AssertionError('{}: {} cells differ, first {} got {} want {}'.format(
      what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _same_cov(ctx, want, what, keys=COV_KEYS):
  """Every visited contig's arrays and the counts of the context's session against np_cov's."""
  cov, cnt = want
  for i in cov:
    got, c = ctx.cov_result(i)
    for k in keys:
      _same(got[k], cov[i][k], '{}: contig {} {}'.format(what, i, k))
    assert c == cnt, (what, c, cnt)


def _run(ctx, lengths, bl, tuples, chunk=None, seqs=None):
  """tuples through a fresh session, `chunk` records per call (None: one call)."""
  ctx.cov_begin(lengths, bl)
  if seqs is not None:
    for i, s in enumerate(seqs[:CU.N_VISITED]):
      ctx.upload_contig(0, s)
      ctx.cov_gc(i, 0)
  recs = [CU.record(*t) for t in tuples]
  step = chunk or max(len(recs), 1)
  for o in range(0, len(recs), step):
    ctx.cov_add_records(b''.join(recs[o:o + step]), CU.offsets(recs[o:o + step]))


@pytest.mark.parametrize('name', SETS)
def test_golden_gc_cov(native, golden_files, tmp_path, name):
  from mitty_amd.empirical import gc
  g = CU.golden()
  s = g['sets'][name]
  for kw in ({}, {'chunk_bytes': 20000}):   # many chunks, contigs changing inside a chunk
    pkl = str(tmp_path / 'g.pkl')
    d = gc.process_bam_parallel(golden_files['bam'], golden_files['fasta'], pkl, block_len=s['block_len'], threads=3,
                                **kw)
    CU.check_gc_cov(d, s, g, '{} {}'.format(name, kw))
    with open(pkl, 'rb') as fp:
      CU.check_gc_cov(pickle.load(fp), s, g, '{} {} (.pkl)'.format(name, kw))
  _, counts = gc.count_bam(golden_files['bam'], golden_files['fasta'], s['block_len'], chunk_bytes=20000)
  assert counts == CU.np_cov(g['tuples'], g['lengths'], s['block_len'])[1]


def test_golden_bq_and_empty_files(native, golden_files, tmp_path):
  from mitty_amd.empirical import bq, gc
  g = CU.golden()
  for kw in ({}, {'chunk_bytes': 20000}):
    pkl = str(tmp_path / 'b.pkl')
    d = bq.process_bam_parallel(golden_files['bam'], pkl, threads=3, **kw)
    CU.check_bq(d, g['bq'], g, 'bq {}'.format(kw))
    with open(pkl, 'rb') as fp:
      CU.check_bq(pickle.load(fp), g['bq'], g, 'bq {} (.pkl)'.format(kw))
  _, counts = bq.count_bam(golden_files['bam'], chunk_bytes=20000)
  want = CU.np_bq(g['tuples'], len(g['sq']))[1]
  assert {k: counts[k] for k in want} == want and counts['skipped_every'] == 0
  assert counts['min_rlen'] == 1 and counts['max_rlen'] == 500
  e = g['empty']
  CU.check_gc_cov(gc.process_bam_parallel(golden_files['empty'], golden_files['fasta'], str(tmp_path / 'e.pkl'),
                                          block_len=e['gc_cov']['block_len']), e['gc_cov'], g, 'empty')
  CU.check_bq(bq.process_bam_parallel(golden_files['empty'], str(tmp_path / 'eb.pkl')), e['bq'], g, 'empty bq')


def _random_tuples(rng, lengths, n):
  """Records over the contigs (26 of them: also contigs 25, 26 and unplaced), ends past LN, spans of 1 to 3000."""
  out = []
  for _ in range(n):
    tid = int(rng.randint(-1, len(lengths))) if len(lengths) > 1 else 0
    ln = lengths[max(tid, 0)]
    span = int(rng.choice([1, 1, 2, 5, 60, 150, 3000]))
    cigar = ['{}M'.format(span), '{}M{}N1M'.format(1, span), '2S{}={}D1X'.format(1, span), '3S'][int(rng.randint(4))]
    flag = int(rng.choice([0, 0x10, 0x800, 0x400, 0x4, 0x100, 0x200], p=[.4, .3, .1, .05, .05, .05, .05]))
    out.append((flag, tid, -1 if tid < 0 else int(rng.randint(ln)), cigar, [30, 31]))
  return out


def test_shapes(ctx):
  rng = np.random.RandomState(11)
  keys = COV_KEYS + ('n_n', 'n_gc')
  for ln in (1, 2, 3, 2047, 2048, 2049, 4097):   # around the scan's tile of 2048 cells (a contig owns LN + 1)
    seq = bytes(rng.choice(list(b'ACGTNgc'), size=ln).astype(np.uint8))
    for bl in (1, 2, 2048, 5000):
      t = _random_tuples(rng, [ln], 40)
      _run(ctx, [ln], bl, t, seqs=[seq])
      _same_cov(ctx, CU.np_cov(t, [ln], bl, [seq]), 'LN {} block_len {}'.format(ln, bl), keys)
  for n_refs in (24, 26):
    lengths = [int(x) for x in rng.choice([1, 2, 3, 100, 2047, 2048, 2049, 4097], size=n_refs)]
    seqs = [bytes(rng.choice(list(b'ACGTNgc'), size=x).astype(np.uint8)) for x in lengths]
    t = _random_tuples(rng, lengths, 1500)
    for bl, chunk in ((64, None), (5, 333)):
      _run(ctx, lengths, bl, t, chunk=chunk, seqs=seqs)
      want = CU.np_cov(t, lengths, bl, seqs)
      assert len(want[0]) == 24 and all(want[1][k] for k in want[1] if n_refs > 24 or k != 'skipped_ref')
      _same_cov(ctx, want, '{} contigs block_len {}'.format(n_refs, bl), keys)
  # an empty session
  _run(ctx, [100, 50], 10, [])
  _same_cov(ctx, CU.np_cov([], [100, 50], 10), 'empty')
  got, c = ctx.cov_result(0)
  assert not got['covered'].any() and not got['span_sum'].any() and not got['max_end'].any()
  assert (got['min_pos'] == CU.NO_POS).all() and c['seen'] == 0


def test_contention(ctx):
  n, ln, bl = 20000, 30000, 100
  same = CU.record(0, 0, 1234, '150M', [30])
  for what, blob, pos in (('identical', same * n, [1234] * n),
                          ('staggered', b''.join(CU.record(0, 0, 100 + i, '150M', [30]) for i in range(n)),
                           [100 + i for i in range(n)])):
    ctx.cov_begin([ln], bl)
    ctx.cov_add_records(blob, np.arange(n + 1, dtype=np.int64) * len(same))
    got, c = ctx.cov_result(0)
    a = np.arange(CU.n_blocks(ln, bl), dtype=np.int64) * bl
    b = np.minimum(a + bl + 1, ln)
    p = np.asarray(pos, dtype=np.int64)
    hit = (p[None, :] < b[:, None]) & (p[None, :] + 150 > a[:, None])   # [block, record]
    _same(got['span_sum'], 150 * hit.sum(axis=1), what + ' span_sum')
    _same(got['min_pos'], np.where(hit, p[None, :], CU.NO_POS).min(axis=1), what + ' min_pos')
    _same(got['max_end'], np.where(hit, p[None, :] + 150, 0).max(axis=1), what + ' max_end')
    depth = np.zeros(ln + 1, np.int64)
    np.add.at(depth, p, 1)
    np.add.at(depth, p + 150, -1)
    cum = np.concatenate([[0], np.cumsum(np.cumsum(depth)[:ln] > 0)])
    _same(got['covered'], cum[b] - cum[a], what + ' covered')
    assert c == dict(seen=n, used=n, skipped_unplaced=0, skipped_ref=0, skipped_flag=0, skipped_nospan=0)
  # one record over 1210 blocks of one base (a long N operation), beside short ones
  t = [(0, 0, 10, '5M1200N5M', [30] * 10), (0, 0, 3, '2M', [30] * 2), (0x10, 0, 700, '1M', [30])] * 3
  _run(ctx, [4097], 1, t)
  want = CU.np_cov(t, [4097], 1)
  assert (want[0][0]['span_sum'] >= 3 * 1210).sum() >= 1000
  _same_cov(ctx, want, 'a record over 1210 blocks')


def test_results_and_resets(ctx):
  rng = np.random.RandomState(12)
  lengths = [5000, 300]
  t = _random_tuples(rng, lengths, 600)
  _run(ctx, lengths, 37, t[:300])
  _same_cov(ctx, CU.np_cov(t[:300], lengths, 37), 'first half')
  recs = [CU.record(*x) for x in t[300:]]
  ctx.cov_add_records(b''.join(recs), CU.offsets(recs))      # after a result: shows up in the next one
  _same_cov(ctx, CU.np_cov(t, lengths, 37), 'both halves')
  ctx.cov_reset()
  _same_cov(ctx, CU.np_cov([], lengths, 37), 'after reset')
  ctx.cov_add_records(b''.join(recs), CU.offsets(recs))
  _same_cov(ctx, CU.np_cov(t[300:], lengths, 37), 'second half alone')
  # bq: the same
  recs_all = [CU.record(*x) for x in t]
  ctx.bq_begin(2)
  ctx.bq_add_records(b''.join(recs_all[:300]), CU.offsets(recs_all[:300]))
  mats, cnt = CU.np_bq(t[:300], 2)
  for i in mats:
    _same(ctx.bq_result(i)[0], mats[i], 'bq first half')
  ctx.bq_add_records(b''.join(recs_all[300:]), CU.offsets(recs_all[300:]))
  mats, cnt = CU.np_bq(t, 2)
  for i in mats:
    m, c = ctx.bq_result(i)
    _same(m, mats[i], 'bq both halves')
    assert {k: c[k] for k in cnt} == cnt
  ctx.bq_reset()
  assert not ctx.bq_result(0)[0].any() and ctx.bq_result(1)[1]['seen'] == 0


def test_gc_counts(ctx):
  # upper case only, N apart from n, IUPAC bytes are neither; the base at (k + 1) bl belongs to blocks k and k + 1
  rng = np.random.RandomState(13)
  seq = bytearray(rng.choice(list(b'ACGTacgtNnRYSWKM'), size=300).astype(np.uint8))
  seq[7], seq[14], seq[64], seq[128] = b'GNCN'
  seq[210:231] = b'N' * 21
  seq = bytes(seq)
  for bl in (7, 64):
    ctx.cov_begin([300], bl)
    ctx.upload_contig(3, seq)
    ctx.cov_gc(0, 3)
    got, _ = ctx.cov_result(0)
    want = CU.np_cov([], [300], bl, [seq])[0][0]
    _same(got['n_n'], want['n_n'], 'n_n block_len {}'.format(bl))
    _same(got['n_gc'], want['n_gc'], 'n_gc block_len {}'.format(bl))
    k = 0   # the shared base counts on both sides
    assert got['n_gc'][k] == sum(ch in b'GC' for ch in seq[0:bl + 1])
    assert got['n_gc'][k + 1] == sum(ch in b'GC' for ch in seq[bl:2 * bl + 1])
  assert sum(ch in b'gcn' for ch in seq) > 20
  ctx.upload_contig(3, seq[:299])
  with pytest.raises(ValueError) as e:   # a contig of another length than the header's
    ctx.cov_gc(0, 3)
  assert '299' in str(e.value) and '300' in str(e.value)
  with pytest.raises(ValueError):       # not one of the session's contigs
    ctx.cov_gc(1, 3)
  ctx.release_contig(3)
  with pytest.raises(ValueError):       # released
    ctx.cov_gc(0, 3)
  ctx.release_contig(3)                 # (an id that is not there: nothing to do)


def test_errors_store_nothing_and_leave_the_context_usable(ctx):
  rng = np.random.RandomState(14)
  lengths = [400, 300, 200]
  tup = [x for x in _random_tuples(rng, lengths, 200) if x[1] >= 0][:100]
  assert len(tup) == 100
  good = [CU.record(*x) for x in tup]
  blob, off = b''.join(good), CU.offsets(good)
  want1, want3 = CU.np_cov(tup, lengths, 16), CU.np_cov(tup * 3, lengths, 16)
  bad = {'pos': CU.record(0, 1, 300, '10M', [30] * 10), 'tid': CU.record(0, 3, 5, '10M', [30] * 10)}
  for what, rec in bad.items():
    recs = good[:50] + [rec] + good[50:]
    ctx.cov_begin(lengths, 16)
    ctx.cov_add_records(blob, off)
    ctx.cov_add_records(b''.join(recs), CU.offsets(recs))
    ctx.cov_add_records(blob, off)                      # after the failure: not added either
    with pytest.raises(ValueError) as e:
      ctx.cov_result(0)
    assert 'record 150' in str(e.value), (what, str(e.value))   # 100 good ones, then the 51st of the second call
    for i in want1[0]:   # the first call's sums are intact; nothing of the failing call or of the one after it
      got, c, msg = ctx.cov_result(i, failed_ok=True)
      assert 'record 150' in msg and c == want1[1], (what, msg, c)
      for k in COV_KEYS:
        _same(got[k], want1[0][i][k], '{} before the failing call: contig {} {}'.format(what, i, k))
    ctx.cov_reset()
    _same_cov(ctx, CU.np_cov([], lengths, 16), 'reset after ' + what)
    for _ in range(3):
      ctx.cov_add_records(blob, off)
    _same_cov(ctx, want3, 'after ' + what)
  # removed by its flag, or without a span, a record's position is never looked at
  odd = [(0x400, 1, 300, '10M', [30] * 10), (0, 1, 300, '10S', [30] * 10)]
  _run(ctx, lengths, 16, tup[:50] + odd + tup[50:])
  _same_cov(ctx, CU.np_cov(tup[:50] + odd + tup[50:], lengths, 16), 'skipped records')
  # a CIGAR cut short by the record's end never reaches the device: refused by the host check of the same call, and
  # the earlier chunk's sums are intact
  broken = bytearray(good[0])
  struct.pack_into('<H', broken, 16, 4000)
  ctx.cov_begin(lengths, 16)
  ctx.cov_add_records(blob, off)
  with pytest.raises(ValueError) as e:
    ctx.cov_add_records(bytes(broken), CU.offsets([bytes(broken)]))
  assert 'record 100' in str(e.value), str(e.value)   # the session's 101st
  _same_cov(ctx, want1, 'after a refused chunk')
  ctx.cov_add_records(blob, off)                       # usable: the next chunk is the session's second
  _same_cov(ctx, CU.np_cov(tup * 2, lengths, 16), 'a chunk after the refused one')
  # bq: a quality of 100, a read of 501 bases
  mats1, cnt1 = CU.np_bq(tup, 3)
  for what, rec in (('quality', CU.record(0, 0, 5, '3M', [30, 100, 30])), ('long', CU.record(0, 0, 5, '501M', [30] * 501))):
    recs = good[:50] + [rec] + good[50:]
    ctx.bq_begin(3)
    ctx.bq_add_records(blob, off)
    ctx.bq_add_records(b''.join(recs), CU.offsets(recs))
    ctx.bq_add_records(blob, off)
    with pytest.raises(ValueError) as e:
      ctx.bq_result(0)
    assert 'record 150' in str(e.value), (what, str(e.value))
    ctx.bq_reset()
    assert not ctx.bq_result(0)[0].any() and ctx.bq_result(0)[1]['seen'] == 0
    ctx.bq_add_records(blob, off)
    for i in mats1:
      m, c = ctx.bq_result(i)
      _same(m, mats1[i], 'bq after ' + what)
      assert {k: c[k] for k in cnt1} == cnt1
  ok500 = CU.record(0x10, 2, 5, '500M', list(range(100)) * 5)   # exactly 500 bases, qualities up to 99
  ctx.bq_begin(3)
  ctx.bq_add_records(ok500, CU.offsets([ok500]))
  m = ctx.bq_result(2)[0]
  assert m.sum() == 500 and m[0, 99] == 1 and m[499, 0] == 1
  # arguments
  for ln, bl in (([100], 0), ([100], -5), ([-1], 10), ([1 << 31], 10)):
    with pytest.raises(ValueError):
      ctx.cov_begin(ln, bl)


def _import_records(c, recs):
  """Records into the context's store as a packed piece (mh_bam_import): no host check looks at them."""
  blob = b''.join(recs)
  o_roff, o_key, o_info, total = c_layout(len(recs), len(blob))
  piece = np.zeros(total, np.uint8)
  piece[:len(blob)] = np.frombuffer(blob, np.uint8)
  piece[o_roff:o_key] = CU.offsets(recs).view(np.uint8)
  c.bam_import(len(recs), len(blob), piece.ctypes.data)


def c_layout(n, nbytes):
  from mitty_amd import _native
  return _native.bam_piece_layout(n, nbytes)


def test_device_bounds_of_the_record_walk(native):
  """k_cov_head's own checks (36 bytes of fixed fields; 36 + l_read_name + 4 n_cigar <= the record's size), reached
  through the record store, which mh_bam_import fills without the host reader's checks: a CIGAR that ends exactly at
  the record's end is read, one entry more is refused, with nothing stored, the right index, the earlier chunk's sums
  intact and the context usable."""
  rng = np.random.RandomState(15)
  lengths = [400, 300, 200]
  tup = [x for x in _random_tuples(rng, lengths, 200) if x[1] >= 0][:100]
  good = [CU.record(*x) for x in tup]
  want1 = CU.np_cov(tup, lengths, 16)
  # no bases: the record ends with its CIGAR's last entry (36 + 2 + 4 * 2 = its size)
  edge_t = (0, 1, 7, '5M3D', [])
  edge = CU.record(*edge_t)
  assert len(edge) == 36 + 2 + 8 and struct.unpack_from('<H', edge, 16)[0] == 2
  over = bytearray(edge)
  struct.pack_into('<H', over, 16, 3)                    # a third entry would start at the record's end
  short = struct.pack('<i', 16) + bytes(16)              # 20 bytes: no room for the fixed fields
  c = native.Context(0)
  try:
    c.bam_set_refs(['a', 'b', 'c'], lengths)
    # the exact fit is a record like any other
    _import_records(c, good[:50] + [edge] + good[50:])
    c.cov_begin(lengths, 16)
    c.cov_add_store()
    _same_cov(c, CU.np_cov(tup[:50] + [edge_t] + tup[50:], lengths, 16), 'a CIGAR that ends at the record\'s end')
    for what, bad in (('a CIGAR cut by the record\'s end', bytes(over)), ('a record of 20 bytes', short)):
      c.bam_reset()
      c.bam_set_refs(['a', 'b', 'c'], lengths)
      _import_records(c, good[:50] + [bad] + good[50:])
      c.cov_begin(lengths, 16)
      c.cov_add_records(b''.join(good), CU.offsets(good))
      c.cov_add_store()
      c.cov_add_records(b''.join(good), CU.offsets(good))   # after the failure: not added either
      with pytest.raises(ValueError) as e:
        c.cov_result(0)
      assert 'record 150' in str(e.value) and 'fit' in str(e.value), (what, str(e.value))
      for i in want1[0]:
        got, cnt, msg = c.cov_result(i, failed_ok=True)
        assert 'record 150' in msg and cnt == want1[1], (what, msg, cnt)
        for k in COV_KEYS:
          _same(got[k], want1[0][i][k], '{}: contig {} {}'.format(what, i, k))
      c.cov_reset()
      c.cov_add_records(b''.join(good), CU.offsets(good))
      _same_cov(c, want1, 'after ' + what)
  finally:
    c.close()


def test_store_path(native):
  """The golden syn genome's reads god-aligned into the store: the sessions over the store equal the NumPy rules
  over the oracle's records."""
  from mitty_amd.empirical import bq, gc
  from mitty_amd.lib import fasta as mfasta
  model = G.MODELS[0]
  l1, l2 = (G.fastq_bytes('e2e_{}.r{}.fq.gz'.format(model, k)).split(b'\n') for k in (1, 2))
  keep = [i for i in range(0, len(l1) - 1, 4)   # (without the templates the BAM builder refuses: a read cut short)
          if len(l1[i + 1]) == len(l1[i + 3]) and len(l2[i + 1]) == len(l2[i + 3])]
  f1, f2 = (b''.join(b'\n'.join(l[i:i + 4]) + b'\n' for i in keep) for l in (l1, l2))
  sq = G.load_json('god_header.json')
  lengths = [s['LN'] for s in sq]
  seqs = mfasta.read_fasta_py(G.path('data/syn.fa'))
  orc = OG.god_records(f1, f2, {s['SN']: i for i, s in enumerate(sq)})
  tup = [(OG.flag(r), r['reference_id'], r['pos'], r['cigarstring'], [ord(ch) - 33 for ch in r['qual']]) for r in orc]
  assert len(tup) > 1000
  bl = 500
  c = native.Context(0)
  try:
    c.bam_set_refs([s['SN'] for s in sq], lengths)
    c.bam_add_fastq(f1, f2)
    # the context's owner has contigs of its own (an Engine's region ri is contig ri): they are left alone, and
    # what from_store uploaded is gone again
    own = b'GGCCN' * 20
    c.upload_contig(0, own)
    d, counts = gc.from_store(c, sq, seqs, block_len=bl)
    b, bcounts = bq.from_store(c, sq)
    c.cov_begin([len(own)], 10)
    c.cov_gc(0, 0)
    assert c.cov_result(0)[0]['n_gc'].tolist() == CU.np_cov([], [len(own)], 10, [own])[0][0]['n_gc'].tolist()
    with pytest.raises(ValueError):
      c.cov_gc(0, gc.SCRATCH_CONTIG_ID)
  finally:
    c.close()
  cov, cnt = CU.np_cov(tup, lengths, bl, [seqs[s['SN']] for s in sq])
  assert counts == cnt and cnt['used'] + cnt['skipped_nospan'] == len(tup)   # (reads inside an insertion: no span)
  lo, hi = np.inf, -np.inf
  for i, s in enumerate(sq):
    want = gc.gc_cov_from_counts(s['LN'], bl, **{k: cov[i][k] for k in ('n_n', 'n_gc') + COV_KEYS})
    CU.same_floats(d[s['SN']]['gc'], want['gc'], 'store gc ' + s['SN'])
    CU.same_floats(d[s['SN']]['coverage'], want['coverage'], 'store coverage ' + s['SN'])
    ok = ~np.isnan(want['coverage'])
    lo, hi = min(lo, want['coverage'][ok].min()), max(hi, want['coverage'][ok].max())
  got = np.concatenate([d[s['SN']]['coverage'] for s in sq])
  got = got[~np.isnan(got)]
  assert len(got) > 50 and got.min() == lo and got.max() == hi and hi > 0   # the range the rule gives, no other bound
  mats, bcnt = CU.np_bq(tup, len(sq))
  for i, s in enumerate(sq):
    _same(b[s['SN']], mats[i], 'store bq ' + s['SN'])
  assert {k: bcounts[k] for k in bcnt} == bcnt


def test_cli(native, golden_files, tmp_path):
  from click.testing import CliRunner
  from mitty_amd.cli import cli
  g = CU.golden()
  pkl = str(tmp_path / 'c.pkl')
  res = CliRunner().invoke(cli, ['gc-cov', golden_files['bam'], golden_files['fasta'], pkl, '-b', '37', '-t', '2'])
  assert res.exit_code == 0, res.output + repr(res.exception)
  with open(pkl, 'rb') as fp:
    CU.check_gc_cov(pickle.load(fp), g['sets']['bl37'], g, 'cli gc-cov')
  res = CliRunner().invoke(cli, ['bq', golden_files['bam'], pkl, '--threads', '2'])
  assert res.exit_code == 0, res.output + repr(res.exception)
  with open(pkl, 'rb') as fp:
    CU.check_bq(pickle.load(fp), g['bq'], g, 'cli bq')
