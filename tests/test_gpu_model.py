"""GPU tests of bam2illumina: the device histogram pass (mh_model.hip) against the reference's golden models, edge
shapes, contention, the god-aligner store path, the error returns, and the model in use.  Every comparison of counts
is exact integer equality."""
import numpy as np
import pytest

from tests import golden_io as G
from tests import model_util as MU
from tests import score_util as SU

pytestmark = pytest.mark.gpu

SETS = ['defaults', 'every3', 'bq50']


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
def golden_bams(tmp_path_factory):
  """Per parameter set, its golden records as a BAM file; 3000-byte BGZF blocks, so records straddle them."""
  g = MU.golden()
  d = tmp_path_factory.mktemp('model')
  out = {}
  for name in SETS:
    out[name] = str(d / (name + '.bam'))
    with open(out[name], 'wb') as fp:
      fp.write(SU.bgzf_bytes(SU.bam_bytes([g['recs'][i] for i in MU.subset(g, g['sets'][name])], g['sq']), block=3000))
  return out


def _same(got, want, what):
  assert got.dtype == np.uint64 and got.shape == want.shape, what
  if not np.array_equal(got, want):
    bad = np.argwhere(got != want)
    raise AssertionError('{}: {} cells differ, first {} got {} want {}'.format(
      what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _same_result(got, want, what):
  _same(got[0], want[0], what + ': bq_mat')
  _same(got[1], want[1], what + ': tlen')
  assert got[2] == want[2], what


@pytest.mark.parametrize('name', SETS)
def test_golden_bam_models(native, golden_bams, tmp_path, name):
  from mitty_amd import readmodel
  from mitty_amd.empirical import bam2illumina as b2i
  g = MU.golden()
  s = g['sets'][name]
  pkl = str(tmp_path / 'm.pkl')
  m = b2i.process_bam_parallel(golden_bams[name], pkl, model_description=s['model_description'], threads=3,
                               **s['params'])
  MU.check_model(m, s, name)
  assert m['model_description'] == s['model_description']
  MU.check_model(readmodel.load_model_file(pkl), s, name + ' (.pkl)')
  # many small chunks: the ordinal of `every` is carried across chunk boundaries inside a contig
  want = MU.np_model([g['tuples'][i] for i in MU.subset(g, s)], len(g['sq']), **s['params'])
  _same_result(b2i.count_bam(golden_bams[name], threads=2, chunk_bytes=20000, **s['params']), want, name + ' chunked')
  _same_result(b2i.count_bam(golden_bams[name], threads=2, **s['params']), want, name)
  npz = str(tmp_path / 'm.npz')
  b2i.process_bam_parallel(golden_bams[name], npz, model_description=s['model_description'], chunk_bytes=20000,
                           **s['params'])
  MU.check_model(readmodel.load_model_file(npz), s, name + ' (.npz)')


def _run(ctx, n_refs, recs, chunk=None, **kw):
  """recs (a list of record bytes) through model_add_records, `chunk` records per call (None: one call)."""
  ctx.model_begin(n_refs, **kw)
  step = chunk or max(len(recs), 1)
  for o in range(0, len(recs), step):
    part = recs[o:o + step]
    ctx.model_add_records(b''.join(part), MU.offsets(part))
  return ctx.model_result()


def test_shapes(ctx):
  g = MU.golden()
  got = _run(ctx, 26, [])
  assert not got[0].any() and not got[1].any()
  assert got[2] == dict(seen=0, used=0, skipped_unplaced=0, skipped_ref=0, skipped_every=0, skipped_flag=0,
                        min_rlen=None, max_rlen=0)
  for n in (1, 257, 700):   # one record; counts that are no multiple of the 64-record batch or the 256-record tile
    for kw in ({}, {'every': 3, 'min_mq': 20}):
      _same_result(_run(ctx, 26, g['recs'][:n], **kw), MU.np_model(g['tuples'][:n], 26, **kw), 'n={} {}'.format(n, kw))
  # every call sees a single record: the ordinals live in the session
  for kw in ({}, {'every': 2}):
    _same_result(_run(ctx, 26, g['recs'][:300], chunk=1, **kw), MU.np_model(g['tuples'][:300], 26, **kw),
                 'single-record calls {}'.format(kw))


def test_record_layouts(ctx):
  # the qualities' place in the record: l_seq 1, odd, and max_bp; no CIGAR and five operations; a short and a
  # 254-character name (far from the head, at every alignment)
  rng = np.random.RandomState(5)
  tuples, recs = [], []
  for i in range(240):
    L = [1, 2, 3, 63, 64, 65, 129, 255, 300][i % 9]
    t = ([0x43, 0x93, 0x53, 0x83][i % 4], i % 3, 60, int(rng.randint(-1200, 1200)), rng.randint(0, 94, L).tolist())
    tuples.append(t)
    recs.append(MU.record(*t, qname='q' * [1, 2, 3, 4, 254, 17][i % 6], n_cigar=[1, 0, 5][i % 3]))
  for kw in ({}, {'max_tlen': 5000}):   # (5000 bins: the template lengths take the path without LDS counters)
    _same_result(_run(ctx, 3, recs, **kw), MU.np_model(tuples, 3, **kw), 'layouts {}'.format(kw))
  want = MU.np_model(tuples, 3)
  assert want[2]['min_rlen'] == 1 and want[2]['max_rlen'] == 300 and want[0][:, 299].sum() > 0


def test_shape_beyond_lds(ctx):
  # 600 x 256 counters per mate: five slabs of base positions per mate; 255 is an ordinary quality here
  rng = np.random.RandomState(6)
  tuples = [([0x43, 0x93, 0x53, 0x83][i % 4], 0, 60, 300, rng.randint(0, 256, 500 if i % 5 else 600).tolist())
            for i in range(150)]
  tuples.append((0x83, 0, 60, 300, [255] * 7))
  recs = [MU.record(*t) for t in tuples]
  kw = {'max_bp': 600, 'max_bq': 256}
  _same_result(_run(ctx, 1, recs, **kw), MU.np_model(tuples, 1, **kw), 'max_bp 600, max_bq 256')
  _same_result(_run(ctx, 1, recs, chunk=40, **kw), MU.np_model(tuples, 1, **kw), 'max_bp 600, max_bq 256, chunks')


def test_unsorted_refs_with_every(ctx):
  rng = np.random.RandomState(7)
  tuples = [(0x43 if i & 1 else 0x83, int(rng.choice([0, 1, 2, 23, 24, -1, 7])), 60, 200,
             rng.randint(0, 94, int(rng.randint(1, 80))).tolist()) for i in range(1500)]
  recs = [MU.record(*t) for t in tuples]
  for every in (2, 7):
    for chunk in (None, 333):
      _same_result(_run(ctx, 30, recs, chunk=chunk, every=every), MU.np_model(tuples, 30, every=every),
                   'every {} chunk {}'.format(every, chunk))
  # flags do not enter the ordinal: the same records, some of them secondary
  tuples = [((t[0] | 0x100) if i % 3 == 0 else t[0],) + t[1:] for i, t in enumerate(tuples)]
  recs = [MU.record(*t) for t in tuples]
  _same_result(_run(ctx, 30, recs, every=2), MU.np_model(tuples, 30, every=2), 'every 2 with secondaries')


def test_contention(ctx):
  n = 100000
  q = [(7 * i) % 41 + 2 for i in range(150)]
  a = MU.record(0x93, 0, 60, -350, q)
  b = MU.record(0x93, 0, 60, 350, [41 - (v % 7) for v in q])
  assert len(a) == len(b)
  for blob, qs in ((a * n, [q]), ((a + b) * (n // 2), [q, [41 - (v % 7) for v in q]])):
    roff = np.arange(n + 1, dtype=np.int64) * len(a)
    runs = []
    for _ in range(2):   # every cell of the records is hot, and one template length
      ctx.model_begin(1)
      ctx.model_add_records(blob, roff)
      runs.append(ctx.model_result())
    bq, tl, cnt = runs[0]
    want = np.zeros((2, 300, 94), np.uint64)
    for qq in qs:   # reverse strand: stored back to front
      want[1, np.arange(150), qq[::-1]] += np.uint64(n // len(qs))
    _same(bq, want, 'bq_mat of {} distinct records'.format(len(qs)))
    if len(qs) == 1:
      assert all(bq[1, i, q[149 - i]] == n for i in range(150))
    assert bq.sum() == n * 150 and not bq[0].any() and bq[1].sum(axis=1)[:150].tolist() == [n] * 150
    assert tl[350] == n and tl.sum() == n
    assert cnt == dict(seen=n, used=n, skipped_unplaced=0, skipped_ref=0, skipped_every=0, skipped_flag=0,
                       min_rlen=150, max_rlen=150)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[1][2] == cnt


def _corrupted_pair(model):
  """The golden corrupted FASTQ pair without the templates the BAM builder refuses (sequence and quality lengths
  differ: a read cut short by a deletion that runs past the region end)."""
  l1 = G.fastq_bytes('corrupt_{}.r1.fq.gz'.format(model)).split(b'\n')
  l2 = G.fastq_bytes('corrupt_{}.r2.fq.gz'.format(model)).split(b'\n')
  keep = [i for i in range(0, len(l1) - 1, 4)
          if len(l1[i + 1]) == len(l1[i + 3]) and len(l2[i + 1]) == len(l2[i + 3])]
  return [l1[i:i + 4] for i in keep], [l2[i:i + 4] for i in keep]


def _fastq_hist(files, max_bp=300, max_bq=94):
  bq = np.zeros((2, max_bp, max_bq), np.uint64)
  for m, recs in enumerate(files):
    for r in recs:
      q = np.frombuffer(r[3], np.uint8).astype(np.int64) - 33
      bq[m, np.arange(len(q)), q] += np.uint64(1)
  return bq


@pytest.mark.parametrize('model', G.MODELS)
def test_store_path(native, tmp_path, model):
  from mitty_amd.empirical import bam2illumina as b2i
  f1, f2 = _corrupted_pair(model)
  sq = G.load_json('god_header.json')
  c = native.Context(0)
  try:
    c.bam_set_refs([s['SN'] for s in sq], [s['LN'] for s in sq])
    c.bam_add_fastq(b''.join(b'\n'.join(r) + b'\n' for r in f1), b''.join(b'\n'.join(r) + b'\n' for r in f2))
    c.model_begin(0)   # (the store's own reference count is used)
    c.model_add_store()
    bq, tl, cnt = c.model_result()
    bam = str(tmp_path / 's.bam')
    c.bam_write(bam, '@HD\tVN:1.4\tSO:coordinate\n', level=1, threads=2)
  finally:
    c.close()
  n = len(f1)
  assert n > 100
  # the god-aligner stores strand-1 qualities reversed; the model reverses them back: the FASTQ's own strings
  _same(bq, _fastq_hist((f1, f2)), 'bq_mat of the store')
  lens = [len(r[3]) for r in f1 + f2]
  assert cnt == dict(seen=2 * n, used=2 * n, skipped_unplaced=0, skipped_ref=0, skipped_every=0, skipped_flag=0,
                     min_rlen=min(lens), max_rlen=max(lens))
  assert tl[0] == n and tl.sum() == n   # the god-aligner leaves TLEN 0
  _same_result(b2i.count_bam(bam, threads=2), (bq, tl, cnt), 'file vs store')


def test_errors_store_nothing_and_leave_the_context_usable(ctx):
  g = MU.golden()
  good = g['recs'][:100]
  want = MU.np_model(g['tuples'][:100], 26)
  want3 = MU.np_model(g['tuples'][:100] * 3, 26)
  bad = {
    'long': (0x43, 0, 60, 0, [30] * 301),
    'quality': (0x43, 0, 60, 0, [30] * 10 + [94]),
    'no qualities': (0x43, 0, 60, 0, [255] * 20),
    'empty': (0x43, 0, 60, 0, []),
    'tid': (0x43, 26, 60, 0, [30] * 10),
  }
  for what, t in bad.items():
    rec = MU.record(*t)
    recs = good[:50] + [rec] + good[50:]
    ctx.model_begin(26)
    ctx.model_add_records(b''.join(good), MU.offsets(good))
    ctx.model_add_records(b''.join(recs), MU.offsets(recs))
    ctx.model_add_records(b''.join(good), MU.offsets(good))      # after the failure: not added either
    with pytest.raises(ValueError) as e:
      ctx.model_result()
    assert 'record 150' in str(e.value), (what, str(e.value))     # 100 good ones, then the 51st of the second call
    ctx.model_reset()
    got = ctx.model_result()
    assert not got[0].any() and not got[1].any() and got[2]['seen'] == 0 and got[2]['min_rlen'] is None, what
    for _ in range(3):
      ctx.model_add_records(b''.join(good), MU.offsets(good))
    _same_result(ctx.model_result(), want3, 'after ' + what)
    if what == 'tid':
      continue
    # removed by `every` (ordinal 150 of its contig, every 4) or by its flag, the record is never looked at
    same_ref = [MU.record(f, 0, mq, tl, q) for f, _, mq, tl, q in g['tuples'][:200]]
    tup = [(f, 0, mq, tl, q) for f, _, mq, tl, q in g['tuples'][:200]]
    got = _run(ctx, 26, same_ref[:150] + [rec] + same_ref[150:], every=4)
    _same_result(got, MU.np_model(tup[:150] + [t] + tup[150:], 26, every=4), what + ' behind every')
    t2 = (t[0] | 0x100,) + t[1:]
    got = _run(ctx, 26, good[:50] + [MU.record(*t2)] + good[50:])
    assert got[2]['skipped_flag'] == want[2]['skipped_flag'] + 1 and got[2]['used'] == want[2]['used'], what
    _same(got[0], want[0], what + ' behind flag 0x100')
  # a structurally broken record never reaches the device: refused by the host check of the same call
  broken = bytearray(good[0])
  broken[12] = 0
  ctx.model_begin(26)
  with pytest.raises(ValueError):
    ctx.model_add_records(bytes(broken), MU.offsets([bytes(broken)]))
  assert ctx.model_result()[2]['seen'] == 0
  # arguments
  for kw in ({'every': 0}, {'max_bq': 0}, {'max_bq': 257}, {'max_bp': 0}, {'max_tlen': 0},
             {'max_bp': 1 << 23, 'max_bq': 256}):
    with pytest.raises(ValueError):
      ctx.model_begin(26, **kw)


def test_the_model_is_usable(native, tmp_path):
  """corrupt-reads with a model built here emits only qualities the model saw at that position of that file."""
  from click.testing import CliRunner
  from mitty_amd import readmodel
  from mitty_amd.cli import cli
  from mitty_amd.readmodel import get_read_model
  from mitty_amd.simulation import readcorrupt
  model = 'hiseq-X-v2.5-Garvan'
  f1, f2 = _corrupted_pair(model)
  sq = G.load_json('god_header.json')
  bam, pkl = str(tmp_path / 'g.bam'), str(tmp_path / 'fresh.pkl')
  c = native.Context(0)
  try:
    c.bam_set_refs([s['SN'] for s in sq], [s['LN'] for s in sq])
    c.bam_add_fastq(b''.join(b'\n'.join(r) + b'\n' for r in f1), b''.join(b'\n'.join(r) + b'\n' for r in f2))
    c.bam_write(bam, '@HD\tVN:1.4\tSO:coordinate\n', level=1, threads=2)
  finally:
    c.close()
  res = CliRunner().invoke(cli, ['bam2illumina', bam, pkl, 'fresh', '-t', '2', '--every', '0'])   # (every: max(1, .))
  assert res.exit_code == 0, res.output + repr(res.exception)
  m = readmodel.load_model_file(pkl)
  assert m['model_description'] == 'fresh' and m['bq_mat'].shape == (2, 300, 94) and m['tlen'].shape == (1000,)
  mod, mdl = get_read_model(pkl)
  assert mod is not None and mdl['r_cnt'] == 2 * len(f1) and mod.read_model_params(mdl, 10.0)['rlen'] == m['max_rlen']
  o1, o2 = str(tmp_path / 'c1.fq'), str(tmp_path / 'c2.fq')
  readcorrupt.multi_process(mod, mdl, G.path('e2e_{}.r1.fq.gz'.format(model)), o1,
                            G.path('e2e_{}.r2.fq.gz'.format(model)), o2, seed=11, rng='philox')
  for f, path in enumerate((o1, o2)):
    recs = G.parse_fastq(open(path, 'rb').read())
    assert len(recs) > 100
    for _, _, quals in recs:
      q = np.frombuffer(quals.encode(), np.uint8).astype(np.int64) - 33
      assert (m['bq_mat'][f, np.arange(len(q)), q] > 0).all()
