"""GPU tests of the alignment scorers (mq-plot / derr-plot): the device pass (mh_score.hip) against the reference's
golden matrices, edge shapes, contention, the god-aligner store path and the error returns.  Every comparison is
exact integer equality."""
import numpy as np
import pytest

from tests import golden_io as G
from tests import score_util as SU

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
def golden_bam(tmp_path_factory):
  """The golden aligned reads as a BAM file; 3000-byte BGZF blocks, so records straddle them."""
  g = SU.golden()
  path = str(tmp_path_factory.mktemp('score') / 'golden.bam')
  with open(path, 'wb') as fp:
    fp.write(SU.bgzf_bytes(SU.bam_bytes(g['recs'], g['sq']), block=3000))
  return path


def _same(got, want, what):
  assert got.dtype == np.uint64 and got.shape == want.shape, what
  if not np.array_equal(got, want):
    bad = np.argwhere(got != want)
    raise AssertionError('{}: {} cells differ, first {} got {} want {}'.format(
      what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize('strict', [0, 1])
@pytest.mark.parametrize('max_d', [200, 5])
def test_golden_bam_matrices(native, golden_bam, tmp_path, strict, max_d):
  from mitty_amd.benchmarking import derr, mq
  g = SU.golden()
  k = 's{}_d{}'.format(strict, max_d)
  csv = str(tmp_path / 'mq.csv')
  got = mq.process_bam(golden_bam, max_d=max_d, strict=bool(strict), processes=3, out_csv=csv)
  want = SU.dense(g['mq'][k], (100, 2 * max_d + 1))
  _same(got, want, 'mq_mat ' + k)
  assert np.array_equal(np.loadtxt(csv, delimiter=',', dtype=np.uint64), want)
  assert int(want.sum()) == sum(1 for r in g['records'] if r[2] is not None)
  for mv in (200, 10):
    got = derr.process_bam(golden_bam, max_v_len=mv, max_d=max_d, strict=bool(strict), processes=2)
    _same(got, SU.dense(g['derr']['{}_v{}'.format(k, mv)], (2 * max(mv, 51) + 2, 2 * max_d + 1)),
          'd_err_mat {} v{}'.format(k, mv))


def test_golden_bam_sample_filter_and_counts(native, golden_bam):
  from mitty_amd.benchmarking import derr, mq, score
  g = SU.golden()
  s = g['sample']
  _same(mq.process_bam(golden_bam, sample_name=s['name']), SU.dense(s['mq'], (100, 401)), 'mq_mat sample')
  _same(derr.process_bam(golden_bam, sample_name=s['name']), SU.dense(s['derr'], (402, 401)), 'd_err_mat sample')
  # many small chunks through the two staging buffers: the same sums, and the counts add up
  m, d, cnt = score.score_bam(golden_bam, sample_name=s['name'], processes=4, chunk_bytes=20000)
  _same(m, SU.dense(s['mq'], (100, 401)), 'mq_mat sample, chunked')
  _same(d, SU.dense(s['derr'], (402, 401)), 'd_err_mat sample, chunked')
  placed = [r for r in g['records'] if r[2] is not None]
  assert cnt == {'seen': len(g['records']), 'scored': sum(1 for r in placed if r[0].startswith(s['name'])),
                 'skipped_unplaced': len(g['records']) - len(placed),
                 'skipped_sample': sum(1 for r in placed if not r[0].startswith(s['name']))}
  assert cnt['skipped_sample'] > 0 and cnt['skipped_unplaced'] > 0


def _score(ctx, names, recs, chunk=None, **kw):
  """recs (a list of record bytes) through score_add_records, `chunk` records per call (None: one call)."""
  ctx.score_begin(names, **kw)
  step = chunk or max(len(recs), 1)
  for o in range(0, len(recs), step):
    part = recs[o:o + step]
    ctx.score_add_records(b''.join(part), SU.offsets(part))
  return ctx.score_result()


def test_shapes(ctx):
  g = SU.golden()
  names = [s['SN'] for s in g['sq']]
  # zero records, then one record
  mq, dv, cnt = _score(ctx, names, [])
  assert not mq.any() and not dv.any() and cnt['seen'] == 0
  for n in (1, 257, 700):   # one record; a count that is no multiple of the workgroup's 256
    want = SU.py_matrices(g['records'][:n])
    mq, dv, cnt = _score(ctx, names, g['recs'][:n])
    _same(mq, want[0], 'mq_mat n={}'.format(n))
    _same(dv, want[1], 'd_err_mat n={}'.format(n))
    assert cnt['seen'] == n
  # every scoring call sees a single record
  mq, dv, _ = _score(ctx, names, g['recs'][:300], chunk=1)
  want = SU.py_matrices(g['records'][:300])
  _same(mq, want[0], 'mq_mat, single-record calls')
  _same(dv, want[1], 'd_err_mat, single-record calls')


def test_qname_longer_than_the_lds_row(ctx):
  # 192-byte rows hold 36 fixed bytes and the name: a 254-character qname is read from memory instead
  vl = ','.join(['7', '-12', '0', '300', '-300'] * 12)
  q = 'S1:0:0:1|2|1|0|5000|150|50=7I93=|' + vl + '|1|5200|150|150=|'
  q += ',' * (254 - len(q))   # (empty items: read 2 carries no variant)
  assert len(q) == 254
  recs, aligned = [], []
  for i, (flag, pos, mapq) in enumerate([(0x43, 4999, 60), (0x83, 5199, 17), (0x43, 5049, 3), (0x43, 4990, 99)] * 40):
    recs.append(SU.record(q, flag, 1, pos, mapq))
    aligned.append((q, flag, '2', pos, mapq))
    short = 'S1:0:0:{}|2|1|0|5000|150|150=||1|5200|150|150=|'.format(i)   # rows of both kinds in one workgroup
    recs.append(SU.record(short, 0x43, 1, 4999 + i % 3, 60))
    aligned.append((short, 0x43, '2', 4999 + i % 3, 60))
  for mv in (200, 400):
    want = SU.py_matrices(aligned, max_v_len=mv)
    mq, dv, _ = _score(ctx, ['1', '2', '3'], recs, max_v_len=mv)
    _same(mq, want[0], 'mq_mat')
    _same(dv, want[1], 'd_err_mat v{}'.format(mv))
  assert want[1][400 + 300].sum() == 12 * 120 and want[1][400 - 300].sum() == 12 * 120


def test_contention(ctx):
  n = 100000
  q = 'S1:0:0:1|1|0|0|1000|100|100=|'
  hit = SU.record(q, 0, 0, 999, 60)
  blob, roff = hit * n, np.arange(n + 1, dtype=np.int64) * len(hit)
  runs = []
  for _ in range(2):   # every record in one cell of each matrix
    ctx.score_begin(['1'], max_d=200, max_v_len=200)
    ctx.score_add_records(blob, roff)
    runs.append(ctx.score_result())
  mq, dv, cnt = runs[0]
  assert mq[60, 200] == n and mq.sum() == n and dv[401, 200] == n and dv.sum() == n and cnt['scored'] == n
  assert all(np.array_equal(a, b) for a, b in zip(runs[0][:2], runs[1][:2]))
  # both extremes +-max_d (strict: clamped), SNP row, interleaved
  q2 = 'S1:0:0:1|1|0|0|1000|100|50=1X49=|0'
  lo, hi = SU.record(q2, 0, 0, 999 - 205, 60), SU.record(q2, 0, 0, 999 + 205, 60)
  assert len(lo) == len(hi)
  blob, roff = (lo + hi) * (n // 2), np.arange(n + 1, dtype=np.int64) * len(lo)
  runs = []
  for _ in range(2):
    ctx.score_begin(['1'], max_d=200, max_v_len=200, strict=True)
    ctx.score_add_records(blob, roff)
    runs.append(ctx.score_result())
  mq, dv, cnt = runs[0]
  assert mq[60, 0] == n // 2 and mq[60, 400] == n // 2 and mq.sum() == n
  assert dv[200, 0] == n // 2 and dv[200, 400] == n // 2 and dv.sum() == n
  assert all(np.array_equal(a, b) for a, b in zip(runs[0][:2], runs[1][:2]))


def _god_fastqs(model):
  """The golden FASTQ pair without the templates the BAM builder refuses (a read cut short by a deletion that runs
  past the region end keeps rlen qualities: sequence and quality lengths differ)."""
  l1 = G.fastq_bytes('e2e_{}.r1.fq.gz'.format(model)).split(b'\n')
  l2 = G.fastq_bytes('e2e_{}.r2.fq.gz'.format(model)).split(b'\n')
  keep = [i for i in range(0, len(l1) - 1, 4)
          if len(l1[i + 1]) == len(l1[i + 3]) and len(l2[i + 1]) == len(l2[i + 3])]
  return (b''.join(b'\n'.join(l1[i:i + 4]) + b'\n' for i in keep),
          b''.join(b'\n'.join(l2[i:i + 4]) + b'\n' for i in keep))


def _template_truth(fq1, paired):
  """(qname, flag, chrom, pos, 60) of the god-aligner's records for file 1's qnames."""
  from mitty_amd.simulation import readgenerate as rg
  out = []
  for line in fq1.split(b'\n')[0::4]:
    if not line:
      continue
    q = line[1:].split()[0].decode()
    for mate, ri in enumerate(rg.parse_qname(q)[:2 if paired else 1]):
      flag = (0x10 if ri.strand else 0) | ((0x3 | (0x40 if mate == 0 else 0x80)) if paired else 0)
      out.append((q, flag, ri.chrom, ri.pos - 1, 60))
  return out


@pytest.mark.parametrize('strict', [True, False])
def test_store_path_equals_file_path(native, ctx, tmp_path, strict):
  g = SU.golden()
  names, lens = [s['SN'] for s in g['sq']], [s['LN'] for s in g['sq']]
  b1, b2 = _god_fastqs('hiseq-X-v2.5-Garvan')
  ctx.bam_set_refs(names, lens)
  ctx.bam_add_fastq(b1, b2)
  ctx.score_begin([], max_d=200, max_v_len=200, strict=strict)   # (the store's own names are used)
  ctx.score_add_store()
  mq, dv, cnt = ctx.score_result()
  n = 2 * (b1.count(b'\n') // 4)
  truth = _template_truth(b1, True)
  inside = sum(1 for q, flag, _, _, _ in truth if '>' in q.split('|')[11 if flag & 0x80 else 6])
  assert cnt == {'seen': n, 'scored': n, 'skipped_unplaced': 0, 'skipped_sample': 0} and inside > 0
  assert mq.sum() == n and mq[60].sum() == n
  if strict:
    assert mq[60, 200] == n
  else:   # reads from inside a long insertion score max_d wherever they are
    assert mq[60, 200] == n - inside and mq[60, 400] == inside
  want = SU.py_matrices(truth, strict=strict)
  _same(mq, want[0], 'mq_mat of the store')
  _same(dv, want[1], 'd_err_mat of the store')
  # the BAM the same store writes, scored from the file
  from mitty_amd.benchmarking import score
  bam = str(tmp_path / 's.bam')
  ctx.bam_write(bam, '@HD\tVN:1.4\tSO:coordinate\n', level=1, threads=2)
  m2, d2, c2 = score.score_bam(bam, strict=strict, processes=2)
  _same(m2, mq, 'mq_mat file vs store')
  _same(d2, dv, 'd_err_mat file vs store')
  assert c2 == cnt


def test_store_written_in_sorted_order_from_the_arenas(native):
  """mh_bam_add_output writes the store straight into coordinate order; the sums are the same."""
  from mitty_amd.engine import Engine
  from mitty_amd.lib import fasta as mfasta, vcfio
  from mitty_amd.readmodel import get_read_model
  from mitty_amd.simulation import readgenerate
  # the 2x250 golden run: none of its reads is cut short by a deletion past the region end, which the BAM builder
  # refuses (sequence and quality lengths differ)
  c = G.load_json('e2e_config.json')['1kg-pcr-free']
  mod, mdl = get_read_model('1kg-pcr-free.pkl')
  rm = mod.read_model_params(mdl, c['coverage'])
  vdf = vcfio.load_variants_soa(G.path(c['vcf']), c['sample'], G.path(c['bed']))
  seqs = mfasta.read_fasta(G.path(c['fasta']))
  units = [(ps, w['region_idx'], w['region_cpy'], w['rng_seed'])
           for ps, w in enumerate(readgenerate.get_data_for_workers(rm, vdf, c['seed']))]
  eng = Engine(0)
  try:
    for ri, reg in enumerate(vdf):
      eng.load_region(ri, reg['region'], mfasta.fetch(seqs, *reg['region']))
    eng.run_units(units, lambda r, cp: vdf[r]['copies'][cp], rm['p'], rm['rlen'], rm['cum_tlen'], c['sample'])
    d1, _ = eng.ctx.fetch_output()
    eng.ctx.bam_set_refs(['1', '2', '3'], [50000, 20000, 8000])
    t = eng.ctx.bam_add_output()
    eng.ctx.score_begin([], strict=False)
    eng.ctx.score_add_store()
    mq, dv, cnt = eng.ctx.score_result()
  finally:
    eng.close()
  truth = _template_truth(bytes(d1), True)
  assert t > 100 and cnt['scored'] == 2 * t == len(truth)
  want = SU.py_matrices(truth)
  _same(mq, want[0], 'mq_mat')
  _same(dv, want[1], 'd_err_mat')


def test_errors_store_nothing_and_leave_the_context_usable(ctx):
  g = SU.golden()
  names = [s['SN'] for s in g['sq']]
  good = g['recs'][:100]
  want = SU.py_matrices(g['records'][:100])
  bad = {
    'parse': SU.record('S1:0:0:1|1|0|x|1000|100|100=|', 0, 0, 999, 60),          # strand is not a number
    'fields': SU.record('no-bars-at-all', 0, 0, 999, 60),
    'read2': SU.record('S1:0:0:1|1|0|0|1000|100|100=|', 0x83, 0, 999, 60),       # read2, one group
    'mapq': SU.record('S1:0:0:1|1|0|0|1000|100|100=|', 0, 0, 999, 100),
    'tid': SU.record('S1:0:0:1|1|0|0|1000|100|100=|', 0, 7, 999, 60),            # past the header's names
  }
  for what, rec in bad.items():
    ctx.score_begin(names)
    ctx.score_add_records(b''.join(good), SU.offsets(good))
    recs = good[:50] + [rec] + good[50:]
    ctx.score_add_records(b''.join(recs), SU.offsets(recs))
    ctx.score_add_records(b''.join(good), SU.offsets(good))      # after the failure: not added either
    with pytest.raises(ValueError) as e:
      ctx.score_result()
    assert 'record 150' in str(e.value), (what, str(e.value))     # 100 good ones, then the 51st of the second call
    ctx.score_reset()
    mq, dv, cnt = ctx.score_result()
    assert not mq.any() and not dv.any() and cnt['seen'] == 0, what
    ctx.score_add_records(b''.join(good), SU.offsets(good))
    mq, dv, cnt = ctx.score_result()
    _same(mq, want[0], 'mq_mat after ' + what)
    _same(dv, want[1], 'd_err_mat after ' + what)
  # a structurally broken record never reaches the device: refused by the host check of the same call
  broken = bytearray(good[0])
  broken[12] = 0
  ctx.score_begin(names)
  with pytest.raises(ValueError):
    ctx.score_add_records(bytes(broken), SU.offsets([bytes(broken)]))
  mq, dv, cnt = ctx.score_result()
  assert cnt['seen'] == 0
