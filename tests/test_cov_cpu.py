"""CPU tests of gc-cov and bq: the NumPy statement of both rules (tests/cov_util.py) against the reference's golden
results, gc-cov's finishing step bit for bit, the output dicts, the error cases, and the command line."""
import numpy as np
import pytest

from tests import cov_util as CU

SETS = ['bl100', 'bl37', 'bl1000']


@pytest.fixture(scope='module')
def g():
  return CU.golden()


def _gc_cov(g, block_len, records=None):
  from mitty_amd.empirical import gc
  cov, c = CU.np_cov(g['tuples'] if records is None else records, g['lengths'], block_len, g['seqs'])
  d = {'block_len': block_len, 'seq_info': g['sq']}
  for i, s in enumerate(g['sq'][:CU.N_VISITED]):
    d[s['SN']] = gc.gc_cov_from_counts(s['LN'], block_len, **{k: cov[i][k] for k in (
      'n_n', 'n_gc', 'covered', 'span_sum', 'min_pos', 'max_end')})
  return d, cov, c


@pytest.mark.parametrize('name', SETS)
def test_numpy_rule_and_finishing_step_equal_the_reference(g, name):
  s = g['sets'][name]
  d, cov, c = _gc_cov(g, s['block_len'])
  CU.check_gc_cov(d, s, g, name)
  assert c['seen'] == len(g['tuples']) == sum(v for k, v in c.items() if k != 'seen')
  assert all(c[k] > 0 for k in c), c   # the fixture reaches every class
  # ... and both sides of the N rule at its edge: a block of exactly 10 % N is kept, one above is NaN
  n = np.concatenate([cov[i]['n'] for i in cov])
  n_n = np.concatenate([cov[i]['n_n'] for i in cov])
  gc_all = np.concatenate([d[q['SN']]['gc'] for q in g['sq'][:CU.N_VISITED]])
  edge = 10 * n_n == n
  assert edge.any() and not np.isnan(gc_all[edge]).any()
  assert np.array_equal(np.isnan(gc_all), 10 * n_n > n) and np.isnan(gc_all).any()


def test_empty_file(g):
  s = g['empty']['gc_cov']
  d, _, c = _gc_cov(g, s['block_len'], records=[])
  CU.check_gc_cov(d, s, g, 'empty')
  assert c['seen'] == 0
  cov = np.concatenate([d[q['SN']]['coverage'] for q in g['sq'][:CU.N_VISITED]])
  assert not np.nan_to_num(cov).any()
  mats, c = CU.np_bq([], len(g['sq']))
  CU.check_bq(dict(mats_by_name(g, mats), seq_info=g['sq']), g['empty']['bq'], g, 'empty bq')


def mats_by_name(g, mats):
  return {g['sq'][i]['SN']: m for i, m in mats.items()}


def test_bq_rule_equals_the_reference(g):
  mats, c = CU.np_bq(g['tuples'], len(g['sq']))
  CU.check_bq(dict(mats_by_name(g, mats), seq_info=g['sq']), g['bq'], g, 'bq')
  assert c['seen'] == len(g['tuples']) == sum(v for k, v in c.items() if k != 'seen')
  assert all(c[k] > 0 for k in c), c
  assert sum(int(m.sum()) for m in mats.values()) == sum(
    len(t[4]) for t in g['tuples'] if 0 <= t[1] < CU.N_VISITED and t[0] <= 255)


def test_fixture_covers_the_edges(g):
  t = g['tuples']
  ln = g['lengths']
  assert len(ln) == 26 and {1, 2, 3} <= set(ln) and sum(x > 2 * 2048 for x in ln[:24]) >= 3
  for bl in (100, 37, 1000):
    assert any(x > 2 and (x - 1) % bl == 0 for x in ln[:24]), bl
  for bit in (0x4, 0x10, 0x100, 0x200, 0x400, 0x800):
    assert any(x[0] & bit for x in t), hex(bit)
  ops = set(''.join(x[3] for x in t))
  assert set('MIDNSH=XP') <= ops and any(x[3] == '' for x in t)
  assert {-1, 24, 25} <= {x[1] for x in t}
  assert any(0 <= x[1] < 24 and x[2] + CU.ref_span(x[3]) > ln[x[1]] for x in t)          # ends past LN
  assert any(CU.ref_span(x[3]) == 1 and x[2] % 100 == 0 and x[2] > 0 for x in t)          # a shared base alone
  assert any(CU.ref_span(x[3]) > 3 * 100 for x in t)                                      # three blocks and more
  assert max(len(x[4]) for x in t) == 500 and max(max(x[4]) for x in t) == 99
  seq = b''.join(g['seqs'])
  assert all(ch in seq for ch in b'Ngcn') and any(ch in seq for ch in b'RYSWKM')


def test_block_layout():
  # range(1, LN, bl): no block below two bases, the last block clipped, neighbours share one base
  for ln, bl, want in ((1, 5, []), (2, 5, [(0, 2)]), (6, 5, [(0, 6)]), (7, 5, [(0, 6), (5, 7)]),
                       (11, 5, [(0, 6), (5, 11)]), (12, 5, [(0, 6), (5, 11), (10, 12)]), (3, 1, [(0, 2), (1, 3)])):
    cov, _ = CU.np_cov([], [ln], bl)
    assert list(zip(cov[0]['a'].tolist(), cov[0]['b'].tolist())) == want, (ln, bl)
    assert CU.n_blocks(ln, bl) == len(want)


def test_closed_form_equals_a_column_walk():
  """U and S of np_cov against the walk the pileup does: every column of every overlapping record."""
  rng = np.random.RandomState(3)
  for _ in range(60):
    ln, bl = int(rng.randint(2, 90)), int(rng.randint(1, 25))
    recs = []
    for _ in range(int(rng.randint(0, 12))):
      pos = int(rng.randint(ln))
      recs.append((0, 0, pos, '{}M'.format(int(rng.randint(1, 40))), [30]))
    cov, _ = CU.np_cov(recs, [ln], bl)
    for k, (a, b) in enumerate(zip(cov[0]['a'], cov[0]['b'])):
      cols = {}
      for _, _, pos, cig, _ in recs:
        end = pos + CU.ref_span(cig)
        if pos < b and end > a:
          for x in range(pos, end):
            cols[x] = cols.get(x, 0) + 1
      o = cov[0]
      u = o['covered'][k] + max(0, a - o['min_pos'][k]) + max(0, o['max_end'][k] - b)
      assert (o['span_sum'][k], u) == (sum(cols.values()), len(cols)), (ln, bl, k, recs)


def test_errors_name_the_record():
  ok = (0, 0, 5, '10M', [30] * 10)
  for bad in [(0, 0, 50, '10M', [30] * 10), (0, 0, -1, '10M', [30] * 10), (0, 3, 5, '10M', [30] * 10)]:
    with pytest.raises(CU.CovError) as e:
      CU.np_cov([ok, ok, bad, ok], [50, 60, 70], 7)
    assert e.value.index == 2
    if bad[1] < 3:   # removed by its flag, or without a span, the record's position is never looked at
      CU.np_cov([ok, (0x400,) + bad[1:], (0, 0, bad[2], '4S', [30] * 4)], [50, 60, 70], 7)
  CU.np_cov([(0, 0, 49, '10M', [30] * 10)], [50], 7)   # an end past LN is fine
  for bad in [(0, 0, 5, '', []), (0, 0, 5, '501M', [30] * 501), (0, 0, 5, '3M', [30, 100, 30]),
              (0, 0, 5, '3M', [255] * 3), (0, 3, 5, '3M', [30] * 3)]:
    with pytest.raises(CU.CovError) as e:
      CU.np_bq([ok, ok, bad, ok], 3)
    assert e.value.index == 2
    if bad[1] < 3:
      CU.np_bq([ok, (0x100,) + bad[1:], ok], 3)


def test_fasta_contigs_must_be_the_headers(g, tmp_path):
  """A contig that is missing from the FASTA, or whose length is not LN, is an error that names it (pysam would
  clip): checked before a device is touched."""
  from mitty_amd.empirical import gc
  from tests import score_util as SU
  bam = str(tmp_path / 'g.bam')
  with open(bam, 'wb') as fp:
    fp.write(SU.bgzf_bytes(SU.bam_bytes(g['recs'][:50], g['sq'], CU.header_text(g))))
  text = CU.fasta_text(g)
  cut = text.index(b'>c3\n')
  cases = {'missing': (text[:cut] + text[text.index(b'>c4\n'):], 'c3', None),
           'short': (text.replace(b'>c3\n', b'>c3\nACGT\n>c3rest\n'), 'c3', ('4', '750')),
           'beyond the visited 24': (text[:text.index(b'>c25\n')], None, None)}
  for what, (fa_bytes, name, nums) in cases.items():
    fa = str(tmp_path / 'f.fa')
    with open(fa, 'wb') as fp:
      fp.write(fa_bytes)
    seqs = gc._native.read_fasta(fa, [s['SN'] for s in g['sq'][:24]])
    if name is None:
      gc.check_fasta(g['sq'], seqs)   # contigs 25 and 26 are never fetched
      continue
    for call in (lambda: gc.check_fasta(g['sq'], seqs), lambda: gc.process_bam_parallel(bam, fa, str(tmp_path / 'p'))):
      with pytest.raises(ValueError) as e:
        call()
      assert 'contig ' + name in str(e.value), (what, str(e.value))
      assert nums is None or all(x in str(e.value) for x in nums), (what, str(e.value))
    assert not (tmp_path / 'p').exists()


def test_seq_info():
  from mitty_amd.benchmarking.god_aligner import seq_info
  g = CU.golden()
  assert seq_info(CU.header_text(g)) == g['sq']
  got = seq_info('@HD\tVN:1.4\n@SQ\tSN:a\tLN:7\tUR:file:/x:y\tM5:00ff\n@RG\tID:r\n@SQ\tSN:b\tLN:9\n')
  assert got == [{'SN': 'a', 'LN': 7, 'UR': 'file:/x:y', 'M5': '00ff'}, {'SN': 'b', 'LN': 9}]
  assert list(got[0]) == ['SN', 'LN', 'UR', 'M5'] and type(got[0]['LN']) is int
  assert seq_info('@HD\tVN:1.4\n', ['a', 'b'], [3, 4]) == [{'SN': 'a', 'LN': 3}, {'SN': 'b', 'LN': 4}]


def test_cli_lists_the_commands():
  from click.testing import CliRunner
  from mitty_amd import cli
  out = CliRunner().invoke(cli.cli, ['--help'])
  assert out.exit_code == 0 and 'gc-cov' in out.output and 'bq' in out.output
  out = CliRunner().invoke(cli.cli, ['gc-cov', '--help'])
  assert out.exit_code == 0
  for opt in ('-b', '--block-len', '-t', '--threads', '--device', 'BAM FASTA PKL'):
    assert opt in out.output, opt
  out = CliRunner().invoke(cli.cli, ['bq', '--help'])
  assert out.exit_code == 0
  for opt in ('-t', '--threads', '--device', 'BAM PKL'):
    assert opt in out.output, opt
  scope = cli.__doc__.split('Out of scope')[1]
  assert 'gc-cov' not in scope and 'bq' not in scope
