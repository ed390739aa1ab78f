"""CPU tests of bam2illumina: the NumPy statement of the histogram rule (tests/model_util.py) against the reference's
golden models, the model's finishing step bit for bit, the written files, and the command line."""
import pickle

import numpy as np
import pytest

from tests import model_util as MU

SETS = ['defaults', 'every3', 'bq50']


@pytest.mark.parametrize('name', SETS)
def test_numpy_rule_equals_the_reference(name):
  g = MU.golden()
  s = g['sets'][name]
  idx = MU.subset(g, s)
  assert len(idx) == s['n_records']
  bq, tl, c = MU.np_model([g['tuples'][i] for i in idx], len(g['sq']), **s['params'])
  assert np.array_equal(bq, MU.dense_bq(s)) and np.array_equal(tl, MU.dense_tlen(s))
  assert c['used'] == s['r_cnt'] and c['min_rlen'] == s['min_rlen'] and c['max_rlen'] == s['max_rlen']
  assert c['seen'] == len(idx) == sum(c[k] for k in ('used', 'skipped_unplaced', 'skipped_ref', 'skipped_every',
                                                      'skipped_flag'))
  # the fixture reaches every branch of the rule
  assert c['skipped_unplaced'] and c['skipped_ref'] and c['skipped_flag'] and tl.sum() > 0 and bq[0].any() and bq[1].any()
  assert (c['skipped_every'] > 0) == (s['params'].get('every', 1) > 1)
  assert c['max_rlen'] == s['params'].get('max_bp', 300)


def test_fixture_covers_the_edges():
  g = MU.golden()
  t = g['tuples']
  assert len(g['sq']) == 26
  lens = {len(x[4]) for x in t}
  assert set(range(1, 151)) <= lens and {160, 300} <= lens
  flags = [x[0] for x in t]
  for bit in (0x10, 0x100, 0x200, 0x400, 0x800, 0x4):
    assert any(f & bit for f in flags), hex(bit)
  assert any(f & 0xc0 == 0 for f in flags) and any(f & 0xc0 == 0xc0 for f in flags)
  assert {0, 10, 60, 255} <= {x[2] for x in t}
  assert {999, -999, 1000, -1000, 499, -499, 500, -500, MU.INT32_MIN} <= {x[3] for x in t}
  assert {-1, 24, 25} <= {x[1] for x in t}
  # INT32_MIN as a template length: |T| is taken in 64 bits and is no bin
  bq, tl, c = MU.np_model([(0x83, 0, 60, MU.INT32_MIN, [30] * 5)], 1)
  assert tl.sum() == 0 and c['used'] == 1


def test_numpy_rule_raises_where_the_reference_does():
  ok = (0x43, 0, 60, 0, [30] * 10)
  for bad in [(0x43, 0, 60, 0, [30] * 11), (0x43, 0, 60, 0, [30] * 9 + [40]), (0x43, 0, 60, 0, [255] * 10),
              (0x43, 0, 60, 0, []), (0x43, 3, 60, 0, [30] * 10)]:
    with pytest.raises(MU.ModelError) as e:
      MU.np_model([ok, ok, bad, ok], 3, max_bp=10, max_bq=40)
    assert e.value.index == 2
    # removed by `every` (its contig's second record) or by its flag: never looked at (a tid past the header still is)
    if bad[1] < 3:
      MU.np_model([ok, bad, ok], 3, every=2, max_bp=10, max_bq=40)
      MU.np_model([ok, (0x143,) + bad[1:], ok], 3, max_bp=10, max_bq=40)


@pytest.mark.parametrize('name', SETS)
def test_model_from_counts_bit_for_bit(name):
  from mitty_amd.empirical import bam2illumina as b2i
  s = MU.golden()['sets'][name]
  m = b2i.model_from_counts(MU.dense_bq(s), MU.dense_tlen(s), s['r_cnt'], s['min_rlen'], s['max_rlen'],
                            s['model_description'], s['min_mq'])
  MU.check_model(m, s, name)
  assert m['model_description'] == s['model_description']


def test_model_from_counts_empty():
  from mitty_amd.empirical import bam2illumina as b2i
  s = MU.golden()['empty']
  with np.errstate(all='raise'):   # quiet too
    m = b2i.model_from_counts(np.zeros((2, 300, 94), np.uint64), np.zeros(1000, np.uint64), 0, None, 0,
                              s['model_description'], 0)
  MU.check_model(m, s, 'empty')
  assert m['r_cnt'] == 0 and m['min_rlen'] == 1e13 and m['max_rlen'] == 0 and np.isnan(m['cum_tlen']).all()
  assert not m['cum_bq_mat'].any()


def _golden_model(name='defaults'):
  from mitty_amd.empirical import bam2illumina as b2i
  s = MU.golden()['sets'][name]
  return s, b2i.model_from_counts(MU.dense_bq(s), MU.dense_tlen(s), s['r_cnt'], s['min_rlen'], s['max_rlen'],
                                  s['model_description'], s['min_mq'])


def test_written_pkl_is_a_read_model(tmp_path):
  from mitty_amd import readmodel
  s, m = _golden_model()
  path = str(tmp_path / 'm.pkl')
  with open(path, 'wb') as fp:
    pickle.dump(m, fp)
  back = readmodel.load_model_file(path)   # (the parser that never unpickles)
  MU.check_model(back, s, 'pkl')
  mod, model = readmodel.get_read_model(path)
  assert mod is not None
  p = mod.read_model_params(model, 30.0)
  assert p['rlen'] == s['mean_rlen'] and len(p['cum_tlen']) == 1000


def test_npz_round_trip(tmp_path):
  from mitty_amd import readmodel
  s, m = _golden_model('every3')
  path = str(tmp_path / 'm.npz')
  readmodel.save_model_npz(m, path)
  back = readmodel.load_model_file(path)
  MU.check_model(back, s, 'npz')
  assert back['model_description'] == s['model_description']


def test_cli_lists_the_command():
  from click.testing import CliRunner
  from mitty_amd import cli
  out = CliRunner().invoke(cli.cli, ['--help'])
  assert out.exit_code == 0 and 'bam2illumina' in out.output
  out = CliRunner().invoke(cli.cli, ['bam2illumina', '--help'])
  assert out.exit_code == 0
  for opt in ('--every', '--min-mq', '--threads', '--max-bp', '--max-tlen', '--device'):
    assert opt in out.output, opt
  assert 'bam2illumina' not in cli.__doc__.split('Out of scope')[1]
