"""GC-bias curves and the thinning rule's NumPy restatement, on the host (no GPU): the restatement on hand-computed
cases, the thresholds, the curve file's refusals, the fit to a synthetic gc-cov result and the two CLI entry points."""
import json
import pickle

import numpy as np
import pytest

from mitty_amd.simulation import gcbias
from tests import gcbias_ref as R
from tests import golden_io as G

FULL = np.full(101, 1 << 32, np.uint64)


def _bins_of(hap, spans, rlen=1, p_min=1):
  """Bins of the spans [(first byte, last byte + 1)] of hap: pos0 = first, pos1 + rlen = end, in sample coordinates."""
  pos0 = np.array([p_min + a for a, _ in spans], np.int64)
  pos1 = np.array([p_min + b - rlen for _, b in spans], np.int64)
  return R.bins(hap, p_min, pos0, pos1, rlen)


def test_restatement_bins_by_hand():
  assert _bins_of(b'G' + b'A' * 99, [(0, 100)]).tolist() == [1]          # 100 * 1 // 100
  assert _bins_of(b'GC' * 50, [(0, 100)]).tolist() == [100]
  assert _bins_of(b'gcN', [(0, 3)]).tolist() == [0]                      # lower case and N count in L only
  assert _bins_of(b'gcNG', [(0, 4), (3, 4)]).tolist() == [25, 100]
  assert _bins_of(b'GGGG', [(2, 2)], rlen=0).tolist() == [0]             # L == 0
  # the clamps: a span starting before p_min, one reaching past the end, one wholly outside (L == 0 again)
  hap = b'GGAAAAAAAC'
  assert R.bins(hap, 100, [95], [100], 2).tolist() == [100]              # bytes [0, 2): 'GG'
  assert R.bins(hap, 100, [108], [120], 5).tolist() == [50]              # bytes [8, 10): 'AC'
  assert R.bins(hap, 100, [300], [320], 5).tolist() == [0]
  assert R.bins(hap, 100, [50], [60], 5).tolist() == [0]                 # end clamped up to start


def test_restatement_extremes():
  hap, n = b'ACGT' * 64, 4096
  pos0 = np.arange(n, dtype=np.int64) % 200 + 1
  fo0 = np.zeros(n, np.int8)
  idx, b, seen, kept = R.thin(hap, 1, fo0, pos0, pos0 + 20, 10, np.zeros(101, np.uint64), 7, 9)
  assert len(idx) == 0 and kept.sum() == 0 and seen.sum() == n
  idx, b, seen, kept = R.thin(hap, 1, fo0, pos0, pos0 + 20, 10, FULL, 7, 9)
  assert np.array_equal(idx, np.arange(n)) and np.array_equal(seen, kept)
  # T = 2^32 keeps the largest draw there is, T = 2^32 - 1 does not
  top = np.uint64(0xffffffff)
  assert top < FULL[0] and not top < np.uint64((1 << 32) - 1)
  # the draw is word 0 of the Philox block of the template's 64-bit index, whatever the array it sits in
  u = R.draws(n, 7, 9)
  assert np.array_equal(R.draws(100, 7, 9, t0=1000), u[1000:1100])
  assert u.max() <= 0xffffffff and len(np.unique(u)) > n - 8
  assert R.keys((5 << 32) | 7, (3 << 32) | 9) == (7, 9, (5 ^ 3 ^ 0x67636269))
  hi = R.draws(2, 7, 9, t0=(1 << 32) - 1)   # the index's high word is counter word 1
  assert hi[0] == u_at(7, 9, (1 << 32) - 1, 0) and hi[1] == u_at(7, 9, 0, 1)


def u_at(seed, unit_key, lo, hi):
  from tests.philox_ref import philox4x32_10
  k0, k1, c3 = R.keys(seed, unit_key)
  return philox4x32_10([lo], [hi], [0], [c3], k0, k1)[0][0]


def test_thresholds():
  w = np.zeros(101)
  w[1], w[2], w[3] = 1.0, 0.5, 2.0 ** -33
  t = gcbias.thresholds(w)
  assert t.dtype == np.uint64 and t.shape == (101,)
  assert t[:4].tolist() == [0, 1 << 32, 1 << 31, 0]
  w[3] = 2.0 ** -32
  assert gcbias.thresholds(w)[3] == 1
  w[3] = 1.0 - 2.0 ** -40
  assert gcbias.thresholds(w)[3] == (1 << 32) - 1


def _write(tmp_path, d):
  p = str(tmp_path / 'curve.json')
  with open(p, 'w') as fp:
    json.dump(d, fp)
  return p


@pytest.mark.parametrize('what,weight,cls', [
  ('101', [0.5] * 100, 'gc-bias'),
  ('not finite', [0.5] * 50 + [float('nan')] + [0.5] * 50, 'gc-bias'),
  ('outside', [0.5] * 50 + [1.5] + [0.5] * 50, 'gc-bias'),
  ('zero', [0.0] * 101, 'gc-bias'),
  ('model_class', [0.5] * 101, 'illumina'),
])
def test_load_curve_refusals(tmp_path, what, weight, cls):
  p = _write(tmp_path, {'model_class': cls, 'description': 'x', 'weight': weight})
  with pytest.raises(ValueError, match=what):
    gcbias.load_curve(p)


def test_load_curve_other_refusals_and_round_trip(tmp_path):
  for d in ([1, 2], {'model_class': 'gc-bias'}, {'model_class': 'gc-bias', 'weight': ['a'] * 101},
            {'model_class': 'gc-bias', 'weight': [True] * 101}, {'model_class': 'gc-bias', 'weight': [-0.1] * 101}):
    with pytest.raises(ValueError):
      gcbias.load_curve(_write(tmp_path, d))
  p = str(tmp_path / 'bad.json')
  with open(p, 'w') as fp:
    fp.write('{not json')
  with pytest.raises(ValueError, match='JSON'):
    gcbias.load_curve(p)
  with pytest.raises(ValueError):
    gcbias.load_curve(str(tmp_path / 'missing.json'))
  w = np.linspace(0.25, 1.0, 101)
  gcbias.save_curve(p, w, 'ramp')
  assert np.array_equal(gcbias.load_curve(p), w)
  d = json.load(open(p))
  assert d['model_class'] == 'gc-bias' and d['description'] == 'ramp' and len(d['weight']) == 101
  with pytest.raises(ValueError):
    gcbias.save_curve(p, [2.0] * 101)


def _gc_cov(blocks, extra=None):
  """A gc-cov dict with one contig 'c1' of (gc, coverage, count) block groups."""
  gc = np.concatenate([np.full(n, g) for g, _, n in blocks])
  cov = np.concatenate([np.full(n, c) for _, c, n in blocks])
  a = np.empty(len(gc), dtype=[('gc', float), ('coverage', float)])
  a['gc'], a['coverage'] = gc, cov
  d = {'block_len': 10000, 'seq_info': [{'SN': 'c1', 'LN': 10000 * len(gc)}], 'c1': a}
  d.update(extra or {})
  return d


def test_fit_curve():
  nan = float('nan')
  # bins 30 (mean 10), 40 (mean 20) and 50 (mean 40) populated; 35 has too few blocks; NaN blocks are dropped
  d = _gc_cov([(0.305, 10.0, 30), (0.355, 999.0, 3), (0.405, 20.0, 25), (0.505, 30.0, 10), (0.509, 50.0, 10),
               (nan, 5.0, 40), (0.2, nan, 40)])
  w = gcbias.fit_curve(d, min_blocks=20, smooth=1)
  assert w.shape == (101,) and w.max() == 1.0 and w.min() > 0
  assert np.array_equal(w[:31], np.full(31, 0.25))        # below the first populated bin: its mean (10 / 40)
  assert np.array_equal(w[31:36], np.full(5, 0.25))       # 35 is equally far from 30 and 40: the lower bin wins
  assert np.array_equal(w[36:46], np.full(10, 0.5))       # 45 is equally far from 40 and 50: the lower bin again
  assert np.array_equal(w[46:], np.full(55, 1.0))
  # the moving average, truncated at the ends: width 5 around the 35 | 36 step
  w5 = gcbias.fit_curve(d, min_blocks=20, smooth=5)
  assert w5.max() == 1.0
  f = np.where(np.arange(101) < 36, 10.0, np.where(np.arange(101) < 46, 20.0, 40.0))
  want = np.array([f[max(0, b - 2):b + 3].mean() for b in range(101)])
  assert np.allclose(w5, want / want.max(), rtol=0, atol=1e-15)
  assert w5[0] == 0.25 and w5[100] == 1.0 and 0.25 < w5[34] < w5[35] < w5[36] < w5[37] < 0.5 + 1e-12
  # a lower min_blocks lets bin 35 in
  assert gcbias.fit_curve(d, min_blocks=3, smooth=1)[35] == 1.0
  # contigs past the first 24 of seq_info are not visited; a listed contig without an array is skipped
  many = _gc_cov([(0.5, 10.0, 30)])
  many['seq_info'] = [{'SN': 'x{}'.format(i), 'LN': 1} for i in range(24)] + many['seq_info']
  with pytest.raises(ValueError, match='no GC bin'):
    gcbias.fit_curve(many)
  with pytest.raises(ValueError, match='no GC bin'):
    gcbias.fit_curve(_gc_cov([(nan, nan, 50), (0.5, nan, 50)]))
  with pytest.raises(ValueError, match='odd'):
    gcbias.fit_curve(d, smooth=4)


def test_cli_gc_bias_model_round_trip(tmp_path):
  from click.testing import CliRunner
  from mitty_amd.cli import cli
  d = _gc_cov([(0.305, 10.0, 30), (0.405, 20.0, 25), (0.505, 40.0, 20)])
  pkl, out = str(tmp_path / 'gc.pkl'), str(tmp_path / 'curve.json')
  with open(pkl, 'wb') as fp:
    pickle.dump(d, fp)
  res = CliRunner().invoke(cli, ['gc-bias-model', pkl, out, '--min-blocks', '20', '--smooth', '3', '--desc', 'synthetic'])
  assert res.exit_code == 0, res.output + repr(res.exception)
  assert np.array_equal(gcbias.load_curve(out), gcbias.fit_curve(d, 20, 3))
  assert json.load(open(out))['description'] == 'synthetic'
  res = CliRunner().invoke(cli, ['gc-bias-model', '--help'])
  assert res.exit_code == 0 and 'trusted' in res.output
  with open(pkl, 'wb') as fp:
    pickle.dump(_gc_cov([(float('nan'), 1.0, 30)]), fp)
  res = CliRunner().invoke(cli, ['gc-bias-model', pkl, out])
  assert res.exit_code != 0 and 'no GC bin' in res.output
  res = CliRunner().invoke(cli, ['generate-reads', '--help'])
  assert res.exit_code == 0 and '--gc-bias' in res.output and '--gc-seed' in res.output


def test_cli_generate_reads_refuses_a_malformed_curve_before_any_device(tmp_path, monkeypatch):
  from click.testing import CliRunner
  from mitty_amd import _native
  from mitty_amd.cli import cli

  def no_device(*a, **k):
    raise AssertionError('a device context was created')
  monkeypatch.setattr(_native, 'Context', no_device)
  c = G.load_json('e2e_config.json')['hiseq-X-v2.5-Garvan']
  bad = _write(tmp_path, {'model_class': 'gc-bias', 'description': '', 'weight': [0.5] * 100})
  f1 = str(tmp_path / 'r1.fq')
  res = CliRunner().invoke(cli, ['generate-reads', G.path(c['fasta']), G.path(c['vcf']), c['sample'], G.path(c['bed']),
                                 'hiseq-X-v2.5-Garvan.pkl', str(c['coverage']), str(c['seed']), f1, '--gc-bias', bad])
  assert res.exit_code != 0 and not isinstance(res.exception, AssertionError)
  assert '101 weights' in res.output and '--gc-bias' in res.output
  import os
  assert not os.path.exists(f1)
  # the library entry point refuses it too, before the engine exists
  from mitty_amd.readmodel import get_read_model
  from mitty_amd.simulation import readgenerate
  mod, mdl = get_read_model('hiseq-X-v2.5-Garvan.pkl')
  with pytest.raises(ValueError, match='outside'):
    readgenerate.process_multi_threaded(G.path(c['fasta']), G.path(c['vcf']), c['sample'], G.path(c['bed']), mod, mdl,
                                        c['coverage'], f1, None, seed=c['seed'], gc_bias=[1.5] * 101)


def test_distributed_host_backend_refuses_a_curve(tmp_path):
  """A backend without set_gc_bias (the tests' host stand-in) cannot thin: a clear NotImplementedError."""
  from mitty_amd import distributed as D
  from mitty_amd.readmodel import get_read_model
  from tests import dist_host
  c = G.load_json('e2e_config.json')['hiseq-X-v2.5-Garvan']
  mod, mdl = get_read_model('hiseq-X-v2.5-Garvan.pkl')
  backend = dist_host.OracleBackend()
  with pytest.raises(NotImplementedError, match='set_gc_bias'):
    D.generate_reads_distributed(G.path(c['fasta']), G.path(c['vcf']), c['sample'], G.path(c['bed']), mod, mdl,
                                 c['coverage'], str(tmp_path / 'a.fq'), None, seed=c['seed'], backend=backend,
                                 gc_bias=[0.5] * 101)
