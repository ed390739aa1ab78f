"""GC-bias curves for generate-reads --gc-bias (the reference sampler's `# TODO: GC-bias goes here`,
mitty/simulation/illumina.py:67; no reference behaviour exists, so the rule is this project's own: mitty_hip.h
mh_gc_thin, restated in tests/gcbias_ref.py).

A curve is 101 weights w[b], b = 0 .. 100 (GC percent of the haplotype bytes a template spans), each finite and in
[0, 1], max > 0: a sampled template of bin b is kept with probability w[b].  fit_curve makes one from a gc-cov result
(empirical/gc.py), so what gc-cov measured on a sequencer's BAM can be simulated.  Host code only.
"""
import json

import numpy as np

N_BINS = 101
MODEL_CLASS = 'gc-bias'
MAX_CHROMS = 24   # gc-cov visits seq_info[:24] (empirical/gc.py)


def check_weight(weight):
  """The curve as float64[101]; ValueError naming what is wrong with it."""
  try:
    w = np.asarray(weight, dtype=np.float64)
  except (TypeError, ValueError):
    raise ValueError('gc-bias curve: the weights are not numbers')
  if w.shape != (N_BINS,):
    raise ValueError('gc-bias curve: {} weights needed (GC percent 0 .. 100), got {}'.format(
      N_BINS, 'shape {}'.format(w.shape) if w.ndim != 1 else len(w)))
  if not np.all(np.isfinite(w)):
    raise ValueError('gc-bias curve: weight {} is not finite'.format(int(np.flatnonzero(~np.isfinite(w))[0])))
  bad = np.flatnonzero((w < 0) | (w > 1))
  if len(bad):
    raise ValueError('gc-bias curve: weight {} = {} is outside [0, 1]'.format(int(bad[0]), w[bad[0]]))
  if not w.max() > 0:
    raise ValueError('gc-bias curve: every weight is zero')
  return w


def thresholds(weight):
  """uint64[101]: T[b] = min(2^32, floor(w[b] * 2^32)); a template of bin b is kept iff its 32-bit draw < T[b].
  (w * 2^32 is exact in f64: a power-of-two scale.)"""
  w = check_weight(weight)
  return np.minimum(np.floor(w * 4294967296.0), 4294967296.0).astype(np.uint64)


def load_curve(path):
  """The weights (float64[101]) of a curve file: JSON {"model_class": "gc-bias", "description": str,
  "weight": [101 floats]}.  Anything else is a ValueError naming what is wrong."""
  try:
    with open(path) as fp:
      d = json.load(fp)
  except (OSError, UnicodeDecodeError, ValueError) as e:   # (json.JSONDecodeError is a ValueError)
    raise ValueError('gc-bias curve {}: not readable as JSON ({})'.format(path, e))
  if not isinstance(d, dict):
    raise ValueError('gc-bias curve {}: a JSON object is needed'.format(path))
  if d.get('model_class') != MODEL_CLASS:
    raise ValueError('gc-bias curve {}: model_class is {!r}, not {!r}'.format(path, d.get('model_class'), MODEL_CLASS))
  if not isinstance(d.get('description', ''), str):
    raise ValueError('gc-bias curve {}: description is not a string'.format(path))
  if not isinstance(d.get('weight'), list):
    raise ValueError('gc-bias curve {}: no "weight" list'.format(path))
  if any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in d['weight']):
    raise ValueError('gc-bias curve {}: the weights are not numbers'.format(path))
  try:
    return check_weight(d['weight'])
  except ValueError as e:
    raise ValueError('{} ({})'.format(e, path))


def save_curve(path, weight, description=''):
  w = check_weight(weight)
  with open(path, 'w') as fp:
    json.dump({'model_class': MODEL_CLASS, 'description': str(description), 'weight': [float(x) for x in w]}, fp,
              indent=1)
    fp.write('\n')


def fit_curve(gc_cov, min_blocks=20, smooth=5):
  """A curve from a gc-cov result (the dict empirical/gc.py pickles): over the contigs of seq_info[:24] every block
  with finite gc and coverage goes to bin int(gc * 100); the mean coverage per bin; a bin with fewer than min_blocks
  blocks takes the nearest populated bin's mean (on a tie the lower bin); a centred moving average of odd width
  `smooth`, truncated at the ends; divided by the maximum.  ValueError when no bin is populated."""
  if smooth < 1 or smooth % 2 != 1:
    raise ValueError('fit_curve: smooth must be odd and positive, got {}'.format(smooth))
  tot, cnt = np.zeros(N_BINS), np.zeros(N_BINS, np.int64)
  for s in gc_cov['seq_info'][:MAX_CHROMS]:
    a = gc_cov.get(s['SN'])
    if a is None:
      continue
    gc, cov = np.asarray(a['gc'], np.float64), np.asarray(a['coverage'], np.float64)
    ok = np.isfinite(gc) & np.isfinite(cov)
    b = np.clip((gc[ok] * 100).astype(np.int64), 0, N_BINS - 1)
    tot += np.bincount(b, weights=cov[ok], minlength=N_BINS)
    cnt += np.bincount(b, minlength=N_BINS)
  pop = np.flatnonzero(cnt >= max(int(min_blocks), 1))
  if not len(pop):
    raise ValueError('fit_curve: no GC bin has {} blocks with finite gc and coverage'.format(max(int(min_blocks), 1)))
  mean = np.zeros(N_BINS)
  mean[pop] = tot[pop] / cnt[pop]
  # nearest populated bin; argmin takes the first of equally near ones, and pop ascends: the lower bin wins
  near = pop[np.abs(np.arange(N_BINS)[:, None] - pop[None, :]).argmin(axis=1)]
  filled = mean[near]
  h = smooth // 2
  sm = np.array([filled[max(0, b - h):b + h + 1].mean() for b in range(N_BINS)])
  top = sm.max()
  if not np.isfinite(top) or top <= 0:
    raise ValueError('fit_curve: the mean coverage is zero in every populated bin')
  return np.clip(sm / top, 0.0, 1.0)
