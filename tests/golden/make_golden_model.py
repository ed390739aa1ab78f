#!/usr/bin/env python3
"""Capture the golden vectors of bam2illumina from the reference — build container only.

Run:  python tests/golden/make_golden_model.py      (needs /root/reference; writes tests/golden/model.json.gz)

Like make_golden_score.py, the reference is imported from /root/reference through tests/golden/refshim, with empty
`matplotlib` stand-ins and an in-memory `pysam.AlignmentFile`: .header['SQ'] is the @SQ list and fetch(reference=SN)
yields the records placed on SN in file order, as htslib's does for a sorted file.  The reference's own
process_bam_parallel runs (its multiprocessing Pool included: the workers are forked after the stand-in is installed)
and writes a .pkl, which is read back here.

model.json.gz (data only):
  sq        the BAM header's @SQ list, 26 names: only the first 24 are visited
  records   [flag, reference_name or null, mapq, tlen, qualities as a phred+33 string], seeded (see records())
  sets      per parameter set: 'params' (process_bam_parallel's keyword arguments), 'max_len' and 'max_q' (the set runs
            over the records with at most max_len qualities, all below max_q: the reference raises on the others), and
            the reference's model: bq_mat sparse (four parallel lists m, i, q, count), tlen sparse ([t, count]),
            cum_tlen as float.hex() per entry, sha256 of cum_bq_mat's little-endian f64 bytes (C order), the scalars
  empty     the model of a file without records (defaults)
"""
import gzip
import hashlib
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
INT32_MIN = -(1 << 31)

SETS = {
  'defaults': ({}, 300, 94),
  'every3': ({'every': 3, 'min_mq': 20, 'max_bp': 160, 'max_tlen': 500}, 160, 94),
  'bq50': ({'max_bq': 50}, 300, 50),
}


def quals(rng, n, low):
  """n qualities: a few values per position (hot cells), falling along the read; `low`: all below 50."""
  top = 41 if low else int(rng.choice([41, 41, 60, 93]))
  q = top - (np.arange(n) // 25) * 3 - rng.choice([0, 0, 0, 0, 2, 7, 25], size=n)
  return ''.join(chr(33 + int(v)) for v in np.clip(q, 2 if low else 0, top))


def records(rng, sq_names):
  out = []
  edge_tlen = [999, -999, 1000, -1000, 499, -499, 500, -500, INT32_MIN, 0]
  for i in range(1600):
    n = int(rng.randint(1, 151))
    if i % 97 == 0:
      n = 300   # exactly the default max_bp
    elif i % 89 == 0:
      n = 160   # exactly max_bp of the second set
    elif i % 61 == 0:
      n = int(rng.choice([1, 63, 64, 65, 127, 129, 150]))
    flag = 0x1 | 0x2 | (0x40 if rng.randint(2) else 0x80) | (0x10 if rng.randint(2) else 0)
    u = rng.random_sample()
    if u < 0.04:
      flag &= ~0xc0     # neither mate bit
    elif u < 0.08:
      flag |= 0xc0      # both
    elif u < 0.16:
      flag |= int(rng.choice([0x100, 0x200, 0x400, 0x800]))
    elif u < 0.19:
      flag |= 0x4       # unmapped flag on a placed record: still visited
    ref = sq_names[int(rng.choice([0, 0, 0, 1, 1, 2, 5, 23]))]
    v = rng.random_sample()
    if v < 0.05:
      ref = sq_names[24]   # contig #25
    elif v < 0.07:
      ref = sq_names[25]
    elif v < 0.11:
      ref = None
    mapq = int(rng.choice([0, 10, 60, 60, 60, 255]))
    tlen = (int(rng.choice(edge_tlen)) if rng.random_sample() < 0.15
            else int(rng.normal(350, 60)) * (1 if rng.randint(2) else -1))
    out.append([flag, ref, mapq, tlen, quals(rng, n, low=rng.random_sample() < 0.4)])
  return out


def sparse_bq(bq):
  m, i, q = np.nonzero(bq)
  return [m.tolist(), i.tolist(), q.tolist(), bq[m, i, q].tolist()]


def model_json(m):
  cum = np.ascontiguousarray(m['cum_bq_mat'], dtype='<f8')
  return {
    'model_class': m['model_class'], 'model_description': m['model_description'], 'min_mq': m['min_mq'],
    'r_cnt': m['r_cnt'], 'mean_rlen': m['mean_rlen'], 'min_rlen': m['min_rlen'], 'max_rlen': m['max_rlen'],
    'shape': list(m['bq_mat'].shape), 'n_tlen': int(m['tlen'].shape[0]),
    'bq': sparse_bq(m['bq_mat']), 'tlen': [[int(t), int(m['tlen'][t])] for t in np.flatnonzero(m['tlen'])],
    'cum_bq_sha256': hashlib.sha256(cum.tobytes()).hexdigest(),
    'cum_tlen': [float(x).hex() for x in m['cum_tlen']],
  }


def main():
  sys.path[:0] = [os.path.join(HERE, 'refshim'), REF]
  mpl = types.ModuleType('matplotlib')
  mpl.use = lambda *a, **k: None
  mpl.pyplot = types.ModuleType('matplotlib.pyplot')
  sys.modules['matplotlib'], sys.modules['matplotlib.pyplot'] = mpl, mpl.pyplot
  import pysam
  import mitty.empirical.bam2illumina as b2i

  sq = [{'SN': 'c{}'.format(i + 1), 'LN': 100000 + 1000 * i} for i in range(26)]
  sq_names = [s['SN'] for s in sq]
  recs = records(np.random.RandomState(20250704), sq_names)

  class Rec:
    __slots__ = ('flag', 'reference_name', 'mapq', 'tlen', 'query_qualities')

    def __init__(self, t):
      self.flag, self.reference_name, self.mapq, self.tlen = t[:4]
      self.query_qualities = [ord(c) - 33 for c in t[4]]

    is_read1 = property(lambda s: bool(s.flag & 0x40))
    is_read2 = property(lambda s: bool(s.flag & 0x80))
    rlen = property(lambda s: len(s.query_qualities))

  tables = {}

  class AlignmentFile:
    def __init__(self, fname, mode='rb', *a, **k):
      self.table = tables[fname]
      self.header = {'SQ': sq}

    def fetch(self, reference=None):
      return (r for r in self.table if r.reference_name == reference)

  pysam.AlignmentFile = AlignmentFile

  def run(name, kw):
    with tempfile.TemporaryDirectory() as d:
      pkl = os.path.join(d, 'm.pkl')
      b2i.process_bam_parallel(name, pkl, model_description='golden ' + name, threads=3, **kw)
      with open(pkl, 'rb') as fp:
        return model_json(pickle.load(fp))

  out = {'sq': sq, 'records': recs, 'sets': {}}
  for name, (kw, max_len, max_q) in SETS.items():
    tables[name] = [Rec(t) for t in recs if len(t[4]) <= max_len and max(ord(c) - 33 for c in t[4]) < max_q]
    out['sets'][name] = dict(run(name, kw), params=kw, max_len=max_len, max_q=max_q, n_records=len(tables[name]))
  tables['empty'] = []
  with np.errstate(all='ignore'):
    out['empty'] = run('empty', {})
  path = os.path.join(HERE, 'model.json.gz')
  with gzip.GzipFile(path, 'wb', mtime=0) as fp:
    fp.write(json.dumps(out, separators=(',', ':')).encode())
  print('{}: {} records, {} bytes; {}'.format(path, len(recs), os.path.getsize(path),
                                               {k: (v['r_cnt'], v['n_records']) for k, v in out['sets'].items()}))


if __name__ == '__main__':
  main()
