#!/usr/bin/env python3
"""Capture the golden vectors of gc-cov and bq from the reference — build container only.

Run:  python tests/golden/make_golden_cov.py      (needs /root/reference; writes tests/golden/cov.json.gz)

Like make_golden_model.py, the reference is imported from /root/reference through tests/golden/refshim, with empty
`matplotlib` stand-ins and in-memory pysam stand-ins:
  pysam.FastaFile.fetch(region='SN:s-e')   the 1-based inclusive region of the sequence, clipped to its end
  pysam.AlignmentFile   .header['SQ'] is the @SQ list; fetch(reference=SN) yields the records placed on SN in file
                        order; pileup(region='SN:s-e') is the brute-force statement of htslib's pileup with pysam's
                        defaults (stepper 'all': flag & 0x704 removed; truncate=False): the passing records with a
                        reference span that overlap the region are selected, every column of every selected record
                        (inside the region or not, deleted and skipped columns included) is walked into a dict, and one
                        object with .n is yielded per column.  No closed form enters here: the golden pins the closed
                        form of tests/cov_util.py through the reference's own arithmetic.
The reference's own process_bam_parallel of both modules runs (its multiprocessing Pool included) and writes a .pkl,
which is read back here.

cov.json.gz (data only):
  sq        the BAM header's @SQ list, 26 lines (SN, LN, sometimes further tags): only the first 24 are visited
  fasta     {SN: sequence}
  records   [flag, reference_name or null, pos, CIGAR string, qualities as a phred+33 string], seeded (see records())
  sets      per gc-cov parameter set: block_len, and per visited SN 'gc' and 'coverage' as float.hex() lists ('nan')
  bq        per visited SN the reference's matrix, sparse (three parallel lists i, q, count)
  empty     the same two results for a file without records ('gc_cov' with block_len 100, 'bq')
"""
import gzip
import json
import os
import pickle
import re
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
BLOCK_LENS = {'bl100': 100, 'bl37': 37, 'bl1000': 1000}
FLAG_MASK = 0x4 | 0x100 | 0x200 | 0x400
LENGTHS = [5000, 6000, 750, 201, 1111, 4001, 4097, 4500, 5999, 1, 2, 3, 38, 75, 100, 101, 2048, 2049, 999, 1000, 1001,
           4096, 150, 64, 3000, 500]


def sequences(rng):
  out = []
  for ln in LENGTHS:
    s = rng.choice(list(b'ACGT'), size=ln).astype(np.uint8)
    for _ in range(ln // 400):   # N runs, lower-case runs (not counted), IUPAC bytes
      o, n = int(rng.randint(ln)), int(rng.choice([1, 5, 11, 12, 40, 130]))
      s[o:o + n] = ord('N')
    for _ in range(ln // 300):
      o, n = int(rng.randint(ln)), int(rng.randint(1, 60))
      s[o:o + n] = rng.choice(list(b'gcat'), size=len(s[o:o + n]))
    for _ in range(ln // 200):
      s[int(rng.randint(ln))] = int(rng.choice(list(b'RYSWKMn')))
    out.append(s)
  # exactly 10 % N (kept: the test is > 0.1) in the last block of each set, and a block just above 10 % next to it
  def acgt(n):
    return rng.choice(list(b'ACGT'), size=n).astype(np.uint8)

  s = out[0]                  # block_len 100: the last block is [4900, 5000), n = 100
  s[4800:] = acgt(200)
  s[4900:4910] = ord('N')
  s[4810:4821] = ord('N')     # 11 of 101
  s = out[1]                  # block_len 1000: the last block is [5000, 6000), n = 1000
  s[4990:] = acgt(1010)
  s[5000:5100] = ord('N')
  s[3000:4001] = acgt(1001)
  s[3100:3201] = ord('N')     # 101 of 1001
  s = out[2]                  # block_len 37: the last block is [740, 750), n = 10
  s[700:] = acgt(50)
  s[745] = ord('N')
  s[710:714] = ord('N')       # 4 of 38
  return [bytes(x).decode() for x in out]


def cigar_for(rng, L):
  """A CIGAR whose query-consuming operations sum to L."""
  kind = rng.randint(10)
  if kind == 0:
    return ''
  if kind == 1 or L < 6:
    return '{}M'.format(L)
  a = int(rng.randint(1, L - 4))
  b = int(rng.randint(1, L - a - 2))
  c = L - a - b
  if kind == 2:
    return '{}S{}M{}S'.format(a, b, c)
  if kind == 3:
    return '5H{}M{}I{}M'.format(a, b, c)
  if kind == 4:
    return '{}M{}D{}M'.format(a, int(rng.randint(1, 30)), b + c)
  if kind == 5:
    return '{}M{}N{}M'.format(a, int(rng.choice([40, 120, 250, 1200])), b + c)
  if kind == 6:
    return '{}={}X{}='.format(a, b, c)
  if kind == 7:
    return '{}S{}I'.format(a, b + c)   # no reference span
  if kind == 8:
    return '{}M2P{}I{}M3H'.format(a, b, c)
  return '{}M{}D{}I{}N{}M'.format(a, 2, b, 7, c)


def records(rng, sq):
  out = []
  for i in range(2000):
    L = int(rng.randint(1, 151))
    if i % 211 == 0:
      L = 500
    flag = int(rng.choice([0, 0x10, 0x63, 0x93, 0x53, 0xa3]))
    u = rng.random_sample()
    if u < 0.16:
      flag |= int(rng.choice([0x4, 0x100, 0x200, 0x400, 0x800]))
    ci = int(rng.choice([0, 0, 0, 1, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 16, 17, 21, 23]))
    v = rng.random_sample()
    if v < 0.04:
      ci = 24
    elif v < 0.07:
      ci = 25
    ln = LENGTHS[ci]
    pos = int(rng.randint(ln))
    cigar = cigar_for(rng, L)
    w = rng.random_sample()
    if w < 0.05:     # only a block's shared base
      pos, cigar, L = min(ln - 1, int(rng.choice([37, 100, 1000])) * int(rng.randint(1, 4))), '1M', 1
    elif w < 0.10:   # past the contig's end
      pos = max(0, ln - int(rng.randint(1, 10)))
    elif w < 0.13:
      pos = 0
    top = int(rng.choice([41, 60, 99]))
    q = np.clip(top - (np.arange(L) // 25) * 3 - rng.choice([0, 0, 0, 2, 7, 25], size=L), 0, 99)
    ref = None if v > 0.97 else sq[ci]['SN']
    out.append([flag, ref, -1 if ref is None else pos, cigar, ''.join(chr(33 + int(x)) for x in q)])
  return out


def span(cigar):
  return sum(int(n) for n, op in re.findall(r'(\d+)([MIDNSHP=X])', cigar) if op in 'MDN=X')


def main():
  sys.path[:0] = [os.path.join(HERE, 'refshim'), REF]
  mpl = types.ModuleType('matplotlib')
  mpl.use = lambda *a, **k: None
  mpl.pyplot = types.ModuleType('matplotlib.pyplot')
  mpl.colors = types.ModuleType('matplotlib.colors')
  mpl.colors.LogNorm = None
  sys.modules['matplotlib'], sys.modules['matplotlib.pyplot'], sys.modules['matplotlib.colors'] = \
    mpl, mpl.pyplot, mpl.colors
  import pysam
  import mitty.empirical.bq as rbq
  import mitty.empirical.gc as rgc

  rng = np.random.RandomState(20250911)
  sq = [{'SN': 'c{}'.format(i + 1), 'LN': ln} for i, ln in enumerate(LENGTHS)]
  sq[1]['AS'] = 'syn'
  sq[4].update({'M5': '0123abcd', 'SP': 'none'})
  seqs = sequences(rng)
  fasta = {s['SN']: x for s, x in zip(sq, seqs)}
  recs = records(rng, sq)
  ln_of = {s['SN']: s['LN'] for s in sq}

  def parse_region(r):
    sn, se = r.rsplit(':', 1)
    s, e = se.split('-')
    return sn, int(s) - 1, min(int(e), ln_of[sn])

  class FastaFile:
    def __init__(self, fname):
      pass

    def fetch(self, region=None):
      sn, a, b = parse_region(region)
      return fasta[sn][a:b]

  class Rec:
    __slots__ = ('flag', 'reference_name', 'pos', 'cigar', 'query_qualities', 'end')

    def __init__(self, t):
      self.flag, self.reference_name, self.pos, self.cigar = t[:4]
      self.query_qualities = [ord(c) - 33 for c in t[4]]
      self.end = self.pos + span(self.cigar)

  class Column:
    __slots__ = ('n',)

    def __init__(self, n):
      self.n = n

  tables = {}

  class AlignmentFile:
    def __init__(self, fname, mode='rb', *a, **k):
      self.table = tables[fname]
      self.header = {'SQ': sq}

    def fetch(self, reference=None):
      return (r for r in self.table if r.reference_name == reference)

    def pileup(self, region=None):
      sn, a, b = parse_region(region)
      sel = [r for r in self.table if r.reference_name == sn and not r.flag & FLAG_MASK and r.end > r.pos and
             r.pos < b and r.end > a]
      cols = {}
      for r in sel:
        for x in range(r.pos, r.end):
          cols[x] = cols.get(x, 0) + 1
      return (Column(cols[x]) for x in sorted(cols))

  pysam.AlignmentFile, pysam.FastaFile = AlignmentFile, FastaFile

  def hexes(a):
    return ['nan' if np.isnan(x) else float(x).hex() for x in a]

  def run_gc(name, bl):
    with tempfile.TemporaryDirectory() as d:
      pkl = os.path.join(d, 'g.pkl')
      rgc.process_bam_parallel(name, 'fa', pkl, block_len=bl, threads=3)
      with open(pkl, 'rb') as fp:
        m = pickle.load(fp)
    assert m['block_len'] == bl and m['seq_info'] == sq and len(m) == 2 + 24
    return {'block_len': bl, 'gc': {s['SN']: hexes(m[s['SN']]['gc']) for s in sq[:24]},
            'coverage': {s['SN']: hexes(m[s['SN']]['coverage']) for s in sq[:24]}}

  def run_bq(name):
    with tempfile.TemporaryDirectory() as d:
      pkl = os.path.join(d, 'b.pkl')
      rbq.process_bam_parallel(name, pkl, threads=3)
      with open(pkl, 'rb') as fp:
        m = pickle.load(fp)
    assert m['seq_info'] == sq and len(m) == 1 + 24
    out = {}
    for s in sq[:24]:
      i, q = np.nonzero(m[s['SN']])
      out[s['SN']] = [i.tolist(), q.tolist(), m[s['SN']][i, q].tolist()]
    return out

  tables['all'] = [Rec(t) for t in recs]
  tables['empty'] = []
  out = {'sq': sq, 'fasta': fasta, 'records': recs, 'sets': {k: run_gc('all', bl) for k, bl in BLOCK_LENS.items()},
         'bq': run_bq('all'), 'empty': {'gc_cov': run_gc('empty', 100), 'bq': run_bq('empty')}}
  path = os.path.join(HERE, 'cov.json.gz')
  with gzip.GzipFile(path, 'wb', mtime=0) as fp:
    fp.write(json.dumps(out, separators=(',', ':')).encode())
  print('{}: {} records, {} bytes'.format(path, len(recs), os.path.getsize(path)))


if __name__ == '__main__':
  main()
