#!/usr/bin/env python3
"""Capture the golden vectors of the alignment scorers (mq-plot / derr-plot) from the reference — build container only.

Run:  python tests/golden/make_golden_score.py      (needs /root/reference; writes tests/golden/score.json.gz)

Like make_golden.py, the reference is imported from /root/reference through tests/golden/refshim.  Two more stand-ins
are installed here, at run time: a `matplotlib` / `matplotlib.pyplot` pair of empty modules (the reference's mq.py and
derr.py import them at module level; nothing is drawn), and `pysam.AlignmentFile`, an in-memory table of aligned reads
whose fetch(reference=SN) yields the records placed on SN, as htslib's does.

score.json.gz (data only):
  sq          the BAM header's @SQ list
  records     "aligned read" tuples [qname, flag, reference_name or null, pos (0-based), mapq]: qnames of the golden
              e2e FASTQ pairs (sample S1, both mates) and single-end qnames built from reads.json.gz (sample S2,
              every read from inside an insertion among them), each perturbed by the seeded rule in perturb()
  d_err       per record, readgenerate.score_alignment_error for strict 0/1 x max_d 200/5 (keys 's{strict}_d{max_d}')
  mq          mq.process_bam_part summed over sq, per 's{strict}_d{max_d}', as sparse [row, col, count] triples
  derr        derr.process_bam_part summed over sq, per 's{strict}_d{max_d}_v{max_v_len}' (max_v_len 10 is raised to
              51 first, as derr.process_bam does before it calls process_bam_part), sparse
  sample      the same two matrices for sample_name 'S1' (strict 0, max_d 200, max_v_len 200)
The matrices come from the reference's own process_bam_part loops (not from an accumulation written here);
process_bam itself is not run, because it only sums process_bam_part over the @SQ lines in a multiprocessing pool.
"""
import gzip
import json
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
MAX_D = 200


def load_json(name):
  opener = gzip.open if name.endswith('.gz') else open
  with opener(os.path.join(HERE, name), 'rt') as fp:
    return json.load(fp)


def qnames_paired():
  out = []
  for model, step in (('hiseq-X-v2.5-Garvan', 2), ('1kg-pcr-free', 1)):
    with gzip.open(os.path.join(HERE, 'e2e_{}.r1.fq.gz'.format(model)), 'rt') as fp:
      names = [l[1:].split()[0] for l in fp.read().split('\n')[0::4] if l]
    out += [q for i, q in enumerate(names) if i % step == 0 or '>' in q or 'D' in q]
  return out


def qnames_single():
  with open(os.path.join(HERE, 'data', 'syn.bed')) as fp:
    chroms = [l.split()[0] for l in fp if l.strip()]
  out = []
  for key, reads in sorted(load_json('reads.json.gz').items()):
    what, ri, cpy = key.split('|')
    if what != 'syn':
      continue
    for i, r in enumerate(reads):
      pos, cigar, v_list = r[4], r[5], r[6]
      if cigar.startswith('>') or (('D' in cigar or 'I' in cigar) and i % 8 == 0) or i % 40 == 0:
        out.append('S2:{}:{}:{}|{}|{}|{}|{}|{}|{}|{}'.format(ri, cpy, i, chroms[int(ri)], cpy, i & 1, pos, r[1], cigar,
                                                             ','.join(str(int(v)) for v in v_list)))
  return out


def perturb(rng, ri, flag, sq_names):
  """One aligned-read tuple (flag, reference_name, pos, mapq) for a read whose truth is `ri`."""
  mode = rng.choice(8, p=[0.34, 0.2, 0.1, 0.1, 0.08, 0.06, 0.06, 0.06])
  ref, pos = ri.chrom, ri.pos - 1
  if mode == 1:     # shifted by +-1 .. +-(max_d + 5)
    pos += int(rng.randint(1, MAX_D + 6)) * (1 if rng.randint(2) else -1)
  elif mode == 2:   # shifted by a few bases (inside the small max_d too)
    pos += int(rng.randint(1, 8)) * (1 if rng.randint(2) else -1)
  elif mode == 3:   # placed at the second breakpoint of a deletion read
    p = ri.pos
    for cnt, op in re.findall(r'(\d+)(\D)', ri.cigar):
      if op in '=MXD':
        p += int(cnt)
      if op == 'D':
        pos = p - 1
        break
  elif mode == 4:   # wrong chrom
    ref = sq_names[(sq_names.index(ri.chrom) + 1 + int(rng.randint(len(sq_names) - 1))) % len(sq_names)]
  elif mode == 5:   # unplaced: tid -1
    ref, pos, flag = None, -1, flag | 4
  elif mode == 6:   # flag 4 that still carries a position
    flag |= 4
  elif mode == 7:   # secondary alignment somewhere near
    flag |= 0x100
    pos += int(rng.randint(-30, 31))
  mapq = int(rng.randint(0, 100)) if rng.random_sample() < 0.3 else 60
  return flag, ref, max(pos, 0) if ref is not None else -1, mapq


def sparse(mat):
  r, c = np.nonzero(mat)
  return [[int(a), int(b), int(mat[a, b])] for a, b in zip(r, c)]


def main():
  sys.path[:0] = [os.path.join(HERE, 'refshim'), REF]
  mpl = types.ModuleType('matplotlib')
  mpl.use = lambda *a, **k: None
  mpl.pyplot = types.ModuleType('matplotlib.pyplot')
  sys.modules['matplotlib'], sys.modules['matplotlib.pyplot'] = mpl, mpl.pyplot
  import pysam
  import mitty.simulation.readgenerate as rg
  import mitty.benchmarking.mq as mq
  import mitty.benchmarking.derr as derr

  sq = load_json('god_header.json')
  sq_names = [s['SN'] for s in sq]
  rng = np.random.RandomState(20250611)
  records = []
  for q in qnames_paired():
    ris = rg.parse_qname(q)
    for mate, ri in enumerate(ris):
      flag = 0x1 | 0x2 | (0x40 if mate == 0 else 0x80) | (0x10 if ri.strand else 0)
      records.append((q,) + perturb(rng, ri, flag, sq_names))
  for q in qnames_single():
    ri = rg.parse_qname(q)[0]
    records.append((q,) + perturb(rng, ri, 0x10 if ri.strand else 0, sq_names))

  class Rec:
    __slots__ = ('qname', 'flag', 'reference_name', 'pos', 'mapq')

    def __init__(self, t):
      self.qname, self.flag, self.reference_name, self.pos, self.mapq = t

    @property
    def is_read2(self):
      return bool(self.flag & 0x80)

  table = [Rec(t) for t in records]

  class AlignmentFile:
    def __init__(self, fname, *a, **k):
      assert fname == 'golden'

    def fetch(self, reference=None):
      return (r for r in table if r.reference_name == reference)

  pysam.AlignmentFile = AlignmentFile

  out = {'sq': sq, 'records': [list(t) for t in records], 'd_err': {}, 'mq': {}, 'derr': {}}
  for strict in (0, 1):
    for max_d in (200, 5):
      k = 's{}_d{}'.format(strict, max_d)
      out['d_err'][k] = [int(rg.score_alignment_error(r, rg.parse_qname(r.qname)[1 if r.is_read2 else 0], max_d=max_d,
                                                      strict=bool(strict))) for r in table]
      out['mq'][k] = sparse(sum(mq.process_bam_part('golden', s, max_d, bool(strict), None) for s in sq_names))
      for mv in (200, 10):
        out['derr']['{}_v{}'.format(k, mv)] = sparse(sum(
          derr.process_bam_part('golden', s, max(mv, 51), max_d, bool(strict), None) for s in sq_names))
  out['sample'] = {
    'name': 'S1',
    'mq': sparse(sum(mq.process_bam_part('golden', s, 200, False, 'S1') for s in sq_names)),
    'derr': sparse(sum(derr.process_bam_part('golden', s, 200, 200, False, 'S1') for s in sq_names))}
  path = os.path.join(HERE, 'score.json.gz')
  with gzip.GzipFile(path, 'wb', mtime=0) as fp:
    fp.write(json.dumps(out, separators=(',', ':')).encode())
  print('{}: {} records, {} bytes'.format(path, len(records), os.path.getsize(path)))


if __name__ == '__main__':
  main()
