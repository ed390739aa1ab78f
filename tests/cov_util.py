"""Test-side helpers of the gc-cov and bq tests: the rule of both passes stated in NumPy (pinned to the reference by
tests/test_cov_cpu.py against tests/golden/cov.json.gz), the golden fixture, and BAM records built with the oracle's
encoder.

gc-cov's rule is this project's statement of `[b.n for b in bam_fp.pileup(region=...)]` with pysam's defaults (stepper
'all', truncate=False); there is no htslib here to pin it further.  A record is a tuple
(flag, tid, pos, cigar string, [qualities]); tid < 0: unplaced.

  visited   only the header's first min(24, n_ref) contigs; every record counts in 'seen'
  passes    flag & (0x4 | 0x100 | 0x200 | 0x400) == 0 (supplementary records pass)
  interval  [pos, end), end = pos + the lengths of M, D, N, = and X; end == pos: 'skipped_nospan', looked at no further
            (its pos is not checked); else pos < 0 or pos >= LN raises; end > LN is fine
  blocks    k = 0 .. len(range(1, LN, bl)) - 1; block k = [a, b) = [k bl, min(k bl + bl + 1, LN))
  per block R = the passing records with pos < b and end > a; S = sum over R of end - pos;
            U = #{x in [a, b): depth(x) > 0} + max(0, a - min_R pos) + max(0, max_R end - b)
htslib's max_depth (8000) is not modelled.
"""
import re
import struct

import numpy as np

from oracle import god as OG
from tests import golden_io as G

N_VISITED = 24
FLAG_MASK = 0x4 | 0x100 | 0x200 | 0x400
BQ_SHAPE = (500, 100)
NO_POS = (1 << 63) - 1
_OPS = re.compile(r'(\d+)([MIDNSHP=X])')


class CovError(ValueError):
  """Where the reference (or the BAM's own consistency) fails; .index is the record's index in the input."""

  def __init__(self, index, why):
    ValueError.__init__(self, 'record {}: {}'.format(index, why))
    self.index = index


def ref_span(cigar):
  return sum(int(n) for n, op in _OPS.findall(cigar) if op in 'MDN=X')


def n_blocks(ln, bl):
  return len(range(1, ln, bl))


def np_cov(records, lengths, block_len, seqs=None):
  """({contig index: dict of int64 arrays n, span_sum, min_pos, max_end, covered[, n_n, n_gc]}, counts) over the
  visited contigs; seqs: the contigs' bytes (those of the visited ones are used)."""
  bl = int(block_len)
  n_refs = len(lengths)
  n_vis = min(N_VISITED, n_refs)
  c = {'seen': 0, 'used': 0, 'skipped_unplaced': 0, 'skipped_ref': 0, 'skipped_flag': 0, 'skipped_nospan': 0}
  diff = [np.zeros(lengths[i] + 1, np.int64) for i in range(n_vis)]
  out = {}
  for i in range(n_vis):
    nb = n_blocks(lengths[i], bl)
    a = np.arange(nb, dtype=np.int64) * bl
    out[i] = {'a': a, 'b': np.minimum(a + bl + 1, lengths[i]), 'span_sum': np.zeros(nb, np.int64),
              'min_pos': np.full(nb, NO_POS, np.int64), 'max_end': np.zeros(nb, np.int64)}
  for idx, (flag, tid, pos, cigar, _) in enumerate(records):
    c['seen'] += 1
    if tid < 0:
      c['skipped_unplaced'] += 1
    elif tid >= n_refs:
      raise CovError(idx, 'tid')
    elif tid >= N_VISITED:
      c['skipped_ref'] += 1
    elif flag & FLAG_MASK:
      c['skipped_flag'] += 1
    else:
      end = pos + ref_span(cigar)
      if end == pos:
        c['skipped_nospan'] += 1
        continue
      if pos < 0 or pos >= lengths[tid]:
        raise CovError(idx, 'pos')
      c['used'] += 1
      diff[tid][pos] += 1
      diff[tid][min(end, lengths[tid])] -= 1
      o = out[tid]
      hit = (pos < o['b']) & (end > o['a'])
      o['span_sum'][hit] += end - pos
      o['min_pos'][hit] = np.minimum(o['min_pos'][hit], pos)
      o['max_end'][hit] = np.maximum(o['max_end'][hit], end)
  for i in range(n_vis):
    o = out[i]
    covered = np.concatenate([[0], np.cumsum(np.cumsum(diff[i])[:lengths[i]] > 0)]).astype(np.int64)
    o['covered'] = covered[o['b']] - covered[o['a']]
    o['n'] = o['b'] - o['a']
    if seqs is not None:
      s = np.frombuffer(seqs[i], np.uint8)
      assert len(s) == lengths[i]
      for key, chars in (('n_n', b'N'), ('n_gc', b'GC')):
        cum = np.concatenate([[0], np.cumsum(np.isin(s, list(chars)))]).astype(np.int64)
        o[key] = cum[o['b']] - cum[o['a']]
  return out, c


def np_bq(records, n_refs):
  """({contig index: u64[500, 100]}, counts) of bq.py:20-35 over the visited contigs."""
  n_vis = min(N_VISITED, n_refs)
  mats = {i: np.zeros(BQ_SHAPE, np.uint64) for i in range(n_vis)}
  c = {'seen': 0, 'used': 0, 'skipped_unplaced': 0, 'skipped_ref': 0, 'skipped_flag': 0}
  for idx, (flag, tid, _, _, q) in enumerate(records):
    c['seen'] += 1
    if tid < 0:
      c['skipped_unplaced'] += 1
    elif tid >= n_refs:
      raise CovError(idx, 'tid')
    elif tid >= N_VISITED:
      c['skipped_ref'] += 1
    elif flag > 255:
      c['skipped_flag'] += 1
    else:
      if len(q) == 0 or len(q) > BQ_SHAPE[0]:
        raise CovError(idx, 'length')
      if max(q) >= BQ_SHAPE[1]:
        raise CovError(idx, 'quality')
      c['used'] += 1
      qq = np.asarray(q[::-1] if flag & 0x10 else q, dtype=np.int64)
      mats[tid][np.arange(len(qq)), qq] += np.uint64(1)
  return mats, c


def record(flag, tid, pos, cigar, quals, qname='r'):
  """One BAM record (block_size included): the oracle encodes name, CIGAR, bases and qualities (bytes 0..255 given as
  ints); the flag is then set in place."""
  L = len(quals)
  r = {'qname': qname, 'reference_id': tid, 'pos': pos, 'cigarstring': cigar, 'mapq': 60, 'is_reverse': 0,
       'seq': 'ACGT' * (L // 4) + 'ACGT'[:L % 4], 'qual': ''.join(chr(33 + (v & 0xff)) for v in quals)}
  b = bytearray(OG.encode(r))
  struct.pack_into('<H', b, 18, flag)
  return bytes(b)


def offsets(recs):
  return np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)


_golden = None


def golden():
  """The fixture; 'tuples': (flag, tid, pos, cigar, [q]) per record; 'recs': the same as BAM records; 'lengths';
  'seqs': the contigs' bytes in header order."""
  global _golden
  if _golden is None:
    g = G.load_json('cov.json.gz')
    tid = {s['SN']: i for i, s in enumerate(g['sq'])}
    g['tuples'] = [(f, -1 if ref is None else tid[ref], pos, cig, [ord(ch) - 33 for ch in q])
                   for f, ref, pos, cig, q in g['records']]
    g['recs'] = [record(*t, qname='g{}'.format(i)) for i, t in enumerate(g['tuples'])]
    g['lengths'] = [s['LN'] for s in g['sq']]
    g['seqs'] = [g['fasta'][s['SN']].encode() for s in g['sq']]
    _golden = g
  return _golden


def fasta_text(g, width=60):
  out = []
  for s, seq in zip(g['sq'], g['seqs']):
    out.append(b'>' + s['SN'].encode() + b'\n')
    out += [seq[o:o + width] + b'\n' for o in range(0, len(seq), width)]
  return b''.join(out)


def header_text(g):
  return '@HD\tVN:1.4\tSO:unsorted\n' + ''.join(
    '@SQ\t' + '\t'.join('{}:{}'.format(k, v) for k, v in s.items()) + '\n' for s in g['sq'])


def floats(hex_list):
  return np.array([float.fromhex(x) if x != 'nan' else np.nan for x in hex_list], dtype=np.float64)


def same_floats(got, want, what):
  """Bit for bit, NaN in the same places."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == np.float64 and got.shape == want.shape, what
  assert np.array_equal(np.isnan(got), np.isnan(want)), what + ': NaN places'
  ok = ~np.isnan(want)
  assert got[ok].tobytes() == want[ok].tobytes(), what


def check_gc_cov(d, s, g, what):
  """A gc-cov output dict against the golden set `s`."""
  names = [q['SN'] for q in g['sq'][:N_VISITED]]
  assert sorted(d) == sorted(['block_len', 'seq_info'] + names), what
  assert d['block_len'] == s['block_len'] and d['seq_info'] == g['sq'], what
  for q in d['seq_info']:
    assert type(q['LN']) is int and all(type(v) is str for k, v in q.items() if k != 'LN'), what
  for sn in names:
    a = d[sn]
    assert a.dtype == np.dtype([('gc', float), ('coverage', float)]) and a.ndim == 1, (what, sn)
    same_floats(a['gc'], floats(s['gc'][sn]), '{} {} gc'.format(what, sn))
    same_floats(a['coverage'], floats(s['coverage'][sn]), '{} {} coverage'.format(what, sn))


def dense_bq(sparse):
  m = np.zeros(BQ_SHAPE, np.uint64)
  i, q, n = sparse
  m[i, q] = np.asarray(n, dtype=np.uint64)
  return m


def check_bq(d, s, g, what):
  names = [q['SN'] for q in g['sq'][:N_VISITED]]
  assert sorted(d) == sorted(['seq_info'] + names) and d['seq_info'] == g['sq'], what
  for sn in names:
    assert d[sn].dtype == np.uint64 and d[sn].shape == BQ_SHAPE, (what, sn)
    assert np.array_equal(d[sn], dense_bq(s[sn])), '{} {}'.format(what, sn)
