"""Test-side helpers of the bam2illumina tests: the rule of the histogram pass stated in NumPy (pinned to the
reference by tests/test_model_cpu.py against tests/golden/model.json.gz), the golden fixture, and BAM records built
with the oracle's encoder."""
import hashlib
import struct

import numpy as np

from oracle import god as OG
from tests import golden_io as G

INT32_MIN = -(1 << 31)
N_VISITED = 24   # refs[:24]


class ModelError(ValueError):
  """Where the reference raises; .index is the record's index in the input."""

  def __init__(self, index, why):
    ValueError.__init__(self, 'record {}: {}'.format(index, why))
    self.index = index


def np_model(records, n_refs, every=1, min_mq=0, max_bq=94, max_bp=300, max_tlen=1000):
  """(bq_mat, tlen, counts) of (flag, tid, mapq, tlen, qualities) tuples in file order; tid < 0: unplaced; qualities
  a sequence of ints."""
  bq = np.zeros((2, max_bp, max_bq), np.uint64)
  tl = np.zeros(max_tlen, np.uint64)
  c = {'seen': 0, 'used': 0, 'skipped_unplaced': 0, 'skipped_ref': 0, 'skipped_every': 0, 'skipped_flag': 0,
       'min_rlen': None, 'max_rlen': 0}
  ordinal = {}
  for idx, (flag, tid, mapq, tlen, q) in enumerate(records):
    c['seen'] += 1
    if tid < 0:
      c['skipped_unplaced'] += 1
      continue
    if tid >= n_refs:
      raise ModelError(idx, 'tid')
    if tid >= N_VISITED:
      c['skipped_ref'] += 1
      continue
    n = ordinal.get(tid, 0)
    ordinal[tid] = n + 1
    if n % every:
      c['skipped_every'] += 1
      continue
    if flag > 255:
      c['skipped_flag'] += 1
      continue
    L = len(q)
    if L == 0 or L > max_bp:
      raise ModelError(idx, 'length')
    if max(q) >= max_bq:
      raise ModelError(idx, 'quality')
    c['used'] += 1
    qq = np.asarray(q[::-1] if flag & 0x10 else q, dtype=np.int64)
    bq[0 if flag & 0x40 else 1, np.arange(L), qq] += np.uint64(1)
    c['min_rlen'] = L if c['min_rlen'] is None else min(c['min_rlen'], L)
    c['max_rlen'] = max(c['max_rlen'], L)
    if mapq >= min_mq and mapq != 255 and flag & 0x80 and abs(tlen) < max_tlen:
      tl[abs(tlen)] += np.uint64(1)
  return bq, tl, c


def record(flag, tid, mapq, tlen, quals, qname='r', n_cigar=1, pos=100):
  """One BAM record (block_size included): the oracle encodes name, CIGAR, bases and qualities (bytes 0..255 given as
  ints); flag, MAPQ and TLEN are then set in place.  n_cigar 0: no CIGAR; k > 1: k operations."""
  L = len(quals)
  if n_cigar == 0 or L == 0:
    cigar = ''
  elif n_cigar == 1 or L < n_cigar:
    cigar = '{}M'.format(L)
  else:
    cigar = ''.join('1{}'.format('MX'[k & 1]) for k in range(n_cigar - 1)) + '{}M'.format(L - (n_cigar - 1))
  r = {'qname': qname, 'reference_id': tid, 'pos': pos if tid >= 0 else -1, 'cigarstring': cigar, 'mapq': mapq & 0xff,
       'is_reverse': 0, 'seq': 'ACGT' * (L // 4) + 'ACGT'[:L % 4], 'qual': ''.join(chr(33 + (v & 0xff)) for v in quals)}
  b = bytearray(OG.encode(r))
  struct.pack_into('<H', b, 18, flag)
  struct.pack_into('<i', b, 32, tlen)
  return bytes(b)


def offsets(recs):
  return np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)


_golden = None


def golden():
  """The fixture; 'tuples': (flag, tid, mapq, tlen, [q]) per record; 'recs': the same as BAM records."""
  global _golden
  if _golden is None:
    g = G.load_json('model.json.gz')
    tid = {s['SN']: i for i, s in enumerate(g['sq'])}
    g['tuples'] = [(f, -1 if ref is None else tid[ref], mq, tl, [ord(ch) - 33 for ch in q])
                   for f, ref, mq, tl, q in g['records']]
    g['recs'] = [record(*t, qname='g{}'.format(i)) for i, t in enumerate(g['tuples'])]
    _golden = g
  return _golden


def subset(g, s):
  """Indices of the golden records the parameter set `s` runs over."""
  return [i for i, t in enumerate(g['tuples']) if len(t[4]) <= s['max_len'] and max(t[4]) < s['max_q']]


def dense_bq(s):
  m = np.zeros(s['shape'], np.uint64)
  mi, ii, qi, cnt = s['bq']
  m[mi, ii, qi] = np.asarray(cnt, dtype=np.uint64)
  return m


def dense_tlen(s):
  t = np.zeros(s['n_tlen'], np.uint64)
  for i, n in s['tlen']:
    t[i] = n
  return t


def cum_sha256(a):
  return hashlib.sha256(np.ascontiguousarray(a, dtype='<f8').tobytes()).hexdigest()


def same_floats(got, want_hex, what):
  """Bit for bit, NaN in the same places."""
  want = np.array([float.fromhex(x) for x in want_hex], dtype=np.float64)
  got = np.asarray(got)
  assert got.dtype == np.float64 and got.shape == want.shape, what
  assert got.tobytes() == want.tobytes() or (np.array_equal(np.isnan(got), np.isnan(want)) and
                                            np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])), what


def check_model(model, s, what):
  """Every entry of a model dict against the golden set `s`."""
  assert sorted(model) == sorted(['model_class', 'model_description', 'min_mq', 'bq_mat', 'cum_bq_mat', 'tlen', 'r_cnt',
                                  'cum_tlen', 'mean_rlen', 'min_rlen', 'max_rlen']), what
  for k in ('model_class', 'min_mq', 'r_cnt', 'mean_rlen', 'min_rlen', 'max_rlen'):
    assert model[k] == s[k], (what, k, model[k], s[k])
  assert type(model['r_cnt']) is int, what
  bq, tl = np.asarray(model['bq_mat']), np.asarray(model['tlen'])
  assert bq.dtype == np.uint64 and tl.dtype == np.uint64, what
  assert np.array_equal(bq, dense_bq(s)), what + ': bq_mat'
  assert np.array_equal(tl, dense_tlen(s)), what + ': tlen'
  assert cum_sha256(model['cum_bq_mat']) == s['cum_bq_sha256'], what + ': cum_bq_mat'
  same_floats(model['cum_tlen'], s['cum_tlen'], what + ': cum_tlen')
