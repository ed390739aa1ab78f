"""Test-side helpers of the alignment-scoring tests: a small BGZF writer, BAM files built from the oracle's record
encoder (oracle.god.encode / header_bytes), and the golden score fixture (tests/golden/score.json.gz)."""
import struct
import zlib

import numpy as np

from oracle import god as OG
from tests import golden_io as G

BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def bgzf_block(raw, level=6):
  c = zlib.compressobj(level, zlib.DEFLATED, -15)
  z = c.compress(raw) + c.flush()
  return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(z) + 25) + z +
          struct.pack('<II', zlib.crc32(raw), len(raw)))


def bgzf_bytes(data, block=0xff00, level=6, eof=True):
  """`data` as BGZF blocks of `block` input bytes (any 1..65280: small blocks make records straddle them)."""
  out = [bgzf_block(data[o:o + block], level) for o in range(0, len(data), block)]
  return b''.join(out) + (BGZF_EOF if eof else b'')


def record(qname, flag, tid, pos, mapq, seq='ACGT', cigar=None):
  """One BAM record (block_size included) with the given core fields; the oracle encodes, the flag is then set."""
  r = {'qname': qname, 'reference_id': tid, 'pos': pos, 'cigarstring': cigar or '{}M'.format(len(seq)), 'mapq': mapq,
       'is_reverse': 0, 'seq': seq, 'qual': '~' * len(seq)}
  b = bytearray(OG.encode(r))
  struct.pack_into('<H', b, 18, flag)
  return bytes(b)


def bam_bytes(recs, sq, text='@HD\tVN:1.4\n'):
  return OG.header_bytes(text, sq) + b''.join(recs)


def offsets(recs):
  return np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)


_golden = None


def golden():
  """The fixture, with every tuple also encoded as a BAM record ('recs') once for all tests."""
  global _golden
  if _golden is None:
    g = G.load_json('score.json.gz')
    tid = {s['SN']: i for i, s in enumerate(g['sq'])}
    g['recs'] = [record(q, flag, -1 if ref is None else tid[ref], pos, mapq) for q, flag, ref, pos, mapq in g['records']]
    _golden = g
  return _golden


def py_matrices(aligned, max_d=200, max_v_len=200, strict=False, sample=None):
  """(mq_mat, d_err_mat) of (qname, flag, reference_name or None, pos, mapq) tuples by the Python statement of the
  rule (readgenerate.score_alignment_error, itself pinned to the reference by test_score_cpu.py), accumulated as
  mq.py:63-67 / derr.py:67-75 do."""
  import collections
  from mitty_amd.simulation import readgenerate as rg
  A = collections.namedtuple('A', ['pos', 'reference_name'])
  max_v = max(max_v_len, 51)
  mq = np.zeros((100, 2 * max_d + 1), np.uint64)
  dv = np.zeros((2 * max_v + 2, 2 * max_d + 1), np.uint64)
  for q, flag, ref, pos, mapq in aligned:
    if ref is None or (sample is not None and not q.startswith(sample)):
      continue
    ri = rg.parse_qname(q)[1 if flag & 0x80 else 0]
    d = rg.score_alignment_error(A(pos, ref), ri, max_d=max_d, strict=strict)
    mq[mapq, d + max_d] += 1
    if len(ri.v_list):
      for v in ri.v_list:
        if 0 <= max_v + v < 2 * max_v + 1:
          dv[max_v + v, d + max_d] += 1
    else:
      dv[-1, d + max_d] += 1
  return mq, dv


def dense(triples, shape):
  m = np.zeros(shape, np.uint64)
  for r, c, n in triples:
    m[r, c] = n
  return m
