"""Plain restatements of what the haplotype splice (mh_splice.hip) produces, for the GPU tests: every structure is
rebuilt from the oracle's node arrays (oracle.create_node_list_soa, pinned to the reference by test_oracle_golden.py)
with NumPy and bytes operations, and the accept chain is walked once more in pure Python as a third opinion on which
variants are accepted.  Nothing here touches the GPU."""
import numpy as np

X, I, D, EQ, N = ord('X'), ord('I'), ord('D'), ord('='), ord('N')
FILL_SPAN = 16384        # bytes of haplotype one k_hap_fill workgroup writes
FILL_NODES = 512         # nodes of a span k_hap_fill stages in LDS (more: searched in global memory)
BKT = 256                # positions per node-search bucket
ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)
_COMP = bytes.maketrans(b'ATCGN', b'TAGCN')   # readgenerate.py:56


def contig(n, seed):
  """n i.i.d. bases (no N)."""
  return ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def soa(pos, op, oplen, seed=0):
  """A variant structure of arrays with alt bytes drawn at random: 'X' one base, 'I' oplen + 1, 'D' one."""
  pos = np.ascontiguousarray(pos, dtype=np.int64)
  op = np.ascontiguousarray(op, dtype=np.uint8)
  oplen = np.where(op == X, 0, np.asarray(oplen, dtype=np.int64)).astype(np.int64)
  alen = np.where(op == I, oplen + 1, 1).astype(np.int64)
  aoff = np.cumsum(alen) - alen
  pool = ACGT[np.random.default_rng(seed).integers(0, 4, int(alen.sum()))].tobytes()
  return {'pos': pos, 'op': op, 'oplen': oplen, 'alt_off': aoff.astype(np.int64), 'alt_len': alen, 'alt_pool': pool}


def soa_of(variants):
  """A variant structure of arrays from [(pos, op character, oplen, alt bytes)]."""
  alts = [v[3] for v in variants]
  alen = np.array([len(a) for a in alts], dtype=np.int64)
  return {'pos': np.array([v[0] for v in variants], dtype=np.int64),
          'op': np.array([ord(v[1]) for v in variants], dtype=np.uint8),
          'oplen': np.array([v[2] for v in variants], dtype=np.int64),
          'alt_off': (np.cumsum(alen) - alen).astype(np.int64), 'alt_len': alen, 'alt_pool': b''.join(alts)}


def accept_model(rs, v):
  """The reference's accept rule (rpc.py:55) walked sequentially in pure Python: a variant is accepted when its
  position is not before the ref cursor the last accepted variant left.  Returns (accepted, anchor) boolean arrays;
  an anchor is a variant at or past every earlier variant's end (accepted whatever happened before it)."""
  pos, op, oplen = v['pos'].tolist(), v['op'].tolist(), v['oplen'].tolist()
  acc, anchor = np.zeros(len(pos), bool), np.zeros(len(pos), bool)
  cur, far = rs, rs
  for i, (p, o, ln) in enumerate(zip(pos, op, oplen)):
    end = p + 1 + (ln if o == D else 0)
    anchor[i] = p >= far
    far = max(far, end)
    if p >= cur:
      acc[i] = True
      cur = end
  return acc, anchor


def run_lengths(mask):
  """Lengths of the maximal runs of True in a boolean array."""
  d = np.diff(np.concatenate(([0], np.asarray(mask, np.int8), [0])))
  return np.flatnonzero(d == -1) - np.flatnonzero(d == 1)


def n_runs_of(hap):
  """[start, end) offsets of the maximal runs of 'N' in the bytes hap."""
  d = np.diff(np.concatenate(([0], (np.frombuffer(hap, np.uint8) == N).astype(np.int8), [0])))
  return np.flatnonzero(d == 1).astype(np.int64), np.flatnonzero(d == -1).astype(np.int64)


class Expect:
  """Everything the splice keeps for one haplotype, restated from the oracle's node list."""

  def __init__(self, ref, rs, v):
    from oracle import oracle as O
    ps, pr, op, ol, src, off, sl = O.create_node_list_soa(ref, rs, v)
    self.ps, self.pr, self.op, self.oplen = ps, pr, op, ol
    self.n_nodes = len(ps)
    pool = v['alt_pool']
    self.hap = b''.join((pool if s else ref)[o:o + n]
                        for s, o, n, c in zip(src.tolist(), off.tolist(), sl.tolist(), op.tolist()) if c != D)
    self.rc = self.hap.translate(_COMP)[::-1]
    self.run_start, self.run_end = n_runs_of(self.hap)
    self.keys = ps + (op == D)
    self.p_min, self.p_max = int(ps[0]), int(ps[-1] + ol[-1])
    # the table's size is the library's choice (one bucket per 256 positions and 2048 positions of slack); what is
    # checked is that it reaches past every key, and each entry
    self.n_bkt = ((len(self.hap) + 2048) >> 8) + 1
    assert self.p_min + BKT * self.n_bkt > int(self.keys.max())
    self.bkt = np.searchsorted(self.keys, self.p_min + BKT * np.arange(self.n_bkt + 1), 'left').astype(np.int32)
    # third opinion on the accept chain: the variant nodes are exactly the accepted variants, in order
    self.accepted, self.anchor = accept_model(rs, v)
    self.var_of = np.flatnonzero(self.accepted)
    isv = op != EQ
    got_end = pr[isv] + np.where(op[isv] == X, 1, 0)            # the ref cursor after each variant node
    a = self.var_of
    want_end = v['pos'][a] + 1 + np.where(v['op'][a] == D, v['oplen'][a], 0)
    assert int(isv.sum()) == len(a) and np.array_equal(op[isv], v['op'][a]) and np.array_equal(got_end, want_end), \
      'the oracle and the sequential accept loop disagree'
    self._var_before = np.cumsum(isv) - isv

  def variant_of_node(self, k):
    """The index, in the variant list, of the variant node k belongs to ('trailing' for the last '=' node)."""
    j = int(self._var_before[min(k, self.n_nodes - 1)])
    return int(self.var_of[j]) if j < len(self.var_of) else 'trailing'

  def span_nodes(self):
    """Per FILL_SPAN bytes of haplotype, the nodes k_hap_fill stages for it: from the last node keyed below the
    span's first bucket to the first one past its last bucket."""
    out = []
    for b0 in range(0, max(len(self.hap), 1), FILL_SPAN):
      kb0, kb1 = min(b0 // BKT, self.n_bkt - 1), (b0 + FILL_SPAN - 1) // BKT + 1
      lo = max(int(self.bkt[kb0]) - 1, 0)
      hi = min(int(self.bkt[kb1]) + 1, self.n_nodes) if kb1 < self.n_bkt else self.n_nodes
      out.append(hi - lo)
    return np.array(out)

  def chunk_nodes(self):
    """The most nodes keyed inside one 16-byte chunk of the haplotype."""
    c = (self.keys - self.p_min) // 16
    return int(np.bincount(c[(c >= 0)]).max())


def same(got, want, what, where=None):
  """Exact equality of two arrays (or bytes); a failure names the first differing index and where(index)."""
  if isinstance(want, (bytes, bytearray)):
    got, want = np.frombuffer(bytes(got), np.uint8), np.frombuffer(bytes(want), np.uint8)
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype, '{}: dtype {} for {}'.format(what, got.dtype, want.dtype)
  assert got.shape == want.shape, '{}: {} elements for {}'.format(what, got.shape, want.shape)
  if not np.array_equal(got, want):
    i = int(np.flatnonzero(got != want)[0])
    raise AssertionError('{}: first difference at {}{}: got {} want {} ({} differ)'.format(
      what, i, ' ({})'.format(where(i)) if where else '', got[i], want[i], int((got != want).sum())))


def span_of(i):
  return 'workgroup span {}'.format(i // FILL_SPAN)
