"""GPU tests of what the four record sessions (score, read model, bq, gc-cov) have in common: the text of a failing
record's error, the errors of calls out of order, sessions open side by side on one context, and results that can be
read again and added to.  The sums are checked against the NumPy / Python statements of the rules (py_matrices,
np_model, np_bq, np_cov), the messages against the library's full texts."""
import numpy as np
import pytest

from tests import cov_util as CU
from tests import model_util as MU
from tests import score_util as SU

pytestmark = pytest.mark.gpu

SESSIONS = ('score', 'model', 'bq', 'cov')
LABEL = {'score': 'scoring', 'model': 'read model', 'bq': 'bq', 'cov': 'gc-cov'}
BEGIN_FIRST = {'score': 'call mh_score_begin first', 'model': "call the session's begin first",
               'bq': "call the session's begin first", 'cov': 'call mh_cov_begin first'}
SPILLED = {s: 'the record store has spilled to the host (mh_bam_set_capacity): ' +
           ('score its BAM file' if s == 'score' else 'use its BAM file') for s in SESSIONS}
STATE = 'libmitty_hip error -7: '   # MH_E_STATE through the Python facade
TID = "tid outside the header's references"
NO_FIT = 'fields do not fit the record'
QNAME = 'S1:0:0:1|1|0|0|1000|100|100=|'
COV_LENGTHS = [400, 300, 200]
BLOCK_LEN = 16


@pytest.fixture(scope='module')
def native():
  from mitty_amd import _native
  if _native.device_count() == 0:
    pytest.fail('no HIP device: GPU tests must run on an MI355X')
  return _native


@pytest.fixture(scope='module')
def ctx(native):
  c = native.Context(0)
  yield c
  c.close()


def _cov_tuples(n, seed):
  """(flag, tid, pos, cigar, qualities) on COV_LENGTHS: every class of both rules, no failing record."""
  rng = np.random.RandomState(seed)
  out = []
  for _ in range(n):
    tid = int(rng.randint(-1, 3))
    span = int(rng.choice([1, 2, 5, 60, 150]))
    cigar = ['{}M'.format(span), '1M{}N1M'.format(span), '2S1={}D1X'.format(span), '3S'][int(rng.randint(4))]
    flag = int(rng.choice([0, 0x10, 0x800, 0x400, 0x4, 0x100], p=[.4, .3, .1, .1, .05, .05]))
    q = rng.randint(0, 100, int(rng.randint(1, 70))).tolist()
    out.append((flag, tid, -1 if tid < 0 else int(rng.randint(COV_LENGTHS[tid])), cigar, q))
  return out


class Data:
  """300 good records per session, their expected results per prefix of 100, 200 and 300 records (computed once,
  never changed), and what each session needs to begin."""

  def __init__(self):
    sg, mg = SU.golden(), MU.golden()
    ct = _cov_tuples(300, 21)
    self.names = [s['SN'] for s in sg['sq']]
    self.recs = {'score': sg['recs'][:300], 'model': mg['recs'][:300], 'cov': [CU.record(*t) for t in ct]}
    self.recs['bq'] = self.recs['cov']
    assert all(len(r) == 300 for r in self.recs.values())
    self.want = {}
    for n in (0, 100, 200, 300):
      self.want['score', n] = SU.py_matrices(sg['records'][:n])
      self.want['model', n] = MU.np_model(mg['tuples'][:n], 26)
      self.want['bq', n] = CU.np_bq(ct[:n], 3)
      self.want['cov', n] = CU.np_cov(ct[:n], COV_LENGTHS, BLOCK_LEN)

  def begin(self, c, s):
    if s == 'score':
      c.score_begin(self.names)
    elif s == 'model':
      c.model_begin(26)
    elif s == 'bq':
      c.bq_begin(3)
    else:
      c.cov_begin(COV_LENGTHS, BLOCK_LEN)

  def add(self, c, s, recs):
    getattr(c, s + '_add_records')(b''.join(recs), SU.offsets(recs))

  def check(self, c, s, n, what):
    """The session's result against the rule over its first n good records."""
    want = self.want[s, n]
    what = '{} {}'.format(s, what)
    if s == 'score':
      mq, dv, cnt = c.score_result()
      assert np.array_equal(mq, want[0]) and np.array_equal(dv, want[1]) and cnt['seen'] == n, what
    elif s == 'model':
      bq, tl, cnt = c.model_result()
      assert np.array_equal(bq, want[0]) and np.array_equal(tl, want[1]) and cnt == want[2], what
    elif s == 'bq':
      for i, m in want[0].items():
        got, cnt = c.bq_result(i)
        assert np.array_equal(got, m) and {k: cnt[k] for k in want[1]} == want[1], (what, i)
    else:
      for i, w in want[0].items():
        got, cnt = c.cov_result(i)
        assert cnt == want[1], (what, i)
        for k in ('covered', 'span_sum', 'min_pos', 'max_end'):
          assert np.array_equal(got[k].astype(np.int64), w[k]), (what, i, k)

  def result(self, c, s):
    return c.cov_result(0) if s == 'cov' else c.bq_result(0) if s == 'bq' else getattr(c, s + '_result')()


@pytest.fixture(scope='module')
def data():
  return Data()


# what fails, per session: a record and the text of its failure
def _bad_records():
  m = MU.record
  no_parse = 'qname does not parse (readgenerate.parse_qname)'
  return {
    'score': [(SU.record('S1:0:0:1|1|0|x|1000|100|100=|', 0, 0, 999, 60), no_parse),   # strand is not a number
              (SU.record('no-bars-at-all', 0, 0, 999, 60), no_parse),
              (SU.record(QNAME, 0x83, 0, 999, 60), 'read2 record whose qname has one read group'),
              (SU.record(QNAME, 0, 0, 999, 100), 'MAPQ of 100 or more (mq_mat has 100 rows)'),
              (SU.record(QNAME, 0, 7, 999, 60), TID)],
    'model': [(m(0x43, 0, 60, 0, [30] * 301), 'read longer than max_bp'),
              (m(0x43, 0, 60, 0, [30] * 10 + [94]), 'base quality of max_bq or more (0xff: no qualities stored)'),
              (m(0x43, 0, 60, 0, [255] * 20), 'base quality of max_bq or more (0xff: no qualities stored)'),
              (m(0x43, 0, 60, 0, []), 'l_seq is 0 (no qualities)'),
              (m(0x43, 26, 60, 0, [30] * 10), TID)],
    'bq': [(CU.record(0, 0, 5, '3M', [30, 100, 30]), 'base quality of max_bq or more (0xff: no qualities stored)'),
           (CU.record(0, 0, 5, '501M', [30] * 501), 'read longer than max_bp'),
           (CU.record(0, 3, 5, '10M', [30] * 10), TID)],
    'cov': [(CU.record(0, 1, 300, '10M', [30] * 10), 'pos outside its reference'),
            (CU.record(0, 3, 5, '10M', [30] * 10), TID)],
  }


def _import_records(native, c, recs):
  """Records into the context's store as a packed piece (mh_bam_import): no host check looks at them."""
  blob = b''.join(recs)
  o_roff, o_key, _, total = native.bam_piece_layout(len(recs), len(blob))
  piece = np.zeros(total, np.uint8)
  piece[:len(blob)] = np.frombuffer(blob, np.uint8)
  piece[o_roff:o_key] = SU.offsets(recs).view(np.uint8)
  c.bam_import(len(recs), len(blob), piece.ctypes.data)


def test_failure_texts(native, ctx, data):
  for s, cases in _bad_records().items():
    good = data.recs[s][:100]
    for rec, text in cases:
      data.begin(ctx, s)
      data.add(ctx, s, good)
      data.add(ctx, s, good[:50] + [rec] + good[50:])
      data.add(ctx, s, good)
      with pytest.raises(ValueError) as e:   # 100 good ones, then the 51st of the second call
        data.result(ctx, s)
      assert str(e.value) == '{}: record 150: {}'.format(LABEL[s], text), s
  # a record too short for its fixed fields reaches the device only through the store; the index counts on from the
  # session's earlier records
  short = b'\x10\0\0\0' + bytes(16)
  c = native.Context(0)
  try:
    c.bam_set_refs(['a', 'b', 'c'], COV_LENGTHS)
    _import_records(native, c, [short] + data.recs['cov'][:60])
    for s in SESSIONS:
      data.begin(c, s)
      data.add(c, s, data.recs[s][:100])
      getattr(c, s + '_add_store')()
      with pytest.raises(ValueError) as e:
        data.result(c, s)
      assert str(e.value) == '{}: record 100: {}'.format(
        LABEL[s], 'record shorter than its fixed fields' if s == 'score' else NO_FIT), s
  finally:
    c.close()


def _raw_result(native, c, s):
  """(status, message) of the session's result call on the C ABI, with no output buffers."""
  L = native.lib()
  rc = {'score': lambda: L.mh_score_result(c._h, None, None, None),
        'model': lambda: L.mh_model_result(c._h, None, None, None),
        'bq': lambda: L.mh_bq_result(c._h, 0, None, None),
        'cov': lambda: L.mh_cov_result(c._h, 0, None, None, None, None, None, None, 0, None)}[s]()
  return rc, L.mh_last_error(c._h).decode()


def test_state_errors(native, data):
  c = native.Context(0)
  try:
    for s in SESSIONS:   # nothing begun
      for call in (lambda: data.add(c, s, data.recs[s][:3]), getattr(c, s + '_add_store'), getattr(c, s + '_reset')):
        with pytest.raises(native.NativeError) as e:
          call()
        assert str(e.value) == STATE + BEGIN_FIRST[s], s
      assert _raw_result(native, c, s) == (-7, BEGIN_FIRST[s]), s
    for s in SESSIONS:   # begun, but the store has no references
      data.begin(c, s)
      with pytest.raises(native.NativeError) as e:
        getattr(c, s + '_add_store')()
      assert str(e.value) == STATE + 'call mh_bam_set_refs first', s
    # gc-cov compares the store's references with its own
    for names, lengths, text in ((['a', 'b'], COV_LENGTHS[:2], "the store's references are not the session's"),
                                 (['a', 'b', 'c'], [400, 301, 200],
                                  "the store's reference lengths are not the session's")):
      c.bam_reset()
      c.bam_set_refs(names, lengths)
      with pytest.raises(native.NativeError) as e:
        c.cov_add_store()
      assert str(e.value) == STATE + text
    # a store whose first records have left HBM
    c.bam_reset()
    c.bam_set_refs(['a', 'b', 'c'], COV_LENGTHS)
    _import_records(native, c, data.recs['cov'][:50])
    c.bam_set_capacity(1)
    _import_records(native, c, data.recs['cov'][50:100])
    assert c.bam_spilled()[0] > 0
    for s in SESSIONS:
      with pytest.raises(native.NativeError) as e:
        getattr(c, s + '_add_store')()
      assert str(e.value) == STATE + SPILLED[s], s
      data.check(c, s, 0, 'after the refused calls')   # nothing was added, the sessions are usable
  finally:
    c.close()


def test_four_sessions_side_by_side(native, data):
  bad = {s: cases[0] for s, cases in _bad_records().items()}
  c = native.Context(0)
  try:
    for failing in (None,) + SESSIONS:
      for s in SESSIONS:
        data.begin(c, s)
      for k in range(3):
        for s in SESSIONS:
          part = data.recs[s][100 * k:100 * k + 100]
          if s == failing and k == 1:
            part = part[:30] + [bad[s][0]] + part[30:]
          data.add(c, s, part)
      for s in SESSIONS:
        if s == failing:
          with pytest.raises(ValueError) as e:
            data.result(c, s)
          assert str(e.value) == '{}: record 130: {}'.format(LABEL[s], bad[s][1]), s
        else:
          data.check(c, s, 300, 'beside a failing {}'.format(failing))
  finally:
    c.close()


def test_results_repeat_and_sessions_continue(ctx, data):
  for s in ('score', 'model'):
    data.begin(ctx, s)
    data.add(ctx, s, data.recs[s][:100])
    data.check(ctx, s, 100, 'first result')
    data.check(ctx, s, 100, 'the result read again')
    data.add(ctx, s, data.recs[s][100:200])      # after a result: shows up in the next one
    data.check(ctx, s, 200, 'more records after a result')
    getattr(ctx, s + '_reset')()
    data.check(ctx, s, 0, 'after reset')
    data.add(ctx, s, data.recs[s][:100])
    data.check(ctx, s, 100, 'records after reset')
  assert data.want['model', 0][2]['min_rlen'] is None and data.want['model', 100][2]['used'] > 0
