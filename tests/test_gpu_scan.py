"""Known-answer tests of the device scans (mh_scan.h) through mh_selftest_scan: the three-kernel device_scan /
device_reduce and the single-pass look-back device_scan_sum against NumPy prefix sums on int64, at the sizes where
the code changes path (a wave, a block, a tile, 64 / 65 look-back predecessors, the second round of the partials'
scan), at the top of the look-back words' value range, and across the states of the shared scratch buffer
(ctx->scan_partials: handed from one implementation to the other, grown, reused by a smaller launch, out of epochs).
Every comparison is exact array equality."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048                       # SCAN_TILE == LB_TILE
I64_MIN = np.iinfo(np.int64).min
LB_TOP = (1 << 46) - 1            # the largest total a look-back field may reach
LB_EPOCHS = (1 << 16) - 1         # the last epoch of a look-back scratch before it is zeroed again

SIZES_SMALL = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049,
               64 * TILE - 1, 64 * TILE, 64 * TILE + 1, 65 * TILE, 65 * TILE + 1, 66 * TILE + 1]
SIZES = SIZES_SMALL + [129 * TILE + 3, 256 * TILE, 256 * TILE + 1, 257 * TILE + 5, 4000017]


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


def _columns(rng, n):
  """(n, 3) int64, a distribution per column: all ones | uniform in [0, 1000) | 1 in 500 drawn from [0, 2^30)."""
  x = np.empty((n, 3), np.int64)
  x[:, 0] = 1
  x[:, 1] = rng.integers(0, 1000, n)
  x[:, 2] = np.where(rng.integers(0, 500, n) == 0, rng.integers(0, 1 << 30, n), 0)
  return x


@pytest.fixture(scope='module')
def base():
  """The inputs of the size sweep and their inclusive sums, computed once (read-only): a case of n elements uses
  the first n rows."""
  x = _columns(np.random.default_rng(20240607), max(SIZES))
  c = np.cumsum(x, axis=0, dtype=np.int64)
  x.setflags(write=False)
  c.setflags(write=False)
  return x, c


def _same(got, want, what):
  got = np.asarray(got).reshape(want.shape)
  assert got.dtype == np.int64, what
  if not np.array_equal(got, want):
    i = int(np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))[0])
    raise AssertionError('{}: first difference at element {} (tile {}): got {} want {}'.format(
      what, i, i // TILE, got[i], want[i]))


def _check(res, kind, want_incl, what):
  """res = Context.selftest_scan(...) against the inclusive prefix want_incl (n, fields)."""
  incl, excl, total, _ = res
  n, fields = want_incl.shape
  ident = I64_MIN if kind == 1 else 0
  want_total = want_incl[-1] if n else np.full(fields, ident, np.int64)
  _same(np.atleast_1d(total), want_total, what + ': total')
  if kind == 3:
    assert incl is None and excl is None
    return
  _same(incl, want_incl, what + ': inclusive')
  want_excl = np.empty_like(want_incl)
  want_excl[:1] = ident
  want_excl[1:] = want_incl[:-1]
  _same(excl, want_excl, what + ': exclusive')


def _run_check(ctx, kind, x, what, repeat=1, want_incl=None):
  """One checked call on x (n,) or (n, fields); returns (epoch, ticket base)."""
  x2 = x if x.ndim == 2 else x[:, None]
  if want_incl is None:
    want_incl = np.maximum.accumulate(x2, axis=0) if kind == 1 else np.cumsum(x2, axis=0, dtype=np.int64)
  res = ctx.selftest_scan(kind, x, repeat)
  _check(res, kind, want_incl, what)
  return res[3]


# (kind, columns of `base`): one field with each distribution, then the field-wise structs
SWEEP = ([(k, c) for k in (0, 2) for c in ((0,), (1,), (2,), (0, 1), (0, 1, 2))] +
         [(1, (1,)), (3, (1,)), (3, (0, 1, 2))])


@pytest.mark.parametrize('kind,cols', SWEEP, ids=['k{}-c{}'.format(k, ''.join(map(str, c))) for k, c in SWEEP])
def test_sizes_around_every_boundary(ctx, base, kind, cols):
  x, c = base
  for n in SIZES:
    xi = np.ascontiguousarray(x[:n, cols])
    want = np.ascontiguousarray(c[:n, cols]) if kind != 1 else None   # (the running maximum: computed per case)
    if len(cols) == 1 and n % 2:          # (the 1-d form of the binding as well)
      xi = xi[:, 0]
    _run_check(ctx, kind, xi, 'kind {} cols {} n {}'.format(kind, cols, n), want_incl=want)


def _max_inputs(rng, n):
  lo, hi = -(1 << 62), 1 << 62
  yield 'increasing', np.arange(n, dtype=np.int64) * 3 - n
  yield 'decreasing', n - np.arange(n, dtype=np.int64) * 3
  yield 'equal', np.full(n, -7, np.int64)
  neg = rng.integers(I64_MIN + 2, 0, n)
  if n:
    neg[0] = I64_MIN + 1
  yield 'negative', neg
  for name, at in (('max first', 0), ('max last', n - 1), ('max at a tile start', (n - 1) // TILE * TILE)):
    r = rng.integers(lo, hi, n)
    if n:
      r[at] = hi + 5
    yield name, r


def test_max_scan(ctx):
  rng = np.random.default_rng(7)
  for n in SIZES_SMALL:
    for name, x in _max_inputs(rng, n):
      _run_check(ctx, 1, x, 'max, {}, n {}'.format(name, n))


@pytest.mark.parametrize('fields', [1, 3])
def test_top_of_the_lookback_value_range(ctx, fields):
  rng = np.random.default_rng(46 + fields)
  for n in (1, 2049, 65 * TILE + 1):
    first = np.zeros((n, fields), np.int64)
    first[0] = LB_TOP
    last = np.zeros((n, fields), np.int64)
    last[-1] = LB_TOP
    spread = rng.integers(0, LB_TOP // n + 1, (n, fields))
    spread[rng.integers(0, n)] += LB_TOP - spread.sum(axis=0)
    assert (spread >= 0).all() and (spread.sum(axis=0) == LB_TOP).all()
    for name, x in (('first', first), ('last', last), ('spread', spread)):
      _run_check(ctx, 2, x, 'top of range, {}, fields {}, n {}'.format(name, fields, n))
    # beyond the contract: refused before any launch, and the next valid call is right
    over = last.copy()
    over[0, fields - 1] += 1           # (n == 1: the one element is 2^46)
    assert over[:, fields - 1].sum() == LB_TOP + 1
    with pytest.raises(ValueError):
      ctx.selftest_scan(2, over)
    _run_check(ctx, 2, spread, 'after a refused total, fields {}, n {}'.format(fields, n))
    negative = first.copy()
    negative[n // 2, 0] = -1
    with pytest.raises(ValueError):
      ctx.selftest_scan(2, negative)
    _run_check(ctx, 2, first, 'after a refused negative, fields {}, n {}'.format(fields, n))


class _LbModel:
  """The host's state of one look-back scratch buffer (LbScratchState, lb_reserve), as the calls should leave it."""

  def __init__(self):
    self.zeroed = None            # bytes zeroed; None: no state (new, or handed to device_scan / device_reduce)
    self.epoch = self.ticket = 0

  @staticmethod
  def need(n, fields):            # scan_lb_scratch_bytes
    return 64 + 2 * 8 * fields * max(1, -(-n // TILE)) + 64

  def call(self, kind, n, fields, repeat=1):
    """The (epoch, ticket base) the call's last launch reports, and whether the scratch started over."""
    if kind != 2:
      self.zeroed = None
      return (0, 0), False
    restarts = False
    for _ in range(repeat):
      if self.zeroed is None or self.zeroed < self.need(n, fields) or self.epoch >= LB_EPOCHS:
        self.zeroed, self.epoch, self.ticket = self.need(n, fields), 0, 0
        restarts = True
      base = self.ticket
      self.epoch += 1
      self.ticket += max(1, -(-n // TILE))
    return (self.epoch, base), restarts


def _shared_sequence():
  """[(kind, fields, n)]: a fixed opening that forces each hand-over of the buffer, then seeded random calls."""
  seq = [(2, 1, 5 * TILE), (0, 3, 3), (2, 3, 300 * TILE + 7),      # look-back after device_scan, grown
         (2, 1, 2049), (2, 3, 70 * TILE), (2, 2, 1),               # smaller after larger: the same epochs run on
         (2, 1, 129 * TILE + 3),                                   # more tiles than the last, no growth (1 field)
         (3, 3, 66 * TILE + 1), (2, 3, 2 * TILE + 11),             # look-back after device_reduce
         (2, 3, 65 * TILE + 1),                                    # larger after smaller: grows
         (1, 1, 64 * TILE + 1), (2, 2, 64 * TILE + 1), (0, 2, 257 * TILE + 5), (2, 2, 3)]
  rng = np.random.default_rng(4)
  sizes = [1, 3, 2049, 5 * TILE, 70 * TILE, 64 * TILE + 1, 129 * TILE + 3, 300 * TILE + 7, 65 * TILE, 2 * TILE + 11,
           513, 256 * TILE + 1]
  for _ in range(40):
    kind = int(rng.choice([0, 1, 2, 3], p=[0.15, 0.1, 0.6, 0.15]))
    fields = 1 if kind == 1 else int(rng.integers(1, 4))
    seq.append((kind, fields, int(rng.choice(sizes))))
  return seq


def test_shared_buffer_sequence(native):
  seq = _shared_sequence()
  assert len(seq) >= 40
  model = _LbModel()
  rng = np.random.default_rng(44)
  seen = set()
  c = native.Context(0)
  try:
    prev, prev_info, prev_need = None, None, 0
    for i, (kind, fields, n) in enumerate(seq):
      what = 'call {} (kind {}, fields {}, n {}; after {})'.format(i, kind, fields, n, prev)
      x = rng.integers(-(1 << 40), 1 << 40, n) if kind == 1 else rng.integers(0, 1000, (n, fields))
      info = _run_check(c, kind, x, what)
      want, restarts = model.call(kind, n, fields)
      assert info == want, what
      if kind == 2:
        # the epoch starts over exactly after a device_scan / device_reduce on the buffer or when the scratch had to
        # grow, and otherwise runs on (the ticket counter with it)
        need = model.need(n, fields)
        grows = prev is not None and prev[0] == 2 and need > prev_need
        assert restarts == (prev is None or prev[0] != 2 or grows), what
        if restarts:
          assert info == (1, 0), what
          prev_need = need
        else:
          assert info == (prev_info[0] + 1, prev_info[1] + max(1, -(-prev[2] // TILE))), what
        if prev is not None:
          seen.add({0: 'after scan', 1: 'after scan', 3: 'after reduce'}.get(prev[0]) or
                   ('larger' if n > prev[2] else 'smaller' if n < prev[2] else 'same') +
                   (', grown' if restarts else ', warm'))
        prev_info = info
      prev = (kind, fields, n)
  finally:
    c.close()
  assert {'after scan', 'after reduce', 'larger, grown', 'larger, warm', 'smaller, warm'} <= seen, seen


def test_epoch_exhaustion(native):
  """One scratch buffer through all 65535 epochs: lb_reserve must zero it again and restart the ticket counter, or
  the words the first launches left would pass for the new epoch 1 .. 4's."""
  n, fields = 3 * TILE + 11, 3
  tiles = 4
  rng = np.random.default_rng(65535)
  c = native.Context(0)
  try:
    e, base = _run_check(c, 2, rng.integers(0, 1000, (n, fields)), 'first call')
    assert (e, base) == (1, 0)
    # up to epoch 65533 in one call: 65533 - e launches back to back, the last one checked
    e2, base2 = _run_check(c, 2, rng.integers(0, 1000, (n, fields)), 'the launch of epoch 65533',
                           repeat=LB_EPOCHS - 2 - e)
    assert (e2, base2) == (LB_EPOCHS - 2, (LB_EPOCHS - 3) * tiles)
    seen = []
    for k in range(6):
      # fresh data per call, the same n: a word left from the first epochs 1 .. 4 holds another value
      seen.append(_run_check(c, 2, rng.integers(0, 1000, (n, fields)), 'call {} after epoch 65533'.format(k)))
    assert [s[0] for s in seen] == [65534, 65535, 1, 2, 3, 4]
    assert [s[1] for s in seen] == [65533 * tiles, 65534 * tiles, 0, tiles, 2 * tiles, 3 * tiles]
  finally:
    c.close()


@pytest.mark.parametrize('kind', [2, 0])
def test_repeated_launches_on_a_warm_scratch(ctx, kind):
  n = 129 * TILE + 3
  rng = np.random.default_rng(200 + kind)
  _run_check(ctx, kind, rng.integers(0, 1000, (n, 3)), 'kind {}, 200 launches'.format(kind), repeat=200)
  _run_check(ctx, kind, rng.integers(0, 1000, (n, 3)), 'kind {}, after 200 launches'.format(kind))


def test_two_contexts_at_once(native, base):
  x, c = base
  sizes = [1, 65, 2049, 5 * TILE + 1, 64 * TILE + 1, 65 * TILE, 70 * TILE, 3 * TILE + 11, 513, 66 * TILE + 1]
  cols_of = {1: (1,), 2: (1, 2), 3: (0, 1, 2)}
  errors = [[], []]

  def worker(t):
    rng = np.random.default_rng(1000 + t)
    try:
      cx = native.Context(0)
      try:
        for i in range(150):
          kind, cols, n = int(rng.choice([0, 2])), cols_of[int(rng.integers(1, 4))], int(rng.choice(sizes))
          lo = int(rng.integers(0, len(x) - n))           # (a window of the shared columns: fresh values per call)
          xi = np.ascontiguousarray(x[lo:lo + n, cols])
          try:
            _run_check(cx, kind, xi, 'thread {} call {} (kind {}, cols {}, n {})'.format(t, i, kind, cols, n))
          except (AssertionError, native.NativeError, ValueError) as err:
            errors[t].append(repr(err))
      finally:
        cx.close()
    except Exception as err:   # (reported by the assertion below, not lost with the thread)
      errors[t].append(repr(err))

  ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
  for t in ts:
    t.start()
  for t in ts:
    t.join()
  assert errors == [[], []], errors
