"""The device BAM encoder, coordinate sort, BAI plan and range partition (mitty_amd/csrc/mh_bam.hip; the host BAI
planner in mh_bgzf.cpp) against oracle/god.py on the adversarial inputs of tests/bam_cases.py — read lengths around
the 32-lane group and the 128 / 256-base passes on both strands, the whole sequence alphabet, CIGAR texts around the
32-byte ballot path, name lines around k_bam_parse's 192-byte LDS row, every reg2bin level and long spans over the
linear index, 1 to 3,366 references, 5,200-record ties.  test_bam_cases_cpu.py asserts that the inputs have those
shapes.  Every comparison is exact.

Each case is built three ways — one mh_bam_add_fastq call; the same bytes in several calls cut mid-record at places
that differ between the two files, continued from the returned used1 / used2; a store bounded by mh_bam_set_capacity
that spills to the host at least three times — and each way must give the oracle's sorted stream and raw BAI plan.
"""
import hashlib
import struct

import numpy as np
import pytest

from oracle import god
from tests import bam_cases as C

pytestmark = pytest.mark.gpu

HEADER = '@HD\tVN:1.0\tSO:coordinate\n'
MODES = ('one', 'cut', 'spill')


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


@pytest.fixture(scope='module')
def ctx2(native):
  """The receiving side of the partition test (a second store, as a rank's range store is)."""
  c = native.Context(0)
  yield c
  c.close()


# ---- the helper: build, compare ---------------------------------------------------------------------------------
def _templates(c):
  return c.fq1.count(b'\n') // 4


def _feed(ctx, c, rng, pieces, max_templates=-1):
  """The case's bytes in about `pieces` calls, each file cut at its own arbitrary byte; returns the calls made."""
  n1, n2 = len(c.fq1), len(c.fq2) if c.fq2 is not None else 0
  o1 = o2 = calls = 0
  grow = 1
  while o1 < n1:
    l1 = min(n1 - o1, grow * int(rng.randint(n1 // (2 * pieces), n1 // pieces + 2) + 1))
    l2 = min(n2 - o2, grow * int(rng.randint(n2 // (2 * pieces), n2 // pieces + 2) + 1))
    u1, u2, t = ctx.bam_add_fastq(c.fq1[o1:o1 + l1], None if c.fq2 is None else c.fq2[o2:o2 + l2], max_templates)
    calls += 1
    assert calls < 100 * pieces + 1000
    if t == 0:   # no whole template in the pieces: wider ones
      assert u1 == 0 and u2 == 0
      assert l1 < n1 - o1 or l2 < n2 - o2, 'the rest of the input holds no template'
      grow *= 2
      continue
    grow = 1
    assert c.fq1[o1 + u1 - 1:o1 + u1] == b'\n' and c.fq1[o1:o1 + u1].count(b'\n') == 4 * t
    if c.fq2 is not None:
      assert c.fq2[o2:o2 + u2].count(b'\n') == 4 * t
    o1, o2 = o1 + u1, o2 + u2
  assert o2 == n2
  return calls


def _build(ctx, name, c, e, mode):
  ctx.bam_set_capacity(0)
  ctx.bam_set_refs(list(c.ref_names), list(c.ref_lengths))
  rng = np.random.RandomState(len(c.fq1) % 9973 + MODES.index(mode))
  T = _templates(c)
  if mode == 'one':
    assert ctx.bam_add_fastq(c.fq1, c.fq2) == (len(c.fq1), len(c.fq2) if c.fq2 is not None else 0, T)
  elif mode == 'cut':
    assert _feed(ctx, c, rng, 7) >= min(T, 3)
  else:
    # every call after the first finds more resident bytes than the capacity allows and spills them first
    ctx.bam_set_capacity(max(1, len(e.stream) // 8))
    _feed(ctx, c, rng, 12, max_templates=max(1, T // 6))
    # (a case of fewer than four templates cannot spill three times: one call per template, all but the last spill)
    assert ctx.bam_spilled()[1] >= min(3, T - 1), ctx.bam_spilled()
  assert ctx.bam_records() == (len(e.recs), len(e.stream)), name


def _explain(got, e):
  """The first differing record and field of a sorted stream, both sides decoded."""
  p = 0
  for k, w in enumerate(e.encoded):
    if got[p:p + len(w)] != w:
      dw = god.decode(w)
      try:
        dg = god.decode(got[p:p + 4 + struct.unpack_from('<i', got, p)[0]])
      except Exception as ex:   # (not a record at all)
        return 'record {} ({}): not decodable ({!r}); want {}'.format(k, dw['qname'][:60], ex, dw)
      for f in dw:
        if dg.get(f) != dw[f]:
          return 'record {} of {}: field {}: got {!r}, want {!r} (want qname {}, pos {}, L {})'.format(
            k, len(e.encoded), f, dg.get(f), dw[f], dw['qname'][:80], dw['pos'], len(dw['seq']))
      gb, wb = got[p:p + len(w)], w
      d = next(i for i in range(len(w)) if gb[i:i + 1] != wb[i:i + 1])
      return 'record {}: byte {} of {}: got {!r}, want {!r}'.format(k, d, len(w), gb[d:d + 1], wb[d:d + 1])
    p += len(w)
  return 'no difference in {} records'.format(len(e.encoded))


def _check_stream(ctx, name, e, mode, digest=False):
  ctx.bam_sort()
  got = ctx.bam_sorted_head(len(e.stream))
  if digest:
    assert hashlib.sha256(got).digest() == hashlib.sha256(e.stream).digest(), (name, mode)
  elif got != e.stream:
    pytest.fail('{} [{}]: {}'.format(name, mode, _explain(got, e)))


def _check_plan(ctx, name, c, e, mode):
  runs, win, nwin = ctx.bam_bai_runs(len(c.ref_names))
  w_runs, w_win, w_nwin = C.bai_plan(c, e)
  what = '{} [{}]'.format(name, mode)
  assert runs.shape == w_runs.shape, what
  bad = np.flatnonzero((runs != w_runs).any(1))
  assert len(bad) == 0, '{}: run {}: got {}, want {}'.format(what, bad[0], runs[bad[0]], w_runs[bad[0]])
  assert len(win) == len(w_win), what
  bad = np.flatnonzero(win != w_win)
  assert len(bad) == 0, '{}: window {}: got {}, want {}'.format(what, bad[0], win[bad[0]], w_win[bad[0]])
  assert np.array_equal(nwin, w_nwin), what


def _check_files(ctx, name, c, e, tmp_path, digest=False):
  """mh_bam_write (host deflate, host BAI plan) and mh_bam_write_gpu (device deflate, device BAI plan unless it
  declines): both files decode to the oracle's records, each BAI equals the oracle's over that file's offsets."""
  sq = [{'SN': n, 'LN': ln} for n, ln in zip(c.ref_names, c.ref_lengths)]
  dec = None
  for how in ('host', 'gpu'):
    bam = str(tmp_path / '{}.bam'.format(how))
    if how == 'host':
      assert ctx.bam_write(bam, HEADER, level=1, threads=4, bai_path=bam + '.bai') == (len(e.recs), len(e.stream))
    else:
      assert ctx.bam_write_gpu(bam, HEADER, bai_path=bam + '.bai')[:2] == (len(e.recs), len(e.stream))
    header, recs, vo, vend = god.record_voffsets(open(bam, 'rb').read())
    assert header == god.header_bytes(HEADER, sq), (name, how)
    assert len(recs) == len(e.encoded), (name, how)
    if digest:
      assert hashlib.sha256(b''.join(recs)).digest() == hashlib.sha256(e.stream).digest(), (name, how)
    else:
      assert recs == e.encoded, (name, how)
    if dec is None:
      dec = [god.decode(r) for r in recs]   # (the same records in both files: decoded once)
    assert open(bam + '.bai', 'rb').read() == god.bai(len(sq), dec, vo, vend), (name, how)


@pytest.mark.parametrize('name', C.SMALL)
def test_case_vs_oracle(ctx, native, name, tmp_path):
  c, e = C.case(name), C.expected(name)
  decline = name == 'bins_past_ln'
  for mode in MODES:
    _build(ctx, name, c, e, mode)
    _check_stream(ctx, name, e, mode)
    if decline:   # a record past its reference's windows: no device plan (the host planner indexes the file)
      with pytest.raises(native.NativeError, match='BAI plan: records outside'):
        ctx.bam_bai_runs(len(c.ref_names))
    else:
      _check_plan(ctx, name, c, e, mode)
    if name in C.WRITTEN and mode in ('one', 'spill'):
      _check_files(ctx, name, c, e, tmp_path)
  ctx.bam_set_capacity(0)


def test_big_case_host_planner_joins_pieces(ctx, native, tmp_path):
  """132,000 records on one reference (the host BAI planner splits a reference of 131,072 or more records over
  threads and joins the pieces) and a record past the reference's end (the device plan declines, so the device-
  deflated file's BAI comes from the host planner too).  Records by digest, both BAIs exactly."""
  name = C.BIG[0]
  c, e = C.case(name), C.expected(name)
  on_big1 = sum(1 for r in e.recs if r['reference_id'] == 0)
  assert on_big1 >= 131072
  for mode in MODES:
    _build(ctx, name, c, e, mode)
    _check_stream(ctx, name, e, mode, digest=True)
    with pytest.raises(native.NativeError, match='BAI plan: records outside'):
      ctx.bam_bai_runs(2)
  _check_files(ctx, name, c, e, tmp_path, digest=True)
  ctx.bam_set_capacity(0)


# ---- ties through the partition ---------------------------------------------------------------------------------
def _splitters(n_dest):
  tid, pos, s = C.TIE
  K = tid << 33 | (pos + 1) << 1 | s           # occurs 5,200 times
  absent = tid << 33 | (pos + 50) << 1          # no record there
  above = (1 << 63) + 5                         # above every key
  if n_dest == 1:
    return []
  if n_dest == 2:
    return [K]
  if n_dest == 5:
    return [0, K, absent, above]
  rng = np.random.RandomState(n_dest)
  sp = [0, 0, 5, K - 2, K - 1, K, K, K + 1, K + 2, K + 3, K + 4, absent, absent, 1 << 40, above, above + 1]
  sp += [int(x) for x in rng.randint(0, 1 << 35, n_dest - 1 - len(sp))]
  return sorted(sp)


@pytest.mark.parametrize('n_dest', [1, 2, 5, 64])
def test_ties_survive_partition(ctx, ctx2, native, n_dest):
  """The store in three pieces, each partitioned by coordinate range (mh_bam_partition, tie = the record's global
  input index); every destination imports its segments in a shuffled order (mh_bam_import_tie) and sorts: the
  destinations' streams, concatenated, are the one-store stream — input order on equal keys.  Segment contents
  against NumPy."""
  c, e = C.case('ties'), C.expected('ties')
  ctx.bam_set_capacity(0)
  sp = _splitters(n_dest)
  assert len(sp) == n_dest - 1
  lines = c.fq1.split(b'\n')
  T = _templates(c)
  cuts = [0, T // 5, T // 2 + 1, T]
  rd = C.ref_dict(c)
  segs = [[] for _ in range(n_dest)]
  total = np.zeros(n_dest, np.int64)
  for p in range(3):
    piece = b'\n'.join(lines[4 * cuts[p]:4 * cuts[p + 1]]) + b'\n'
    recs = god.god_records(piece, None, rd)
    enc = [god.encode(r) for r in recs]
    keys = np.array([C.sort_key64(r) for r in recs], np.uint64)
    dest = np.searchsorted(np.array(sp, np.uint64), keys, side='right') if sp else np.zeros(len(keys), np.int64)
    size = np.array([len(x) for x in enc], np.int64)
    ctx.bam_set_refs(list(c.ref_names), list(c.ref_lengths))
    ctx.bam_add_fastq(piece)
    off, n, nb = ctx.bam_partition(sp, p << 32)
    assert np.array_equal(n, np.bincount(dest, minlength=n_dest)), (p, n)
    assert np.array_equal(nb, np.bincount(dest, weights=size, minlength=n_dest).astype(np.int64)), (p, nb)
    buf = np.zeros(max(int(off[-1]), 8), np.uint8)
    ctx.bam_partition_fetch(buf.ctypes.data, len(buf))
    for d in range(n_dest):
      o_roff, o_key, o_info, o_tie, tot = native.bam_part_layout(int(n[d]), int(nb[d]))
      assert off[d + 1] - off[d] == tot
      seg = buf[off[d]:off[d + 1]]
      mine = np.flatnonzero(dest == d)
      assert seg[:nb[d]].tobytes() == b''.join(enc[i] for i in mine), (p, d)
      assert np.array_equal(seg[o_roff:o_key].view(np.int64), np.concatenate([[0], np.cumsum(size[mine])])), (p, d)
      assert np.array_equal(seg[o_key:o_info].view(np.uint64), keys[mine]), (p, d)
      info = [(r['reference_id'], r['pos'], god.end_pos(r), god.reg2bin(r['pos'], god.end_pos(r)))
              for r in (recs[i] for i in mine)]
      assert np.array_equal(seg[o_info:o_tie].view(np.int32).reshape(-1, 4), np.array(info, np.int32).reshape(-1, 4))
      assert np.array_equal(seg[o_tie:tot].view(np.uint64), (np.uint64(p << 32) + mine.astype(np.uint64))), (p, d)
      segs[d].append((int(n[d]), int(nb[d]), seg.copy()))
      total[d] += n[d]
  assert total.sum() == len(e.recs) and (total == 0).sum() >= (2 if n_dest >= 5 else 0)
  rng = np.random.RandomState(7 + n_dest)
  out = []
  for d in range(n_dest):
    ctx2.bam_set_refs(list(c.ref_names), list(c.ref_lengths))   # (an empty store)
    for k in rng.permutation(3):
      n, nb, seg = segs[d][k]
      ctx2.bam_import_tie(n, nb, seg.ctypes.data)
    nrec, nbytes = ctx2.bam_records()
    assert nrec == total[d]
    if nrec:
      ctx2.bam_sort()
      out.append(ctx2.bam_sorted_head(nbytes))
  got = b''.join(out)
  if got != e.stream:
    pytest.fail('n_dest {}: {}'.format(n_dest, _explain(got, e)))


# ---- errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('place', C.ERROR_PLACES)
@pytest.mark.parametrize('kind', sorted(C.ERRORS))
def test_error(ctx, kind, place):
  """One bad template among 600 (first, last, template 300): the call raises with the documented message for that
  error alone, the store is unchanged, and good records added after it give the oracle's stream."""
  bad, good = C.error_case(kind, place)
  seed = C.case('templates_9_paired')
  ctx.bam_set_capacity(0)
  ctx.bam_set_refs(list(seed.ref_names), list(seed.ref_lengths))
  ctx.bam_add_fastq(seed.fq1, seed.fq2)
  before = ctx.bam_records()
  assert before[0] == 18
  with pytest.raises(ValueError) as ei:
    ctx.bam_add_fastq(bad.fq1, bad.fq2)
  msg = str(ei.value)
  assert 'god-aligner input: {};'.format(C.ERRORS[kind]) in msg and msg.count(';') == 1, msg
  assert ctx.bam_records() == before
  ctx.bam_add_fastq(good.fq1, good.fq2)
  both = C.Case(seed.fq1 + good.fq1, seed.fq2 + good.fq2, seed.ref_names, seed.ref_lengths)
  e = C.expected_of(both)
  assert ctx.bam_records() == (len(e.recs), len(e.stream))
  _check_stream(ctx, 'after {} {}'.format(kind, place), e, 'one')
