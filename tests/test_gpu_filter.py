"""GPU tests of filter-bam (mh_filter.hip): the kept records, the counts and the output file against the test-side rule
(tests/filter_ref.py) and the reference's golden MQ matrices; the file's independence of how the input is chunked;
edge shapes, BGZF block edges, record sizes, the predicates and the error returns.  Every comparison is exact byte or
integer equality."""
import os

import numpy as np
import pytest

from tests import filter_ref as FR
from tests import score_util as SU

pytestmark = pytest.mark.gpu

BLOCK = 0xff00
SQ = [{'SN': '1', 'LN': 50000}, {'SN': '2', 'LN': 20000}]
TID = {'1': 0, '2': 1, None: -1, '9': 7}   # '9': a tid past the names
TEXT = '@HD\tVN:1.4\tSO:unsorted\n@SQ\tSN:1\tLN:50000\n@SQ\tSN:2\tLN:20000\n'
CL = 'filter-bam test'


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
def golden_bam(tmp_path_factory):
  """The golden aligned reads as a BAM file; 3000-byte BGZF blocks, so records straddle them."""
  g = SU.golden()
  path = str(tmp_path_factory.mktemp('filter') / 'golden.bam')
  with open(path, 'wb') as fp:
    fp.write(SU.bgzf_bytes(SU.bam_bytes(g['recs'], g['sq']), block=3000))
  return path


def _read(path):
  with open(path, 'rb') as fp:
    return fp.read()


# ---- records with a known verdict -------------------------------------------------------------------------------------
def mk(q, flag, ref, pos, mapq, seq='ACGT'):
  """(the tuple filter_ref judges, the BAM record)"""
  return (q, flag, ref, pos, mapq), SU.record(q, flag, TID[ref], pos, mapq, seq=seq)


def qn(p, pad=0, sample='a'):
  """A one-group qname of a read from chrom 1, position p, padded to any length."""
  return '{}{}:0|1|0|0|{}|4|4=|'.format(sample, 'x' * pad, p)


def wrong(i, pad=0, mapq=60, seq='ACGT'):
  """Placed 3 bases off (d_err 3): kept by default."""
  return mk(qn(100 + i, pad), 0, '1', 100 + i - 1 + 3, mapq, seq)


def right(i, pad=0, mapq=60):
  """Placed where it came from (d_err 0): dropped by default."""
  return mk(qn(100 + i, pad), 0, '1', 100 + i - 1, mapq)


def layout(header_len, kept_bytes):
  """The inflated sizes of the output's BGZF members: the header in its own block(s), then the kept stream cut at
  multiples of 0xff00."""
  cut = lambda n: [BLOCK] * (n // BLOCK) + ([n % BLOCK] if n % BLOCK else [])
  return cut(header_len) + cut(kept_bytes)


def run(ctx, path, calls, text=TEXT, sq=SQ, **rule):
  """The record lists of `calls`, one add_records each, through a filter session; its counts."""
  ctx.filter_begin([s['SN'] for s in sq], [s['LN'] for s in sq], text, path, **rule)
  for recs in calls:
    ctx.filter_add_records(b''.join(recs), SU.offsets(recs))
  return ctx.filter_finish()


def check_file(native, path, want_recs, text=TEXT, sq=SQ):
  data = _read(path)
  got_text, refs, recs = FR.split_bam(data)
  assert got_text == text and refs == [(s['SN'], s['LN']) for s in sq]
  assert len(recs) == len(want_recs)
  assert recs == want_recs
  header_len = len(SU.bam_bytes([], sq, text=text))
  assert FR.member_sizes(data) == layout(header_len, sum(len(r) for r in want_recs))
  bam = native.BamFile(path)   # the project's own reader takes it
  try:
    assert bam.text == text and bam.names == [s['SN'] for s in sq] and bam.lengths == [s['LN'] for s in sq]
    assert b''.join(c[0] for c in bam.chunks()) == b''.join(want_recs)
  finally:
    bam.close()
  return data


def run_and_check(ctx, native, path, items, cuts=None, **rule):
  """items: (tuple, record) pairs; cuts: the sizes of the add calls (None: one call).  The file and the counts against
  filter_ref under the same rule."""
  tuples, recs = [t for t, _ in items], [r for _, r in items]
  calls, o = [], 0
  for n in (cuts or [len(recs)]):
    calls.append(recs[o:o + n])
    o += n
  assert o == len(recs)
  counts = run(ctx, path, [c for c in calls if c] if cuts is None else calls, **rule)
  kw = dict(max_d=rule.get('max_d', 200), strict=rule.get('strict', False), sample=rule.get('sample_prefix'),
            min_derr=rule.get('d_lo', 1), max_derr=rule.get('d_hi'), min_mq=rule.get('mq_lo', 0),
            max_mq=rule.get('mq_hi', 255), unscored='keep' if rule.get('keep_unscored') else 'drop')
  kept, want = FR.verdicts(tuples, sizes=[len(r) for r in recs], known_refs={'1', '2'}, **kw)
  assert counts == want
  data = check_file(native, path, [recs[i] for i in kept])
  return kept, counts, data


# ---- 1. the golden BAM ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('strict', [0, 1])
@pytest.mark.parametrize('max_d', [200, 5])
def test_golden_bam(native, golden_bam, tmp_path, strict, max_d):
  from mitty_amd.benchmarking import filter_bam as fb, mq
  g = SU.golden()
  out = str(tmp_path / 'out.bam')
  counts = fb.filter_bam(golden_bam, out, max_d=max_d, strict=bool(strict), processes=3, command_line=CL)
  kept, want = FR.verdicts(g['records'], max_d=max_d, strict=bool(strict), sizes=[len(r) for r in g['recs']])
  assert counts == want
  text_in = '@HD\tVN:1.4\n'
  check_file(native, out, [g['recs'][i] for i in kept], text=fb.output_header_text(text_in, CL), sq=g['sq'])
  # the loop closed through the project's own reader and scorer: what is left is the matrix without its d_err = 0 column
  mat = SU.dense(g['mq']['s{}_d{}'.format(strict, max_d)], (100, 2 * max_d + 1))
  mat[:, max_d] = 0
  got = mq.process_bam(out, max_d=max_d, strict=bool(strict))
  assert got.dtype == np.uint64 and np.array_equal(got, mat)
  assert int(mat.sum()) == counts['kept']


# ---- 2. the file does not depend on chunking, threads or where the input is inflated ------------------------------------
@pytest.fixture(scope='module')
def golden_out(native, golden_bam, tmp_path_factory):
  from mitty_amd.benchmarking import filter_bam as fb
  out = str(tmp_path_factory.mktemp('filter_ref') / 'default.bam')
  fb.filter_bam(golden_bam, out, command_line=CL)
  data = _read(out)
  assert len(FR.member_sizes(data)) >= 4   # (several blocks, so chunk edges fall inside them)
  return data


@pytest.mark.parametrize('kw', [dict(chunk_bytes=20000), dict(processes=1), dict(processes=4), dict(gpu_inflate=True),
                                dict(chunk_bytes=20000, gpu_inflate=True, processes=3)],
                         ids=['chunk20000', 'threads1', 'threads4', 'gpu_inflate', 'all'])
def test_output_is_independent_of_chunks_threads_and_inflate(native, golden_bam, golden_out, tmp_path, kw):
  from mitty_amd.benchmarking import filter_bam as fb
  out = str(tmp_path / 'out.bam')
  fb.filter_bam(golden_bam, out, command_line=CL, **kw)
  assert _read(out) == golden_out


# ---- 3. shapes ------------------------------------------------------------------------------------------------------
def test_no_records(ctx, native, tmp_path):
  path = str(tmp_path / 'o.bam')
  counts = run(ctx, path, [])
  assert counts == dict.fromkeys(FR.COUNTS, 0)
  data = check_file(native, path, [])
  assert FR.member_sizes(data) == [len(SU.bam_bytes([], SQ, text=TEXT))]


@pytest.mark.parametrize('item', [wrong(0), right(0)], ids=['kept', 'dropped'])
def test_one_record(ctx, native, tmp_path, item):
  kept, counts, _ = run_and_check(ctx, native, str(tmp_path / 'o.bam'), [item])
  assert len(kept) == counts['kept'] == (1 if item[0][3] == 102 else 0)


@pytest.mark.parametrize('n', [255, 256, 257, 700])
def test_alternating_verdicts(ctx, native, tmp_path, n):
  items = [wrong(i, pad=i % 40) if i % 2 else right(i, pad=i % 7) for i in range(n)]
  kept, _, _ = run_and_check(ctx, native, str(tmp_path / 'o.bam'), items)
  assert kept == list(range(1, n, 2))


def test_first_300_dropped_then_all_kept(ctx, native, tmp_path):
  items = [right(i) for i in range(300)] + [wrong(i, pad=i % 11) for i in range(400)]
  kept, _, _ = run_and_check(ctx, native, str(tmp_path / 'o.bam'), items)
  assert kept == list(range(300, 700))


def test_all_kept_and_none_kept(ctx, native, tmp_path):
  items = [wrong(i, pad=i % 13) if i % 3 else right(i) for i in range(600)]
  kept, counts, _ = run_and_check(ctx, native, str(tmp_path / 'all.bam'), items, d_lo=0)
  assert len(kept) == 600 and counts['bytes_kept'] == counts['bytes_in']
  kept, counts, data = run_and_check(ctx, native, str(tmp_path / 'none.bam'), [right(i) for i in range(600)])
  assert kept == [] and counts['dropped_score'] == 600 and len(FR.member_sizes(data)) == 1


def test_every_call_a_single_record(ctx, native, tmp_path):
  items = [wrong(i, pad=i % 50) if i % 3 else right(i) for i in range(300)]
  _, _, one = run_and_check(ctx, native, str(tmp_path / 'one.bam'), items)
  _, _, each = run_and_check(ctx, native, str(tmp_path / 'each.bam'), items, cuts=[1] * 300)
  assert each == one


# ---- 4. block edges ---------------------------------------------------------------------------------------------------
def kept_totalling(total):
  """Kept records (padded qnames) whose bytes sum to exactly `total`, a dropped record behind every third."""
  base = len(wrong(0)[1])
  big = base + 150
  n = total // big - 1
  rest = total - n * big - 2 * base   # the last two records' padding
  assert n >= 1 and 0 <= rest <= 300
  pads = [150] * n + [rest // 2, rest - rest // 2]
  items, k = [], 0
  for i, p in enumerate(pads):
    items.append(wrong(i % 800, pad=p))   # (positions of 3 digits: every record's size is base + pad)
    k += len(items[-1][1])
    if i % 3 == 0:
      items.append(right(i % 800, pad=i % 100))
  assert k == total
  return items


@pytest.mark.parametrize('total', [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK])
def test_kept_bytes_at_block_edges(ctx, native, tmp_path, total):
  items = kept_totalling(total)
  _, counts, data = run_and_check(ctx, native, str(tmp_path / 'o.bam'), items)
  assert counts['bytes_kept'] == total
  assert FR.member_sizes(data)[1:] == {BLOCK - 1: [BLOCK - 1], BLOCK: [BLOCK], BLOCK + 1: [BLOCK, 1],
                                       2 * BLOCK: [BLOCK, BLOCK]}[total]


@pytest.mark.parametrize('carry', [0, 1, BLOCK - 1])
def test_chunk_boundary_leaves_a_given_carry(ctx, native, tmp_path, carry):
  first = kept_totalling(BLOCK + carry if carry != BLOCK - 1 else 2 * BLOCK - 1)
  second = [wrong(i, pad=i % 30) if i % 2 else right(i) for i in range(500)]
  kept1 = sum(len(r) for (t, r) in first if t[3] - int(t[0].split('|')[4]) == 2)
  assert kept1 % BLOCK == carry
  _, _, split = run_and_check(ctx, native, str(tmp_path / 'split.bam'), first + second, cuts=[len(first), len(second)])
  _, _, whole = run_and_check(ctx, native, str(tmp_path / 'whole.bam'), first + second)
  assert split == whole


# ---- 5. record sizes ------------------------------------------------------------------------------------------------
def test_long_qnames_among_short_ones(ctx, native, tmp_path):
  long_pad = 254 - len(qn(100))
  assert len(qn(100, long_pad)) == 254
  items = []
  for i in range(256):
    pad = long_pad if i % 5 == 0 else i % 9
    items.append(wrong(0, pad=pad) if i % 2 else right(0, pad=pad))
  items += [wrong(0, pad=long_pad), right(0, pad=long_pad)]
  kept, _, _ = run_and_check(ctx, native, str(tmp_path / 'o.bam'), items)
  assert len(kept) == 129


def test_one_record_of_more_than_100_kb(ctx, native, tmp_path):
  from mitty_amd.benchmarking import filter_bam as fb
  big_kept, big_dropped = wrong(7, seq='ACGT' * 20000), mk(qn(107), 0, '1', 106, 60, seq='ACGT' * 20000)
  assert len(big_kept[1]) > 100000
  items = ([wrong(i, pad=i % 20) if i % 2 else right(i) for i in range(90)] + [big_kept] +
           [wrong(i, pad=i % 20) if i % 3 else right(i) for i in range(90)] + [big_dropped] +
           [wrong(i) for i in range(40)])
  kept, counts, data = run_and_check(ctx, native, str(tmp_path / 'o.bam'), items)
  assert 90 in kept and 181 not in kept
  assert len(FR.member_sizes(data)) >= 3   # (the record spans several blocks)
  # the same records from a file, in chunks so small that the record is a chunk of its own
  src = str(tmp_path / 'in.bam')
  with open(src, 'wb') as fp:
    fp.write(SU.bgzf_bytes(SU.bam_bytes([r for _, r in items], SQ, text=TEXT), block=5000))
  out = str(tmp_path / 'o2.bam')
  got = fb.filter_bam(src, out, chunk_bytes=4000, command_line=CL)
  assert got == counts
  check_file(native, out, [items[i][1] for i in kept], text=fb.output_header_text(TEXT, CL))


# ---- 6. predicates --------------------------------------------------------------------------------------------------
def test_mapq_range_alone(ctx, native, tmp_path):
  mapqs = [0, 1, 29, 30, 31, 59, 60, 61, 99, 100, 101, 254, 255]
  items = [(wrong if i % 2 else right)(i, mapq=m) for i, m in enumerate(mapqs * 3)]
  for lo, hi in ((30, 60), (100, 255), (0, 255), (255, 255), (61, 99)):
    kept, counts, _ = run_and_check(ctx, native, str(tmp_path / 'o{}_{}.bam'.format(lo, hi)), items, d_lo=0,
                                    mq_lo=lo, mq_hi=hi)
    assert kept == [i for i, m in enumerate(mapqs * 3) if lo <= m <= hi]
    assert counts['dropped_score'] == 0 and counts['dropped_mapq'] == len(items) - len(kept)


def test_unscored_keep_and_drop(ctx, native, tmp_path):
  items = []
  for i in range(120):
    if i % 4 == 0:
      items.append(mk('not a qname at all', 0x4, None, -1, 0))          # unplaced, unparseable
    elif i % 4 == 1:
      items.append(mk(qn(100 + i, sample='b'), 0, '1', 100, 30))        # another sample
    elif i % 4 == 2:
      items.append(mk('b|junk', 0, '2', 5, 30))                         # another sample, unparseable
    else:
      items.append(wrong(i) if i % 8 == 3 else right(i))
  kept, counts, _ = run_and_check(ctx, native, str(tmp_path / 'drop.bam'), items, sample_prefix='a')
  assert kept == [i for i in range(120) if i % 8 == 3]
  assert counts['skipped_unplaced'] == 30 and counts['skipped_sample'] == 60
  kept, counts, _ = run_and_check(ctx, native, str(tmp_path / 'keep.bam'), items, sample_prefix='a', keep_unscored=True)
  assert kept == [i for i in range(120) if i % 4 != 3 or i % 8 == 3]
  assert counts['skipped_unplaced'] == 30 and counts['skipped_sample'] == 60 and counts['kept'] == 105


def test_only_wrong_chromosome_or_far(ctx, native, tmp_path):
  items = []
  for i in range(200):
    p = 1000 + i
    items.append([mk(qn(p), 0, '1', p - 1, 60),            # d_err 0
                  mk(qn(p), 0, '1', p - 1 + 49, 60),       # 49: inside max_d
                  mk(qn(p), 0, '1', p - 1 + 50, 60),       # 50: max_d
                  mk(qn(p), 0, '1', p - 1 - 700, 60),      # far: max_d
                  mk(qn(p), 0, '2', p - 1, 60)][i % 5])    # another chromosome: max_d
  kept, _, _ = run_and_check(ctx, native, str(tmp_path / 'o.bam'), items, max_d=50, d_lo=50, d_hi=50)
  assert kept == [i for i in range(200) if i % 5 >= 2]
  kept, _, _ = run_and_check(ctx, native, str(tmp_path / 's.bam'), items, max_d=50, d_lo=50, d_hi=50, strict=True)
  assert kept == [i for i in range(200) if i % 5 >= 2]


# ---- 7. errors ------------------------------------------------------------------------------------------------------
BAD = {'parse': mk('a:0|1|x', 0, '1', 5, 60),
       'mate': mk(qn(100), 0x80, '1', 99, 60),
       'tid': mk(qn(100), 0, '9', 99, 60)}


@pytest.mark.parametrize('what', sorted(BAD))
def test_a_failing_record_fails_the_session_and_removes_the_file(ctx, native, tmp_path, what):
  good = [wrong(i, pad=i % 17) if i % 2 else right(i) for i in range(300)]
  items = good[:150] + [BAD[what]] + good[150:299]
  recs = [r for _, r in items]
  with pytest.raises(FR.RecordError) as e:
    FR.verdicts([t for t, _ in items], known_refs={'1', '2'})
  assert e.value.index == 150
  path = str(tmp_path / 'o.bam')
  ctx.filter_begin([s['SN'] for s in SQ], [s['LN'] for s in SQ], TEXT, path)
  assert os.path.exists(path)
  for k in range(3):
    ctx.filter_add_records(b''.join(recs[100 * k:100 * k + 100]), SU.offsets(recs[100 * k:100 * k + 100]))
  with pytest.raises(ValueError) as e:
    ctx.filter_finish()
  assert 'filtering: record 150: ' in str(e.value)
  assert not os.path.exists(path)
  # the context goes on: the good records, through the same context
  kept, _, _ = run_and_check(ctx, native, path, good, cuts=[100, 100, 100])
  assert kept == list(range(1, 300, 2))


@pytest.mark.parametrize('rule', [dict(d_lo=-1), dict(d_lo=5, d_hi=4), dict(max_d=10, d_hi=11), dict(max_d=-1),
                                  dict(max_d=(1 << 20) + 1), dict(mq_lo=-1), dict(mq_hi=256), dict(mq_lo=9, mq_hi=8)])
def test_bad_ranges_at_begin_create_no_file(ctx, tmp_path, rule):
  path = str(tmp_path / 'o.bam')
  with pytest.raises(ValueError):
    ctx.filter_begin([s['SN'] for s in SQ], [s['LN'] for s in SQ], TEXT, path, **rule)
  assert not os.path.exists(path)


def test_abort_removes_the_file_and_a_path_that_cannot_be_made_is_an_oserror(ctx, native, tmp_path):
  path = str(tmp_path / 'o.bam')
  recs = [wrong(i)[1] for i in range(50)]
  ctx.filter_begin([s['SN'] for s in SQ], [s['LN'] for s in SQ], TEXT, path)
  ctx.filter_add_records(b''.join(recs), SU.offsets(recs))
  ctx.filter_abort()
  assert not os.path.exists(path)
  with pytest.raises(OSError) as e:
    ctx.filter_begin([s['SN'] for s in SQ], [s['LN'] for s in SQ], TEXT, str(tmp_path / 'no' / 'such' / 'o.bam'))
  assert 'o.bam' in str(e.value)
  if os.path.exists('/dev/full'):   # every write fails there; it is no regular file, so it is not removed
    with pytest.raises(OSError) as e:
      ctx.filter_begin([s['SN'] for s in SQ], [s['LN'] for s in SQ], TEXT, '/dev/full')
    assert '/dev/full' in str(e.value) and os.path.exists('/dev/full')
  with pytest.raises(native.NativeError) as e:   # no session: finish is a call out of order
    ctx.filter_finish()
  assert 'call mh_filter_begin first' in str(e.value)


# ---- 8. two device-BGZF files open on one context ---------------------------------------------------------------------
def test_a_bam_written_from_the_store_between_two_adds(native, tmp_path):
  """The filter's file and the god-aligner store's file (mh_bam_write_gpu) go through a sink each, on the same context
  and the same copy stream: the store is built and written between the session's second and third add.  Both files
  are byte-equal to what each operation writes alone on a fresh context."""
  from tests import bam_cases as C
  c = C.case('ties')
  header = '@HD\tVN:1.0\tSO:coordinate\n'
  recs = [(wrong(i, pad=i % 23) if i % 2 else right(i, pad=i % 5))[1] for i in range(300)]
  calls = [recs[0:100], recs[100:200], recs[200:300]]

  def store_bam(ctx, path):
    ctx.bam_set_refs(list(c.ref_names), list(c.ref_lengths))
    ctx.bam_add_fastq(c.fq1, c.fq2)
    ctx.bam_write_gpu(path, header, bai_path=path + '.bai')
    return _read(path), _read(path + '.bai')

  def filtered(ctx, path, between=None):
    ctx.filter_begin([s['SN'] for s in SQ], [s['LN'] for s in SQ], TEXT, path)
    for k, part in enumerate(calls):
      if k == 2 and between:
        between()
      ctx.filter_add_records(b''.join(part), SU.offsets(part))
    assert ctx.filter_finish()['kept'] == 150
    return _read(path)

  alone = []
  for what in (store_bam, filtered):
    fresh = native.Context(0)
    try:
      alone.append(what(fresh, str(tmp_path / 'alone_{}.bam'.format(len(alone)))))
    finally:
      fresh.close()
  both = native.Context(0)
  try:
    got = []
    data = filtered(both, str(tmp_path / 'f.bam'), lambda: got.append(store_bam(both, str(tmp_path / 's.bam'))))
  finally:
    both.close()
  assert got[0] == alone[0]
  assert data == alone[1]
  assert len(FR.split_bam(data)[2]) == 150 and len(alone[0][0]) > 28


# ---- 9. the command -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gpu_inflate', [False, True])
def test_cli(native, golden_bam, tmp_path, gpu_inflate):
  from click.testing import CliRunner
  from mitty_amd import cli
  g = SU.golden()
  out = str(tmp_path / 'out.bam')
  res = CliRunner().invoke(cli.cli, ['filter-bam', golden_bam, out, '--threads', '2'] +
                           (['--gpu-inflate'] if gpu_inflate else []))
  assert res.exit_code == 0, res.output
  kept, _ = FR.verdicts(g['records'])
  text, refs, recs = FR.split_bam(_read(out))
  assert recs == [g['recs'][i] for i in kept] and refs == [(s['SN'], s['LN']) for s in g['sq']]
  lines = text.split('\n')
  assert lines[0] == '@HD\tVN:1.4' and lines[1].startswith('@PG\tID:mitty-filter-bam\tPN:mitty\t') and lines[2:] == ['']
  assert golden_bam in lines[1] and out in lines[1]
