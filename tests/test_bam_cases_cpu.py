"""The inputs of test_gpu_bam.py have the shapes they are named for (tests/bam_cases.py), asserted from oracle/god.py
alone, so that no GPU test passes vacuously; and the oracle's own nt16 table is the one it states."""
import collections

import pytest

from oracle import god
from tests import bam_cases as C


def _file(r):
  return 2 if r.get('is_read2') else 1


def test_nt16_table_is_the_stated_one():
  """htslib's seq_nt16_table as the issue recalls it (stated from memory, DESIGN.md "Parity unpinned"): written out
  here a second time, by hand."""
  want = [15] * 256
  for c, v in (('=', 0), ('A', 1), ('C', 2), ('M', 3), ('G', 4), ('R', 5), ('S', 6), ('V', 7), ('T', 8), ('W', 9),
               ('Y', 10), ('H', 11), ('K', 12), ('D', 13), ('B', 14), ('N', 15)):
    want[ord(c)] = want[ord(c.lower())] = v
  want[ord('0')], want[ord('1')], want[ord('2')], want[ord('3')] = 1, 2, 4, 8
  assert want[ord('U')] == want[ord('u')] == 15 and want[ord('.')] == want[ord('*')] == want[ord('4')] == 15
  assert god._NT16 == want
  r = {'qname': 'q', 'reference_id': 0, 'pos': 0, 'cigarstring': '1M', 'mapq': 60, 'is_reverse': 0,
       'seq': bytes(range(256)).decode('latin-1'), 'qual': '!' * 256}
  assert god.encode(r)[36 + 2 + 4:36 + 2 + 4 + 128] == bytes(want[2 * i] << 4 | want[2 * i + 1] for i in range(128))


def test_nt16_sweep():
  c = C.case('nt16_sweep')
  every = set(range(256)) - {0x0a}
  for f, fq in ((1, c.fq1), (2, c.fq2)):
    lines = fq.split(b'\n')
    for s in (0, 1):
      seqs = [lines[i + 1] for i in range(0, len(lines) - 1, 4) if lines[i].split(b'|')[3 + 5 * (f - 1)] == b'%d' % s]
      assert len(seqs) >= 2 and all(set(x) == every and len(x) == 255 for x in seqs), (f, s)
  assert len(C.expected('nt16_sweep').recs) == 16


@pytest.mark.parametrize('name', ['read_lengths_paired', 'read_lengths_single'])
def test_read_lengths(name):
  recs = C.expected(name).recs
  have = collections.Counter((len(r['seq']), r['is_reverse'], _file(r)) for r in recs)
  files = (1, 2) if name.endswith('paired') else (1,)
  for L in C.READ_LENGTHS:
    for s in (0, 1):
      for f in files:
        assert have[(L, s, f)] >= 1, (L, s, f)
  for s in (0, 1):
    for f in files:
      seen = set().union(*(set(r['seq']) for r in recs if r['is_reverse'] == s and _file(r) == f))
      assert seen == set(C.SEQ_ALPHABET.decode()), (s, f)
      assert any(len(r['seq']) % 2 and set(C.SEQ_MUST.decode()) <= set(r['seq']) for r in recs
                 if r['is_reverse'] == s and _file(r) == f)
      quals = set().union(*(set(r['qual']) for r in recs if r['is_reverse'] == s and _file(r) == f))
      assert quals == set(C.QUAL_ALPHABET.decode()), (s, f)
  if name.endswith('single'):
    assert len(recs) % 2 == 1


def test_template_counts():
  seen = collections.defaultdict(set)
  for name in C.CASES:
    if name.startswith('templates_'):
      c = C.case(name)
      seen[c.fq2 is not None].add(len(C.expected(name).recs) // (2 if c.fq2 is not None else 1))
      assert c.fq1.count(b'\n') == 4 * int(name.split('_')[1])
  assert seen[True] | seen[False] == set(C.TEMPLATE_COUNTS)
  assert {1, 9, 65, 256} <= seen[True] and {1, 9, 65, 256} <= seen[False]


@pytest.mark.parametrize('name', ['names_paired', 'names_single'])
def test_names(name):
  c, e = C.case(name), C.expected(name)
  paired = c.fq2 is not None
  lens = collections.Counter(len(r['qname']) for r in e.recs)
  for n in C.NAME_LENGTHS + (C.shortest_name(paired),):
    assert lens[n] >= 1, n
  assert max(lens) == 254 and min(lens) == C.shortest_name(paired)
  # long by the rid and long by the v_lists, at each of the lengths
  for n in C.NAME_LENGTHS:
    rid_len = {len(r['qname'].split('|')[0]) for r in e.recs if len(r['qname']) == n}
    assert min(rid_len) < 8 and max(rid_len) > n - 60, (n, rid_len)
  spans = set(C.name_spans(c.fq1))
  for a in range(16):
    for s in C.SPANS:
      assert (a, s) in spans, (a, s)
  lines = c.fq1.split(b'\n')
  assert any(b' ' in ln for ln in lines[0::4]) and any(b'\t' in ln for ln in lines[0::4])
  assert all(' ' not in r['qname'] and '\t' not in r['qname'] for r in e.recs)
  # the last record: one base, and the last 16-byte chunk of its name line passes the end of the buffer
  assert len(lines[-4]) == 1 and len(lines[-2]) == 1
  s0 = len(c.fq1) - sum(len(x) + 1 for x in lines[-5:-1])
  c0, e0 = s0 & ~15, s0 + len(lines[-5])
  assert c.fq1[s0:s0 + 1] == b'@' and c0 + 16 * ((e0 - c0 + 15) >> 4) > len(c.fq1)


def test_cigars():
  recs = C.expected('cigars').recs
  have = collections.Counter((len(r['cigarstring']), r['is_reverse'], _file(r)) for r in recs)
  for n in C.CIGAR_LENGTHS:
    for s in (0, 1):
      for f in (1, 2):
        assert have[(n, s, f)] >= 1, (n, s, f)
  assert any(len(r['cigarstring']) > 64 for r in recs)
  ops = [god._cigar_ops(r['cigarstring']) for r in recs]
  assert {op for o in ops for _, op in o} == set(range(9))
  assert max(len(o) for o in ops) == 40
  digits = collections.Counter()
  for r in recs:
    num = ''
    for ch in r['cigarstring']:
      if ch.isdigit():
        num += ch
      else:
        digits[len(num)] += 1
        digits['zero' if num[0] == '0' and len(num) > 1 else 'plain'] += 1
        num = ''
  assert all(digits[d] >= 1 for d in range(1, 10)) and digits['zero'] >= 20
  assert max(n for o in ops for n, _ in o) == C.MAX_COUNT
  assert sum(1 for r in recs if god.end_pos(r) == r['pos'] + 1 and not any(op in (0, 2, 3, 7, 8) and n for n, op in
                                                                           god._cigar_ops(r['cigarstring']))) >= 10
  raw = [f for ln in C.case('cigars').fq1.split(b'\n')[0::4] for f in ln.decode().split('|')[6::5]]
  assert sum(1 for f in raw if f.startswith('>')) == len(C.CIGAR_INSERTS)
  assert any(f.startswith('>') and len(f.split(':')[0]) > 40 for f in raw)
  assert all(god.end_pos(r) < C.LN29 for r in recs)


@pytest.mark.parametrize('name', ['bins', 'bins_past_ln'])
def test_bins(name):
  c, e = C.case(name), C.expected(name)
  level = collections.Counter(C.bin_level(god.reg2bin(r['pos'], god.end_pos(r))) for r in e.recs)
  assert all(level[k] >= 20 for k in range(6)), level
  pos = {(r['reference_id'], r['pos']) for r in e.recs}
  ends = {(r['reference_id'], god.end_pos(r)) for r in e.recs}
  for t in (0, 1):
    assert (t, 0) in pos and (t, C.LN29 - 2) in pos
    for s in (14, 17, 20, 23, 26):
      B = 1 << s
      assert (t, B) in ends and (t, B + 1) in ends and (t, B) in pos, (t, s)
    wins = sorted({w for r in e.recs if r['reference_id'] == t
                   for w in range(r['pos'] >> 14, ((god.end_pos(r) - 1) >> 14) + 1)})
    assert max(b - a for a, b in zip(wins, wins[1:])) > 64   # megabases with no record between occupied windows
    spans = {((god.end_pos(r) - 1) >> 14) - (r['pos'] >> 14) + 1 for r in e.recs
             if r['reference_id'] == t and 'D' in r['cigarstring']}
    assert set(C.DELETION_WINDOWS) <= spans
    # a run of one start, then a shorter record with that start
    mine = [r for r in e.recs if r['reference_id'] == t]
    assert any(all(x['pos'] == mine[k]['pos'] for x in mine[k - 10:k]) and
               god.end_pos(mine[k]) < min(god.end_pos(x) for x in mine[k - 10:k]) for k in range(10, len(mine)))
  past = [r for r in e.recs if god.end_pos(r) > c.ref_lengths[r['reference_id']]]
  assert len(past) == (1 if name == 'bins_past_ln' else 0)
  # the device plan declines a record whose last window is not among the reference's (LN >> 14) + 1
  assert all((god.end_pos(r) - 1) >> 14 > C.LN29 >> 14 for r in past)


def test_bins_big():
  c = C.case('bins_past_ln_big')
  ids = [ln.split(b'|', 2)[1] for ln in c.fq1.split(b'\n')[0::4] if ln]
  n = collections.Counter(ids)
  assert 2 * n[b'big1'] >= 131072 + 2 * 300 and ids.count(b'big2') > 100
  assert c.fq1.count(b'|4M|') >= 65536


@pytest.mark.parametrize('n', C.N_REFS)
def test_references(n):
  c, e = C.case('refs_{}'.format(n)), C.expected('refs_{}'.format(n))
  assert len(c.ref_names) == n == len(set(c.ref_names))
  used = sorted({r['reference_id'] for r in e.recs})
  assert used == C.refs_used(n) and used[0] == 0 and used[-1] == n - 1
  if n > 2:
    assert len(used) < n and 2 not in used[:-1]
  if n >= 7:
    assert c.ref_names[:7] == C.REF_SPECIAL and len(c.ref_names[6]) == 60 and {0, 1, 3, 4, 5, 6} <= set(used)
    assert all(c.ref_names[t].startswith(c.ref_names[0]) for t in (1, 2)) and c.ref_names[4].startswith(c.ref_names[3])


def test_ties():
  e = C.expected('ties')
  key = collections.Counter((r['reference_id'], r['pos'], r['is_reverse']) for r in e.recs)
  tid, pos, s = C.TIE
  assert key[(tid, pos, s)] >= 5000
  assert key[(tid, pos, 1 - s)] > 1000 and key[(tid, pos - 1, 0)] + key[(tid, pos - 1, 1)] > 500
  assert key[(tid, pos + 1, 0)] + key[(tid, pos + 1, 1)] > 500
  assert len({r['qname'] for r in e.recs}) == len(e.recs)
  # the class is in input order in the sorted stream (the oracle's stable sort), others lie between them in the input
  cls = [int(r['qname'].split('|')[0][1:]) for r in e.recs if (r['reference_id'], r['pos'], r['is_reverse']) == C.TIE]
  assert cls == sorted(cls) and len(cls) == 5200


@pytest.mark.parametrize('kind', sorted(C.ERRORS))
def test_error_cases(kind):
  for place in C.ERROR_PLACES:
    bad, good = C.error_case(kind, place)
    n = good.fq1.count(b'\n') // 4
    assert bad.fq1.count(b'\n') == 4 * (n + 1) == bad.fq2.count(b'\n') and n == 599
    assert len(god.god_records(good.fq1, good.fq2, C.ref_dict(good))) == 2 * n
    # the bad template is where the case says, and it is the only difference
    l1, g1 = bad.fq1.split(b'\n'), good.fq1.split(b'\n')
    at = {'first': 0, 'last': n, 'middle': 300}[place]
    assert [x[0:1] for x in l1[:4 * at:4]] == [b'@'] * at
    if kind == 'name_255':
      assert len(l1[4 * at]) == 256
    if kind == 'name_1_byte':
      assert l1[4 * at] == b'@a'
