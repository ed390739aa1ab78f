"""Adversarial inputs of the god-aligner BAM path (mitty_amd/csrc/mh_bam.hip, the BAI planner in mh_bgzf.cpp): FASTQ
bytes with synthetic qnames in the reference grammar (readgenerate.parse_qname)

  rid|chrom|cpy|strand|pos|rlen|cigar|v_list|strand|pos|rlen|cigar|v_list

No GPU here.  Every case is a Case (fq1, fq2 or None, ref_names, ref_lengths); CASES names them, case(name) builds one
once and expected(name) runs oracle/god.py over it once (test_bam_cases_cpu.py asserts from that alone that each case
has the shape it is named for, test_gpu_bam.py compares the library with it).

Two things the grammar itself rules out, so no valid input can hold them; the error cases feed them instead:
* a 1-byte CIGAR text ('M' is an op before any digit, '5' a trailing number): valid texts are 2..40 bytes here;
* a 1-byte name (it has too few fields): the shortest name the grammar allows stands in.
"""
import collections
import functools

import numpy as np

from oracle import god

Case = collections.namedtuple('Case', 'fq1 fq2 ref_names ref_lengths')
Expected = collections.namedtuple('Expected', 'recs encoded stream soff')   # sorted records, their bytes, offsets

SEQ_ALPHABET = bytes(range(0x21, 0x7f))    # every printable ASCII byte: both cases of each IUPAC letter, U/u, = . * 0-9
QUAL_ALPHABET = bytes(range(0x21, 0x7f))   # '!'..'~'
SEQ_MUST = b'ACMGRSVTWYHKDBNacmgrsvtwyhkdbnUu=.*0123456789'
READ_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 301)
TEMPLATE_COUNTS = (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000)
NAME_LENGTHS = (126, 127, 128, 129, 130, 253, 254)
SPANS = tuple(range(176, 210))             # e0 - c0 of k_bam_parse's staged name line (its LDS row is 192 bytes)
CIGAR_LENGTHS = tuple(range(2, 41))
N_REFS = (1, 2, 3, 4, 7, 8, 1023, 1024, 3366)
LN29 = 1 << 29
SMALL_REFS = (('1', '2', '3'), (50000, 20000, 8000))
TIE = (1, 4999, 0)                         # (tid, pos, strand) of the tie class
DELETION_WINDOWS = (2, 3, 300, 5000)
BIG_TEMPLATES = 66000                      # 132,000 records on one reference: the host BAI planner joins pieces


class _Fastq:
  """A FASTQ (pair) under construction."""

  def __init__(self, paired, seed):
    self.rng = np.random.RandomState(seed)
    self.paired = paired
    self.recs = ([], [])   # per file: [name line, sequence, '+' line, qualities]
    self.len1 = 0          # bytes of file 1 so far

  def draw(self, n, alphabet):
    return np.frombuffer(alphabet, np.uint8)[self.rng.randint(0, len(alphabet), n)].tobytes()

  @staticmethod
  def qname(rid, chrom, reads, vlists=None, cpy=0):
    f = [rid, chrom, str(cpy)]
    for k, (strand, pos, cigar, rlen) in enumerate(reads):
      f += [str(strand), str(pos), str(rlen), cigar, vlists[k] if vlists else '']
    return '|'.join(f)

  def add(self, chrom, reads, rid=None, vlists=None, comment=b'', seqs=None, align=None, qname=None, lead=b'@'):
    """One template.  reads: (strand, pos as the qname holds it (1-based), cigar, read length) per file; align: the
    name line of file 1 starts at that offset modulo 16 (the previous record's '+' line is padded)."""
    assert len(reads) == (2 if self.paired else 1)
    if rid is None:
      rid = 'r{}'.format(len(self.recs[0]))
    qn = (self.qname(rid, chrom, reads, vlists) if qname is None else qname).encode()
    if align is not None:
      if not self.recs[0]:
        self.add(chrom, [(0, 1, '1M', 1)] * len(reads), rid='pad')
      pad = (align - self.len1) % 16
      self.recs[0][-1][2] += b'p' * pad
      self.len1 += pad
    for f, (_, _, _, rlen) in enumerate(reads):
      seq = seqs[f] if seqs is not None and seqs[f] is not None else self.draw(rlen, SEQ_ALPHABET)
      rec = [lead + qn + (comment if f == 0 else b''), seq, b'+', self.draw(len(seq), QUAL_ALPHABET)]
      self.recs[f].append(rec)
      if f == 0:
        self.len1 += sum(len(x) + 1 for x in rec)

  def case(self, ref_names, ref_lengths):
    fq = [b''.join(b'\n'.join(r) + b'\n' for r in recs) for recs in self.recs]
    assert len(fq[0]) == self.len1
    return Case(fq[0], fq[1] if self.paired else None, tuple(ref_names), tuple(ref_lengths))


def _strands(paired):
  return ((0, 0), (0, 1), (1, 0), (1, 1)) if paired else ((0,), (1,))


# ---- 1. read lengths ----------------------------------------------------------------------------------------------
def read_lengths(paired):
  """Every length of READ_LENGTHS on both strands in each file, the whole byte alphabet; single-end: an odd number
  of records (k_bam_write packs two records per wave)."""
  b = _Fastq(paired, 101 + paired)
  names, lens = SMALL_REFS
  for rep in range(2):
    for L in READ_LENGTHS:
      for st in _strands(paired):
        c = b.rng.randint(0, 3)
        b.add(names[c], [(s, b.rng.randint(1, lens[c] - 400), '{}M'.format(L), L) for s in st])
  for st in _strands(paired):   # the alphabet in order, and the bytes the issue names (odd length)
    b.add('1', [(s, 77, '94M', 94) for s in st], seqs=[SEQ_ALPHABET] * len(st))
    b.add('2', [(s, 78, '45M', len(SEQ_MUST)) for s in st], seqs=[SEQ_MUST] * len(st))
  if not paired and len(b.recs[0]) % 2 == 0:
    b.add('3', [(1, 5, '3M', 3)])
  return b.case(names, lens)


def nt16_sweep():
  """Every byte value but the line feed (which cannot lie inside a FASTQ line) as one 255-base sequence, ascending
  and descending, on each strand in each file: pins nt16() and the strand-1 complement."""
  b = _Fastq(True, 150)
  sweep = bytes(x for x in range(256) if x != 0x0a)
  for st in _strands(True):
    b.add('2', [(s, 100, '255M', 255) for s in st], seqs=[sweep, sweep[::-1]])
    b.add('3', [(s, 200, '255M', 255) for s in st], seqs=[sweep[::-1], sweep])
  return b.case(*SMALL_REFS)


# ---- 2. template counts -------------------------------------------------------------------------------------------
def template_count(T, paired):
  b = _Fastq(paired, 200 + 2 * T + paired)
  names, lens = SMALL_REFS
  for _ in range(T):
    c = b.rng.randint(0, 3)
    reads = []
    for _ in range(2 if paired else 1):
      L = b.rng.randint(1, 41)
      reads.append((b.rng.randint(0, 2), b.rng.randint(1, lens[c] - 100), '{}M'.format(L), L))
    b.add(names[c], reads)
  return b.case(names, lens)


# ---- 3. names -----------------------------------------------------------------------------------------------------
_VL = '1234567890I,D;XACGT-_.:'


def _named(b, n, k, by_vlist, comment=b'', align=None, rlen=None):
  """A template whose qname has exactly n bytes, long by its rid or by its v_lists."""
  nr = 2 if b.paired else 1
  c = k % 3
  reads = []
  for _ in range(nr):
    L = rlen if rlen is not None else b.rng.randint(1, 12)
    reads.append((b.rng.randint(0, 2), b.rng.randint(1, SMALL_REFS[1][c] - 100), '{}M'.format(L), L))
  rid = 'n{}'.format(k)
  base = len(_Fastq.qname(rid, SMALL_REFS[0][c], reads))
  assert base <= n, (base, n)
  fill = ''.join(_VL[(k + i) % len(_VL)] for i in range(n - base))
  if by_vlist:
    vl = [fill[:len(fill) // 2], fill[len(fill) // 2:]] if nr == 2 else [fill]
  else:
    rid, vl = rid + fill, None
  b.add(SMALL_REFS[0][c], reads, rid=rid, vlists=vl, comment=comment, align=align)
  assert len(b.recs[0][-1][0]) == 1 + n + len(comment)


def shortest_name(paired):
  return len(_Fastq.qname('a', '1', [(0, 1, '1M', 1)] * (2 if paired else 1)))


def names(paired):
  """Name lengths around k_bam_write's 128-byte second loop and at BAM's 254 limit, every staged span 176..209 of
  k_bam_parse at every start alignment, comments after a space and after a tab, and a last record of one base."""
  b = _Fastq(paired, 300 + paired)
  b.add('1', [(0, 1, '1M', 1)] * (2 if paired else 1), rid='a')   # the shortest name of the grammar
  k = 0
  for n in NAME_LENGTHS:
    for by_vlist in (False, True):
      for comment in (b'', b' a comment', b'\tafter a tab'):
        _named(b, n, k, by_vlist, comment)
        k += 1
  comments = (b'', b' c', b'\tcomment after a tab', b' two words')
  for a in range(16):
    for span in SPANS:
      comment = comments[(a + span) % 4]
      _named(b, span - a - 1 - len(comment), k, (a + span) % 2 == 1, comment, align=a)
      k += 1
  _named(b, 47, k, False, align=1, rlen=1)   # span 49: its last 16-byte chunk ends 8 bytes past the buffer
  return b.case(*SMALL_REFS)


def name_spans(fq1):
  """(start alignment, e0 - c0) of every name line of a FASTQ."""
  out, pos = [], 0
  for i, line in enumerate(fq1.split(b'\n')[:-1]):
    if i % 4 == 0:
      out.append((pos & 15, (pos & 15) + len(line)))
    pos += len(line) + 1
  return out


# ---- 4. CIGAR -----------------------------------------------------------------------------------------------------
_OPS = 'MIDNSHP=X'
_REF_OPS = 'MDN=X'
MAX_COUNT = 268435455   # 2^28 - 1: the largest op count a BAM CIGAR word holds


def gen_cigar(rng, n):
  """A valid CIGAR text of exactly n bytes: op counts of 1 to 9 digits (leading zeros included), reference-consuming
  ops kept short so the span stays inside a reference."""
  out, rem = '', n
  while rem:
    ok = [d for d in range(1, min(9, rem - 1) + 1) if rem - d - 1 != 1]
    d = ok[rng.randint(0, len(ok))]
    op = _OPS[rng.randint(0, 9)]
    v = int(rng.randint(0, 100000)) % 10 ** d if op in _REF_OPS else min(int(rng.randint(0, 10 ** 9)) % 10 ** d, MAX_COUNT)
    out += '{:0{}d}{}'.format(v, d, op)
    rem -= d + 1
  assert len(out) == n
  return out


CIGAR_SPECIALS = (
  ['5' + op for op in _OPS] + [str(MAX_COUNT)[:d] + 'M' for d in range(1, 10)] + [str(MAX_COUNT) + op for op in 'ISHP'] +
  ['0000000012M', '000M', '0I', '007S3M', '10S', '5I3S', '4H6P', '1I', '1M' * 40, '2=1X' * 20, '12M3I' * 8,
   '123456789H' * 8, '1M1I1D1N1S1H1P1=1X' * 4, '99999D'])
CIGAR_INSERTS = ('>12:34I', '>1:007I', '>123456789012345678901234567890:268435455I', '>0:1I',
                 '>99999999999999999999999999999999999999999999999999:12345678I')


def cigars():
  """Every CIGAR text length 2..40 on both strands in both files (k_bam_write packs texts of up to 32 bytes with a
  ballot and shuffles, longer ones serially), every op, counts of 1 to 9 digits up to 2^28 - 1, leading zeros, the
  '>p:nI' form, texts with no reference span, up to 40 ops in one text."""
  b = _Fastq(True, 400)
  refs = ('c1', 'c2')
  for rep in range(3):
    for n in CIGAR_LENGTHS:
      for s in (0, 1):
        b.add(refs[(n + rep) % 2], [(s, b.rng.randint(1, LN29 // 2), gen_cigar(b.rng, n), 4),
                                    (1 - s, b.rng.randint(1, LN29 // 2), gen_cigar(b.rng, n), 5)])
  for n in (41, 48, 63, 64, 65, 80):   # past the 32-lane group and past a wave
    b.add('c1', [(0, b.rng.randint(1, LN29 // 2), gen_cigar(b.rng, n), 3), (1, 7, gen_cigar(b.rng, n), 2)])
  for k, c in enumerate(CIGAR_SPECIALS + list(CIGAR_INSERTS)):
    b.add(refs[k % 2], [(k % 2, 1 + 1000 * k, c, 6), (1 - k % 2, 1, CIGAR_SPECIALS[-1 - k % 8], 7)])
  return b.case(refs, (LN29, LN29))


def cigar_text(cigarstring_field):
  return cigarstring_field.split(':')[-1] if cigarstring_field[0] == '>' else cigarstring_field


# ---- 5. bins and windows ------------------------------------------------------------------------------------------
def bin_level(b):
  return 0 if b == 0 else 1 if b < 9 else 2 if b < 73 else 3 if b < 585 else 4 if b < 4681 else 5


def _bin_sites(rng):
  """(pos, cigar) sites of one reference: every reg2bin level around every level boundary."""
  out = []
  for s in (14, 17, 20, 23, 26):
    B = 1 << s
    last = LN29 // B - 1
    for k in sorted({1, 2, 3, 5, 6, 7, last} & set(range(1, last + 1))):
      for ln in (1, 2, 100, 4097):
        op = 'M=XN'[(k + ln) % 4]
        out.append((k * B - ln, '{}{}'.format(ln, op)))       # ends exactly at the boundary
        out.append((k * B - ln + 1, '{}{}'.format(ln, op)))   # ends one past it (ln = 1: starts on it)
        out.append((k * B, '{}{}'.format(ln, op)))            # starts exactly on it
  out += [(0, '1M'), (0, '16384M'), (0, '16385M'), (LN29 - 2, '1M'), (LN29 - 2, '2M'), (LN29 - 1, '1M')]
  for i, W in enumerate(DELETION_WINDOWS):   # a deletion over W linear-index windows
    out.append(((2000 + 6000 * i) * 16384 + 100, '10M{}D10M'.format((W - 1) * 16384 + 30)))
  # runs of records with one start, long then short, then a neighbour (k_bai_mark's predecessor shortcut)
  p = 40000000
  for rep in range(3):
    out += [(p, '40000M')] * 12 + [(p, '10M')] + [(p + 5, '70000M'), (p + 5, '3M'), (p + 16384, '5M')]
    out += [(p + 200000, '9M300000N9M')] * 30 + [(p + 200000, '1M'), (p + 200001, '2000000N')]
    p += 1 << 22
  for _ in range(60):
    out.append((int(rng.randint(0, LN29 - 5000)), '{}M'.format(rng.randint(1, 5000))))
  return out


def bins(past_ln=False, big=False):
  """Two references of 2^29 bp: every bin level, spans ending at / one past / starting on every level boundary, the
  first and last positions, long deletions, heavy overlap, megabases with no record.  past_ln: one record ends past
  the reference (the device BAI plan declines, the host planner indexes it); big: 132,000 more four-base records on
  one reference, so the host planner works in pieces on threads and joins them."""
  b = _Fastq(True, 500)
  refs = ('big1', 'big2')
  for c in range(2):
    sites = _bin_sites(b.rng)
    if past_ln and c == 1:
      sites.append((LN29 - 2, '1M20000D'))
    if len(sites) % 2:
      sites.append((12345, '6M'))
    order = b.rng.permutation(len(sites))
    for i in range(0, len(order), 2):
      b.add(refs[c], [(b.rng.randint(0, 2), sites[j][0] + 1, sites[j][1], 4) for j in order[i:i + 2]])
  if big:
    for i in range(BIG_TEMPLATES):
      b.add('big1', [(i & 1, 1 + (i * 7919) % 3000000, '4M', 4), ((i >> 1) & 1, 1 + (i * 104729) % 3000000, '4M', 4)],
            rid='b{}'.format(i))
  return b.case(refs, (LN29, LN29))


# ---- 6. references ------------------------------------------------------------------------------------------------
REF_SPECIAL = ('1', '10', '1_', 'chr1', 'chr10', 'chr1_alt', 'chrUn_' + 'KI270442v1_' * 4 + '0123456789')
assert len(REF_SPECIAL[-1]) == 60


def ref_names(n):
  return tuple(REF_SPECIAL[:n]) + tuple('chr1{}'.format(i) for i in range(len(REF_SPECIAL), n))


def refs_used(n):
  """tid 0, the last, a few between (the names that are prefixes of each other among them); tid 2 and, from 8
  references on, most of the others stay empty."""
  if n == 3:
    return [0, 2]
  return sorted({0, n - 1} | {t for t in (1, 3, 4, 5, 6, n // 3, n // 2) if 0 < t < n - 1 and t != 2})


def references(n):
  """n references (the sort's end bit follows n), names that are prefixes of each other, a 60-byte name."""
  b = _Fastq(True, 600 + n)
  nm = ref_names(n)
  lens = tuple(100000 + 1000 * (i % 7) for i in range(n))
  for _ in range(30):
    for t in refs_used(n):
      reads = []
      for _ in range(2):
        L = b.rng.randint(1, 10)
        reads.append((b.rng.randint(0, 2), b.rng.randint(1, lens[t] - 100), '{}M'.format(L), L))
      b.add(nm[t], reads)
  return b.case(nm, lens)


# ---- 7. ties ------------------------------------------------------------------------------------------------------
def ties():
  """5,200 single-end records with one (tid, pos, strand), each with its own name; records of the other strand and
  one base either side interleaved."""
  b = _Fastq(False, 700)
  tid, pos, strand = TIE
  nm = ('1', '2')

  def one(rid, s, p):
    L = b.rng.randint(1, 7)
    b.add(nm[tid], [(s, p + 1, '{}M'.format(L), L)], rid=rid)
  for i in range(5200):
    one('t{}'.format(i), strand, pos)
    if i % 3 == 0:
      one('s{}'.format(i), 1 - strand, pos)
    if i % 5 == 0:
      one('l{}'.format(i), b.rng.randint(0, 2), pos - 1)
    if i % 7 == 0:
      one('h{}'.format(i), b.rng.randint(0, 2), pos + 1)
    if i % 97 == 0:
      one('o{}'.format(i), 0, 10 + i)
      b.add('1', [(1, 30 + i, '2M', 2)], rid='z{}'.format(i))
  return b.case(nm, (100000, 100000))


def sort_key64(r):
  """The device sort key of a record (tid << 33 | (pos + 1) << 1 | strand)."""
  return r['reference_id'] << 33 | (r['pos'] + 1) << 1 | int(r['is_reverse'])


# ---- 8. errors ----------------------------------------------------------------------------------------------------
E_RECORD = 'malformed FASTQ record'
E_NAME = 'read name longer than 254 characters (BAM limit)'
E_CHROM = 'qname chrom not among the @SQ names (.ann)'
E_FIELDS = 'qname does not parse (readgenerate.parse_qname)'
E_CIGAR = 'invalid CIGAR in qname'
E_SEQ = 'quality and sequence mismatch (sequence and quality lengths differ)'
ERRORS = {   # kind -> the message mh_bam_add_fastq documents
  'name_255': E_NAME, 'chrom_unknown': E_CHROM, 'fields_too_few': E_FIELDS, 'name_1_byte': E_FIELDS,
  'strand_not_numeric': E_FIELDS, 'pos_not_numeric': E_FIELDS, 'cigar_op_first': E_CIGAR, 'cigar_op_only': E_CIGAR,
  'cigar_trailing_number': E_CIGAR, 'cigar_number_only': E_CIGAR, 'cigar_unknown_letter': E_CIGAR,
  'seq_qual_file2': E_SEQ, 'no_at': E_RECORD}
ERROR_PLACES = ('first', 'last', 'middle')


def error_case(kind, place, n=600):
  """n good templates with the bad one at template 0, n - 1 or n / 2: (the bad input, the good templates alone)."""
  at = {'first': 0, 'last': n - 1, 'middle': n // 2}[place]
  out = []
  for bad in (True, False):
    b = _Fastq(True, 800)
    for i in range(n):
      c = i % 3
      L1, L2 = 1 + i % 9, 1 + i % 7
      reads = [(i & 1, 1 + 7 * i, '{}M'.format(L1), L1), ((i >> 1) & 1, 3 + 5 * i, '{}M'.format(L2), L2)]
      kw = {}
      if i == at:
        if not bad:
          continue
        if kind == 'name_255':
          rid = 'r{}'.format(i)
          kw['rid'] = rid + 'x' * (255 - len(_Fastq.qname(rid, SMALL_REFS[0][c], reads)))
        elif kind == 'chrom_unknown':
          kw['qname'] = _Fastq.qname('r', '11', reads)   # ('1' is a prefix of it)
        elif kind == 'fields_too_few':
          kw['qname'] = _Fastq.qname('r', '1', reads[:1])   # one read's fields in a paired input
        elif kind == 'name_1_byte':
          kw['qname'] = 'a'
        elif kind == 'strand_not_numeric':
          reads[1] = ('x',) + reads[1][1:]
        elif kind == 'pos_not_numeric':
          reads[0] = (0, '12a', '4M', 4)
        elif kind.startswith('cigar_'):
          reads[1] = reads[1][:2] + ({'cigar_op_first': 'M5', 'cigar_op_only': 'M', 'cigar_trailing_number': '5M3',
                                      'cigar_number_only': '5', 'cigar_unknown_letter': '5Z'}[kind], reads[1][3])
        elif kind == 'no_at':
          kw['lead'] = b'>'
      b.add(SMALL_REFS[0][c], reads, **kw)
      if i == at and kind == 'seq_qual_file2':
        b.recs[1][-1][3] += b'I'
    out.append(b.case(*SMALL_REFS))
  return out


# ---- registry -----------------------------------------------------------------------------------------------------
CASES = collections.OrderedDict()
for _p in (True, False):
  CASES['read_lengths_{}'.format('paired' if _p else 'single')] = functools.partial(read_lengths, _p)
CASES['nt16_sweep'] = nt16_sweep
for _T in TEMPLATE_COUNTS:
  CASES['templates_{}_{}'.format(_T, 'paired' if _T % 2 else 'single')] = functools.partial(template_count, _T, _T % 2 == 1)
for _T in (1, 9, 65, 256):
  _k = 'templates_{}_{}'.format(_T, 'single' if _T % 2 else 'paired')
  CASES[_k] = functools.partial(template_count, _T, _T % 2 == 0)
for _p in (True, False):
  CASES['names_{}'.format('paired' if _p else 'single')] = functools.partial(names, _p)
CASES['cigars'] = cigars
CASES['bins'] = bins
CASES['bins_past_ln'] = functools.partial(bins, True, False)
CASES['bins_past_ln_big'] = functools.partial(bins, True, True)
for _n in N_REFS:
  CASES['refs_{}'.format(_n)] = functools.partial(references, _n)
CASES['ties'] = ties
BIG = ('bins_past_ln_big',)
SMALL = tuple(k for k in CASES if k not in BIG)
WRITTEN = tuple(k for k in CASES if k.startswith(('bins', 'refs_', 'ties')))   # cases whose files are checked too


@functools.lru_cache(maxsize=None)
def case(name):
  return CASES[name]()


def ref_dict(c):
  return {n: i for i, n in enumerate(c.ref_names)}


def expected_of(c):
  recs = god.sorted_stream(god.god_records(c.fq1, c.fq2, ref_dict(c)))
  enc = [god.encode(r) for r in recs]
  soff = np.concatenate([[0], np.cumsum([len(e) for e in enc], dtype=np.int64)]).astype(np.int64)
  return Expected(recs, enc, b''.join(enc), soff)


@functools.lru_cache(maxsize=None)
def expected(name):
  return expected_of(case(name))


def bai_plan(c, e):
  """mh_bam_bai_runs' arrays restated with NumPy from the oracle's sorted records and their data offsets: runs of
  consecutive records of one (tid, bin) as (tid << 32 | bin, first offset, end offset, count); per 16 kbp window of
  every reference the offset of the first record overlapping it or -1; per reference its window count (the last
  window any record overlaps, plus one)."""
  n = len(e.recs)
  tid = np.array([r['reference_id'] for r in e.recs], np.int64)
  beg = np.array([r['pos'] for r in e.recs], np.int64)
  end = np.array([god.end_pos(r) for r in e.recs], np.int64)
  bn = np.array([god.reg2bin(r['pos'], god.end_pos(r)) for r in e.recs], np.int64)
  key = tid << 32 | bn
  first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if n else np.zeros(0, np.int64)
  last = np.concatenate([first[1:], [n]]) if n else first
  runs = np.stack([key[first], e.soff[first], e.soff[last], last - first], 1) if n else np.zeros((0, 4), np.int64)
  woff = np.concatenate([[0], np.cumsum([(ln >> 14) + 1 for ln in c.ref_lengths])]).astype(np.int64)
  win = np.full(int(woff[-1]), -1, np.int64)
  w0, w1 = beg >> 14, (end - 1) >> 14
  for k in range(n - 1, -1, -1):   # backwards: the earliest record overlapping a window is written last
    win[woff[tid[k]] + w0[k]:woff[tid[k]] + w1[k] + 1] = e.soff[k]
  nwin = np.zeros(len(c.ref_lengths), np.int64)
  np.maximum.at(nwin, tid, w1 + 1)
  return runs.astype(np.int64), win, nwin
