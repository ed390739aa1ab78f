"""Test-side statement of filter-bam: the verdict over (qname, flag, reference name or None, pos, mapq) tuples by
readgenerate.parse_qname / score_alignment_error (pinned to the reference by test_score_cpu.py), and a strict splitter
of a BAM file into its header and records."""
import collections
import struct
import zlib

from mitty_amd.simulation import readgenerate as rg

COUNTS = ('seen', 'kept', 'dropped_score', 'dropped_mapq', 'skipped_unplaced', 'skipped_sample', 'bytes_in',
          'bytes_kept')
BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')

_A = collections.namedtuple('A', ['pos', 'reference_name'])


class RecordError(ValueError):
  """A record that fails the session; .index is its position in the input."""

  def __init__(self, index, what):
    ValueError.__init__(self, 'record {}: {}'.format(index, what))
    self.index = index


def verdicts(aligned, max_d=200, strict=False, sample=None, min_derr=1, max_derr=None, min_mq=0, max_mq=255,
             unscored='drop', sizes=None, known_refs=None):
  """(kept indices, counts dict) of the tuples, the verdict applied in the order mh_filter.hip documents:
    1. ref None (tid < 0), or a qname that does not start with `sample`: kept iff unscored == 'keep', qname not parsed
    2. otherwise scored; a qname that does not parse, a read2 record on a one-group qname, and a reference outside
       known_refs (a tid past the names; checked before the sample) raise RecordError
    3. kept iff min_derr <= |d_err| <= max_derr and min_mq <= mapq <= max_mq
  sizes: the records' bytes, for the two byte counts (left 0 without)."""
  d_hi = max_d if max_derr is None else max_derr
  kept, c = [], dict.fromkeys(COUNTS, 0)
  for i, (q, flag, ref, pos, mapq) in enumerate(aligned):
    size = sizes[i] if sizes is not None else 0
    c['seen'] += 1
    c['bytes_in'] += size
    keep = False
    if ref is None:
      c['skipped_unplaced'] += 1
      keep = unscored == 'keep'
    elif known_refs is not None and ref not in known_refs:
      raise RecordError(i, 'tid outside the references')
    elif sample is not None and not q.startswith(sample):
      c['skipped_sample'] += 1
      keep = unscored == 'keep'
    else:
      try:
        reads = rg.parse_qname(q)
        ri = reads[1 if flag & 0x80 else 0]
        d = rg.score_alignment_error(_A(pos, ref), ri, max_d=max_d, strict=strict)
      except (ValueError, IndexError) as e:
        raise RecordError(i, str(e))
      if not min_derr <= abs(d) <= d_hi:
        c['dropped_score'] += 1
      elif not min_mq <= mapq <= max_mq:
        c['dropped_mapq'] += 1
      else:
        keep = True
    if keep:
      kept.append(i)
      c['kept'] += 1
      c['bytes_kept'] += size
  return kept, c


def bgzf_members(data):
  """The inflated payload of every BGZF member of `data`, each checked: the fixed header bytes, the BC field, BSIZE
  inside the file, a raw deflate stream that ends exactly before the trailer, CRC32 and ISIZE.  The file must end with
  the EOF marker, which must be the only empty member at the end."""
  assert data.endswith(BGZF_EOF), 'no BGZF EOF marker'
  out, o = [], 0
  while o < len(data):
    assert data[o:o + 4] == b'\x1f\x8b\x08\x04' and data[o + 10:o + 16] == b'\x06\0BC\x02\0', 'bad member at {}'.format(o)
    bsize = struct.unpack_from('<H', data, o + 16)[0] + 1
    assert o + bsize <= len(data), 'member at {} runs past the file'.format(o)
    d = zlib.decompressobj(-15)
    raw = d.decompress(data[o + 18:o + bsize - 8])
    assert d.eof and not d.unused_data, 'deflate stream of the member at {} does not fill it'.format(o)
    crc, isize = struct.unpack_from('<II', data, o + bsize - 8)
    assert crc == zlib.crc32(raw) and isize == len(raw) <= 0xff00, 'CRC32 / ISIZE of the member at {}'.format(o)
    out.append(raw)
    o += bsize
  assert out[-1] == b'' and data[len(data) - 28:] == BGZF_EOF
  return out[:-1]


def split_bam(data):
  """(header text, [(name, length)], [record bytes, block_size included]) of a BAM file's bytes."""
  raw = b''.join(bgzf_members(data))
  assert raw[:4] == b'BAM\1'
  l_text = struct.unpack_from('<i', raw, 4)[0]
  text = raw[8:8 + l_text].decode()
  o = 8 + l_text
  n_ref = struct.unpack_from('<i', raw, o)[0]
  o += 4
  refs = []
  for _ in range(n_ref):
    l_name = struct.unpack_from('<i', raw, o)[0]
    name = raw[o + 4:o + 4 + l_name]
    assert name.endswith(b'\0')
    refs.append((name[:-1].decode(), struct.unpack_from('<i', raw, o + 4 + l_name)[0]))
    o += 8 + l_name
  recs = []
  while o < len(raw):
    assert o + 4 <= len(raw), 'truncated record'
    size = 4 + struct.unpack_from('<i', raw, o)[0]
    assert size >= 36 and o + size <= len(raw), 'truncated record'
    recs.append(raw[o:o + size])
    o += size
  return text, refs, recs


def member_sizes(data):
  """The inflated sizes of the file's BGZF members, the EOF marker left out."""
  return [len(m) for m in bgzf_members(data)]
