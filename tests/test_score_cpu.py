"""CPU-side checks of the alignment scorers (mq-plot / derr-plot): the Python statement of the scoring rule against
the reference's golden d_err, the host BAM reader record for record, the CLI surface, and the reader under
AddressSanitizer / UBSan on malformed files.  No GPU here."""
import collections
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from mitty_amd import _native
from mitty_amd.simulation import readgenerate as rg
from tests import score_util as SU

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Aligned = collections.namedtuple('Aligned', ['pos', 'reference_name'])


@pytest.mark.parametrize('strict', [0, 1])
@pytest.mark.parametrize('max_d', [200, 5])
def test_score_alignment_error_equals_reference(strict, max_d):
  g = SU.golden()
  want = g['d_err']['s{}_d{}'.format(strict, max_d)]
  got = [rg.score_alignment_error(Aligned(pos, ref), rg.parse_qname(q)[1 if flag & 0x80 else 0], max_d=max_d,
                                  strict=bool(strict)) for q, flag, ref, pos, mapq in g['records']]
  assert got == want
  # the fixture spreads over the range (only the strict rule clamps to -max_d: the other takes |d| < max_d strictly)
  assert len(set(want)) >= min(2 * max_d, 20) and max_d in want and (-max_d in want) == bool(strict)


def test_inside_insertion_read_scores_max_d_when_not_strict():
  # parse_qname strips '>p:' before the rule looks for '>': the read scores max_d wherever it is placed
  ri = rg.parse_qname('S:0|1|0|0|100|5|>3:5I|5')[0]
  assert ri.cigar == '5I' and ri.special_cigar == '>3:5I'
  assert rg.score_alignment_error(Aligned(99, '1'), ri, 200, False) == 200
  assert rg.score_alignment_error(Aligned(99, '1'), ri, 200, True) == 0


def _write(tmp_path, name, data):
  p = str(tmp_path / name)
  with open(p, 'wb') as fp:
    fp.write(data)
  return p


def _read_all(path, chunk, threads=3):
  bam = _native.BamFile(path, threads=threads)
  try:
    out, sizes = [], []
    for recs, roff in bam.chunks(chunk):
      assert roff[0] == 0 and roff[-1] == len(recs)
      out += [recs[roff[i]:roff[i + 1]] for i in range(len(roff) - 1)]
      sizes.append(len(roff) - 1)
    return bam.text, bam.names, bam.lengths, out, sizes
  finally:
    bam.close()


@pytest.mark.parametrize('block', [0xff00, 997, 61])
def test_reader_returns_every_record(tmp_path, block):
  g = SU.golden()
  recs = g['recs'][:700]
  text = '@HD\tVN:1.4\n@CO\t' + 'x' * 300 + '\n'
  path = _write(tmp_path, 'a.bam', SU.bgzf_bytes(SU.bam_bytes(recs, g['sq'], text), block=block))
  for chunk in (1, 300, 5000, 1 << 20):   # single records, records across chunk and block boundaries, one chunk
    t, names, lens, got, sizes = _read_all(path, chunk)
    assert t == text and names == [s['SN'] for s in g['sq']] and lens == [s['LN'] for s in g['sq']]
    assert got == recs
    if chunk == 1:
      assert set(sizes) == {1}
    if chunk == 1 << 20:
      assert sizes == [len(recs)]


def test_reader_empty_and_single_record_files(tmp_path):
  g = SU.golden()
  for n in (0, 1):
    for eof in (True, False):
      path = _write(tmp_path, 'n{}{}.bam'.format(n, eof), SU.bgzf_bytes(SU.bam_bytes(g['recs'][:n], g['sq']), eof=eof))
      _, names, _, got, _ = _read_all(path, 4096, threads=1)
      assert got == g['recs'][:n] and len(names) == 3
  # no references at all
  path = _write(tmp_path, 'noref.bam', SU.bgzf_bytes(SU.bam_bytes([], [])))
  assert _read_all(path, 4096)[1:4] == ([], [], [])


def test_reader_chunk_ending_at_the_buffer_end_before_the_eof_block(tmp_path):
  """The first chunk ends exactly where the inflated bytes end while only the empty end-of-file block is unread: the
  read-ahead then starts from nothing and has only that ISIZE = 0 block to inflate.  The header read inflates at
  least 1 MiB, so the stream is cut to lie between 1 MiB and the 17th 0xff00-byte block's end."""
  g = SU.golden()
  hdr = len(SU.bam_bytes([], g['sq']))
  recs, size, k = [], hdr, 0
  while size < (1 << 20) + 64:
    recs.append(g['recs'][k % len(g['recs'])])
    size += len(recs[-1])
    k += 1
  assert 16 * 0xff00 < (1 << 20) <= size <= 17 * 0xff00
  path = _write(tmp_path, 'edge.bam', SU.bgzf_bytes(SU.bam_bytes(recs, g['sq'])))
  for chunk in (size - hdr, size - hdr - len(recs[-1]) + 1, 1 << 30):
    _, _, _, got, sizes = _read_all(path, chunk)
    assert got == recs and sizes == [len(recs)], chunk


def test_reader_reports_malformed_files(tmp_path):
  g = SU.golden()
  recs = g['recs'][:50]
  raw = SU.bam_bytes(recs, g['sq'])
  good = SU.bgzf_bytes(raw, block=1500)
  bad_crc = bytearray(good)
  bad_crc[len(SU.bgzf_block(raw[:1500])) - 7] ^= 0x40   # the first block's CRC32
  r0 = bytearray(recs[0])
  r0[12] = 0                                             # l_read_name 0
  r1 = bytearray(recs[0])
  struct.pack_into('<i', r1, 20, 1 << 30)                # l_seq far past block_size
  r2 = bytearray(recs[0])
  r2[36 + r2[12] - 1] = ord('x')                         # name not NUL-terminated
  r3 = bytearray(recs[0])
  struct.pack_into('<I', r3, 0, 0x7fffffff)              # absurd block_size
  cases = {
    'magic': SU.bgzf_bytes(b'BAX\1' + raw[4:]),
    'crc': bytes(bad_crc),
    'truncated': good[:len(good) // 2],
    'cut record': SU.bgzf_bytes(raw[:-7]),
    'not bgzf': raw,
    'empty': b'',
    'l_read_name': SU.bgzf_bytes(SU.bam_bytes([bytes(r0)], g['sq'])),
    'l_seq': SU.bgzf_bytes(SU.bam_bytes([bytes(r1)], g['sq'])),
    'nul': SU.bgzf_bytes(SU.bam_bytes([bytes(r2)], g['sq'])),
    'block_size': SU.bgzf_bytes(SU.bam_bytes([bytes(r3)], g['sq'])),
    'header cut': SU.bgzf_bytes(raw[:30]),
  }
  for what, data in cases.items():
    with pytest.raises(ValueError) as e:
      _read_all(_write(tmp_path, 'bad.bam', data), 4096)
    assert str(e.value), what


def test_cli_lists_the_scoring_commands():
  env = dict(os.environ, PYTHONPATH=REPO)
  out = subprocess.check_output([sys.executable, '-m', 'mitty_amd', '--help'], cwd=REPO, env=env).decode()
  assert 'mq-plot' in out and 'derr-plot' in out
  mq = subprocess.check_output([sys.executable, '-m', 'mitty_amd', 'mq-plot', '--help'], cwd=REPO, env=env).decode()
  for opt in ('BAM CSV PLOT', '--max-d', '--strict-scoring', '--sample-name', '--threads', '--device'):
    assert opt in mq, opt
  de = subprocess.check_output([sys.executable, '-m', 'mitty_amd', 'derr-plot', '--help'], cwd=REPO, env=env).decode()
  for opt in ('BAM CSV PLOT', '--max-v', '--max-d', '--strict-scoring', '--sample-name', '--threads', '--device'):
    assert opt in de, opt


def test_compute_p_err():
  from mitty_amd.benchmarking import mq
  m = np.zeros((100, 11), np.uint64)
  m[60, 5], m[60, 7], m[60, 0], m[10, 10] = 90, 6, 4, 5
  p0, p2 = mq.compute_p_err(m, 0), mq.compute_p_err(m, 2)
  assert p0[60] == 0.1 and p2[60] == 0.04 and p0[10] == 1.0 and p0[0] == 0.0


def test_plots_are_skipped_without_matplotlib(tmp_path, monkeypatch, caplog):
  from mitty_amd.benchmarking import derr, mq
  monkeypatch.setitem(sys.modules, 'matplotlib', None)   # import matplotlib now raises ImportError
  for fn, mat, name in ((mq.plot_mq, np.zeros((100, 11), np.uint64), 'mq.png'),
                        (derr.plot_derr, np.zeros((104, 11), np.uint64), 'derr.png')):
    out = str(tmp_path / name)
    with caplog.at_level('WARNING'):
      assert fn(mat, out) is False
    assert not os.path.exists(out) and 'not drawn' in caplog.text
    caplog.clear()


def test_plots_are_drawn(tmp_path):
  pytest.importorskip('matplotlib')
  from mitty_amd.benchmarking import derr, mq
  g = SU.golden()
  mats = ((mq.plot_mq, SU.dense(g['mq']['s0_d200'], (100, 401)), 'mq.png'),
          (derr.plot_derr, SU.dense(g['derr']['s0_d200_v200'], (402, 401)), 'derr.png'),
          (mq.plot_mq, np.zeros((100, 11), np.uint64), 'mq0.png'),          # no reads at all
          (derr.plot_derr, np.zeros((104, 11), np.uint64), 'derr0.png'))
  for fn, mat, name in mats:
    out = str(tmp_path / name)
    assert fn(mat, out) is True
    with open(out, 'rb') as fp:
      assert fp.read(8) == b'\x89PNG\r\n\x1a\n'


def test_bam_reader_under_asan_ubsan(tmp_path):
  """The reader parses untrusted files: built with -fsanitize=address,undefined as a stand-alone program and fed
  truncated, bit-flipped and absurd-length BAMs, it returns errors (or reads what is still valid) with no sanitizer
  report.  The environment is passed through unchanged."""
  if shutil.which('g++') is None:
    pytest.skip('no g++')
  exe = str(tmp_path / 'san_bamread')
  subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                         '-fno-sanitize-recover=undefined', os.path.join(REPO, 'tests', 'sanitize', 'san_bamread.cpp'),
                         os.path.join(REPO, 'mitty_amd', 'csrc', 'mh_bamread.cpp'), '-lz', '-lpthread', '-o', exe])
  g = SU.golden()
  recs = g['recs'][:400]
  raw = SU.bam_bytes(recs, g['sq'])
  good = SU.bgzf_bytes(raw, block=4000)
  out = subprocess.run([exe, _write(tmp_path, 'good.bam', good), '3', '3000'], capture_output=True, text=True)
  assert out.returncode == 0 and out.stdout.startswith('ok {} {} '.format(len(recs), sum(map(len, recs)))), out
  rs = np.random.RandomState(11)
  n_err = 0
  for k in range(48):
    kind = k % 6
    if kind == 0:     # the file truncated anywhere
      b = good[:rs.randint(0, len(good))]
    elif kind == 1:   # bits flipped in the compressed file
      b = bytearray(good)
      for _ in range(4):
        b[rs.randint(len(b))] ^= 1 << rs.randint(8)
    elif kind == 2:   # bits flipped in the BAM stream (valid BGZF around it)
      u = bytearray(raw)
      for _ in range(6):
        u[rs.randint(len(u))] ^= 1 << rs.randint(8)
      b = SU.bgzf_bytes(bytes(u), block=int(rs.randint(50, 5000)))
    elif kind == 3:   # absurd lengths: block_size, l_read_name, n_cigar, l_seq of a record
      u = bytearray(raw)
      o = len(raw) - sum(map(len, recs[rs.randint(1, len(recs)):]))
      field, fmt = [(0, '<I'), (12, '<B'), (16, '<H'), (20, '<i')][rs.randint(4)]
      struct.pack_into(fmt, u, o + field, [0, 1, 0xff, 0x7fffffff, 0xffffffff, 40000][rs.randint(6)] &
                       {'<I': 0xffffffff, '<B': 0xff, '<H': 0xffff, '<i': 0x7fffffff}[fmt])
      b = SU.bgzf_bytes(bytes(u), block=3000)
    elif kind == 4:   # absurd header lengths: l_text, n_ref, l_name
      u = bytearray(raw)
      struct.pack_into('<i', u, [4, 8 + struct.unpack_from('<i', raw, 4)[0], 12 + struct.unpack_from('<i', raw, 4)[0]][
        rs.randint(3)], [-1, 0x7fffffff, 1 << 20, 0][rs.randint(4)])
      b = SU.bgzf_bytes(bytes(u))
    else:             # the uncompressed stream cut inside a record or the header
      b = SU.bgzf_bytes(raw[:rs.randint(1, len(raw))], block=2000)
    out = subprocess.run([exe, _write(tmp_path, 'm.bam', bytes(b)), str(1 + k % 4), str([1, 700, 100000][k % 3])],
                         capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, (k, out.returncode, out.stdout[-300:], out.stderr[-3000:])
    assert out.stdout.startswith(('ok ', 'error ')), (k, out.stdout)
    n_err += out.stdout.startswith('error ')
  # the 16 cut files (kinds 0 and 5) end inside a block or a record unless the cut falls on one of a few hundred
  # boundaries among ~10^5 offsets; flips may land in sequence or quality bytes, where they are harmless
  assert n_err >= 14
