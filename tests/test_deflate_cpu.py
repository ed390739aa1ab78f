"""The single-thread parts of the device BGZF compressor (mitty_amd/csrc/mh_deflate.h) on the CPU: a sequential
restatement of its parse (tests/deflate_host.cpp) builds BGZF with the shared Huffman / header / CRC code, and zlib
inflates it back.  The device kernel itself is checked in tests/test_gpu_parity.py::test_device_bgzf_* and, byte for
byte against this restatement under the kernel's store rule (--device-rules), in tests/test_gpu_deflate.py."""
import gzip
import os
import subprocess

import pytest

import numpy as np

from tests import deflate_cases as C
from tests import golden_io as G

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
  return C.build_tool(tmp_path_factory)


@pytest.mark.parametrize('name', ['fastq', 'zeros', 'tiny', 'abc', 'text', 'multi'])
def test_bgzf_shared_code_round_trip(tool, tmp_path, name):
  data = {'fastq': lambda: G.fastq_bytes('e2e_hiseq-X-v2.5-Garvan.r1.fq.gz'),
          'zeros': lambda: b'\0' * 200000,
          'tiny': lambda: b'A',
          'abc': lambda: b'abcabcabcabc' * 7,
          'text': lambda: open(os.path.join(HERE, '..', 'DESIGN.md'), 'rb').read(),
          'multi': lambda: (G.fastq_bytes('e2e_1kg-pcr-free.r2.fq.gz') * 3)[:400_001]}[name]()
  src, dst = tmp_path / 'in', tmp_path / 'out'
  src.write_bytes(data)
  subprocess.check_call([tool, str(src), str(dst)])
  z = dst.read_bytes()
  assert gzip.decompress(z) == data
  if name in ('fastq', 'multi'):   # FASTQ compresses about as well as gzip -1 (~4x)
    assert len(z) < len(data) / 3.5


def test_bgzf_shared_code_incompressible_block_is_flagged(tool, tmp_path):
  src, dst = tmp_path / 'in', tmp_path / 'out'
  src.write_bytes(os.urandom(100000))
  assert subprocess.run([tool, str(src), str(dst)]).returncode == 3   # the device stores such a block


def test_huffman_fuzz(tool):
  """huffman_from_sorted on 30,000 frequency sets per limit (15, 7) and family (random, Fibonacci, near-flat, powers
  of two): Kraft sum exactly 1, lengths in 1..limit, monotone in frequency, equal to the unlimited lengths whenever
  those fit; the tool fails unless some sets fold at each limit."""
  p = subprocess.run([tool, '--fuzz-huffman', '30000', '20240611'], stderr=subprocess.PIPE)
  assert p.returncode == 0, p.stderr.decode()
  assert p.stderr.decode().count('folded') == 2


def _stored(z):
  out, o = [], 0
  for bsize, isize in C.bgzf_members(z):
    ln, nln = (int.from_bytes(z[o + k:o + k + 2], 'little') for k in (19, 21))
    out.append(bsize == 18 + 5 + isize + 8 and z[o + 18] == 1 and ln == isize == 0xffff ^ nln)
    o += bsize
  return out


@pytest.mark.parametrize('name', ['one', 'five', 'tiny_text', 'random', 'mixed', 'grid', 'wide', 'fib'])
def test_device_rules_round_trip(tool, tmp_path, name):
  """--device-rules: the device's store rule on tiny and incompressible blocks (exit 0, stored members that inflate),
  the stored count reported, deflated members otherwise."""
  rnd = np.random.default_rng(5).integers(0, 256, 70000, dtype=np.uint8).tobytes()
  data, stored = {'one': (b'A', [True]), 'five': (b'tail\n', [True]), 'tiny_text': (C.sized(8), [True]),
                  'random': (rnd, [True, True]),
                  'mixed': (C.sized(C.BLOCK) + rnd[:C.BLOCK] + C.sized(300), [False, True, False]),
                  'grid': (C.grid(), [False]), 'wide': (C.wide_tokens(1), [False]),
                  'fib': (C.fibonacci_literals(0), [False])}[name]
  z, rep = C.Reference(tool, tmp_path)(data)
  assert gzip.decompress(z) == data
  assert _stored(z) == stored and rep['stored_blocks'] == sum(stored) and rep['blocks'] == len(stored)
  assert len(z) <= C.bgzf_bound(len(data))
  if name == 'fib':   # the 15-bit limiter folds (and zlib accepts the folded code)
    assert rep['fold_lit'] == 1 and rep['matches'] == 0
