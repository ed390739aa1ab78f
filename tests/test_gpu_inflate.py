"""BGZF inflate on the device (mitty_amd/csrc/mh_inflate.hip) behind mh_bgzf_inflate_gpu and mh_bamfile_open_gpu: the
named valid streams of tests/inflate_cases.py against gzip, the device deflate's output inflated back, the launch
shapes (one member, two, more members than a grid holds, mixed block types), the named malformed streams as an error
code and offset (fixed inputs whose handling tests/test_inflate_cpu.py has shown bounds-safe under the sanitizers), the
reader on the device path against the host path (header, chunks, error texts), and the four consumers and one CLI run
with gpu_inflate on and off."""
import gzip
import pickle

import numpy as np
import pytest

from tests import deflate_cases as D
from tests import inflate_cases as I
from tests import model_util as MU
from tests import score_util as SU
from tests.test_gpu_cov import golden_files      # noqa: F401  (fixtures: the BAMs the existing GPU tests build)
from tests.test_gpu_model import golden_bams     # noqa: F401
from tests.test_gpu_score import golden_bam      # noqa: F401
from tests.test_inflate_cpu import MALFORMED, NAMES

pytestmark = pytest.mark.gpu


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
def valid(tmp_path_factory):
  ref = D.Reference(D.build_tool(tmp_path_factory), tmp_path_factory.mktemp('ref'))
  return I.valid_cases(ref)


# ---- known answers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_valid_case(native, valid, name):
  z, data = valid[name]
  assert gzip.decompress(z) == data
  assert native.bgzf_inflate_gpu(z) == data


def test_round_trip_through_the_device_deflate(native, ctx, valid):
  for name in NAMES:
    data = valid[name][1]
    z = ctx.bgzf_compress(data)
    assert native.bgzf_inflate_gpu(z) == data, name
  both = valid['dynamic6'][1] + D.grid() + valid['zeros'][1]          # several members, odd destination offsets
  assert native.bgzf_inflate_gpu(ctx.bgzf_compress(both) + I.EOF) == both


def test_launch_shapes(native, valid):
  text = D.text(300000, seed=11)
  one = I.bgzf(text[:100], block=100)
  assert len(I.split(one)) == 1 and native.bgzf_inflate_gpu(one) == text[:100]
  two = I.bgzf(text[:201], block=101)
  assert len(I.split(two)) == 2 and native.bgzf_inflate_gpu(two) == text[:201]
  many = I.bgzf(text, block=100)                                       # more members than the grid has workgroups
  assert len(I.split(many)) == 3000 and native.bgzf_inflate_gpu(many) == text
  mixed = b''.join(valid[n][0] for n in ('empty', 'stored', 'fixed', 'dynamic9', 'eof_marker', 'one_byte',
                                         'stored_after_dynamic', 'full_64k', 'far_distance'))
  assert native.bgzf_inflate_gpu(mixed) == gzip.decompress(mixed)
  assert native.bgzf_inflate_gpu(b'') == b''


def test_capacity_and_framing_errors(native):
  import ctypes
  z = I.bgzf(D.text(5000, seed=2))
  src = np.frombuffer(z, np.uint8)
  out = np.zeros(100, np.uint8)
  used, bad = ctypes.c_int64(), ctypes.c_int64()
  rc = native.lib().mh_bgzf_inflate_gpu(0, native._ptr(src), len(z), native._ptr(out), 100, ctypes.byref(used),
                                        ctypes.byref(bad))
  assert rc == native.MH_E_CAPACITY and used.value == 5000 and not out.any()
  for cut in (10, 30, len(z) - 1):                                      # a header or a block cut by the end
    with pytest.raises(ValueError) as e:
      native.bgzf_inflate_gpu(z + z[:cut])
    assert e.value.bad_offset == len(z)


@pytest.mark.parametrize('name', MALFORMED)
def test_malformed_case(native, name):
  raw, isize, crc = I.malformed_cases()[name]
  first, last = I.bgzf(D.text(3000, seed=4)), I.bgzf(D.text(70000, seed=5))
  with pytest.raises(ValueError) as e:
    native.bgzf_inflate_gpu(first + I.member(raw, isize, crc) + last)
  assert e.value.bad_offset == len(first)
  assert native.bgzf_inflate_gpu(first + last) == gzip.decompress(first + last)   # nothing is left poisoned


# ---- the reader -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def parity_bam():
  """300 records of 60 to 2400 bases over three references: about 0.6 MB of BAM."""
  rng = np.random.default_rng(21)
  sq = [{'SN': 'chr{}'.format(i + 1), 'LN': 1000000 + i} for i in range(3)]
  recs = []
  for k in range(300):
    n = int(rng.integers(60, 2400))
    seq = ''.join('ACGT'[b] for b in rng.integers(0, 4, n))
    recs.append(SU.record('q{}'.format(k), 0, int(rng.integers(0, 3)), int(rng.integers(0, 900000)), 60, seq=seq))
  return SU.bam_bytes(recs, sq, '@HD\tVN:1.4\n@CO\t' + 'x' * 3000 + '\n'), recs


def _read(native, path, device, max_bytes):
  """('ok' | the error text, header, [(record bytes, offsets, n)]) of a whole read."""
  chunks, header = [], None
  try:
    bam = native.BamFile(path, threads=2, device=device)
  except ValueError as e:
    return str(e), header, chunks
  try:
    header = (bam.text, bam.names, bam.lengths)
    for recs, roff in bam.chunks(max_bytes):
      chunks.append((recs, roff.tolist(), len(roff) - 1))
    return 'ok', header, chunks
  except ValueError as e:
    return str(e), header, chunks
  finally:
    bam.close()


@pytest.mark.parametrize('block', [0xff00, 997])
def test_reader_parity(native, parity_bam, tmp_path, block):
  data, recs = parity_bam
  z = SU.bgzf_bytes(data, block=block)
  assert len(I.split(z)) >= 10
  path = str(tmp_path / 'p.bam')
  with open(path, 'wb') as f:
    f.write(z)
  for max_bytes in (1, 4096, 64 << 20):
    host, dev = _read(native, path, None, max_bytes), _read(native, path, 0, max_bytes)
    assert host[0] == 'ok' and dev == host, max_bytes
    assert b''.join(c[0] for c in dev[2]) == b''.join(recs) and sum(c[2] for c in dev[2]) == len(recs)
  # damaged copies: the same text from both readers
  members = I.split(z)
  third = members[2][0]
  size = members[3][0] - third
  crc_at = third + size - 8
  flipped = bytearray(z)
  flipped[crc_at] ^= 0x10
  cut_record = SU.bgzf_bytes(data[:len(data) - 7], block=block)
  wants = {'mid_block': 'truncated BGZF block', 'crc': 'fails to inflate or its CRC32',
           'record': 'BAM record cut by the end'}
  for name, bad in (('mid_block', z[:third + size // 2]), ('crc', bytes(flipped)), ('record', cut_record)):
    with open(path, 'wb') as f:
      f.write(bad)
    for max_bytes in (4096, 64 << 20):
      host, dev = _read(native, path, None, max_bytes), _read(native, path, 0, max_bytes)
      assert wants[name] in host[0], (name, host[0])
      assert dev[0] == host[0] and dev[1] == host[1], (name, max_bytes, dev[0], host[0])


# ---- the consumers --------------------------------------------------------------------------------------------------------
def _equal(a, b):
  if isinstance(a, dict):
    return isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
  if isinstance(a, (list, tuple)):
    return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
  if isinstance(a, np.ndarray):
    if a.dtype.names:                                                  # (a NaN in a record array: field by field)
      return a.dtype == b.dtype and all(_equal(a[n], b[n]) for n in a.dtype.names)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
  return a == b or (a != a and b != b)


def test_score_bam_with_gpu_inflate(native, golden_bam):   # noqa: F811
  from mitty_amd.benchmarking import derr, mq, score
  for kw in ({}, {'chunk_bytes': 20000}, {'strict': True, 'max_d': 5}):
    host = score.score_bam(golden_bam, processes=3, **kw)
    dev = score.score_bam(golden_bam, processes=3, gpu_inflate=True, **kw)
    assert host[2]['scored'] > 0 and _equal(dev, host), kw
  assert _equal(mq.process_bam(golden_bam, gpu_inflate=True), mq.process_bam(golden_bam))
  assert _equal(derr.process_bam(golden_bam, gpu_inflate=True), derr.process_bam(golden_bam))


def test_bam2illumina_with_gpu_inflate(native, golden_bams, tmp_path):   # noqa: F811
  from mitty_amd.empirical import bam2illumina as b2i
  g = MU.golden()
  for name in ('defaults', 'every3'):
    s = g['sets'][name]
    host = b2i.process_bam_parallel(golden_bams[name], str(tmp_path / 'h.npz'), threads=3, **s['params'])
    dev = b2i.process_bam_parallel(golden_bams[name], str(tmp_path / 'd.npz'), threads=3, gpu_inflate=True,
                                   chunk_bytes=20000, **s['params'])
    assert host['r_cnt'] > 0 and _equal(dev, host), name


def test_gc_and_bq_with_gpu_inflate(native, golden_files, tmp_path):   # noqa: F811
  from mitty_amd.empirical import bq, gc
  bam, fasta = golden_files['bam'], golden_files['fasta']
  host = gc.process_bam_parallel(bam, fasta, str(tmp_path / 'h.pkl'), block_len=100, threads=3)
  dev = gc.process_bam_parallel(bam, fasta, str(tmp_path / 'd.pkl'), block_len=100, threads=3, gpu_inflate=True,
                                chunk_bytes=20000)
  assert len(host) > 0 and _equal(dev, host)
  with open(str(tmp_path / 'd.pkl'), 'rb') as f:
    assert _equal(pickle.load(f), host)
  host = bq.process_bam_parallel(bam, str(tmp_path / 'hb.pkl'), threads=3)
  dev = bq.process_bam_parallel(bam, str(tmp_path / 'db.pkl'), threads=3, gpu_inflate=True)
  assert len(host) > 0 and _equal(dev, host)
  empty = golden_files['empty']                                         # a header and no record
  assert _equal(bq.process_bam_parallel(empty, str(tmp_path / 'e.pkl'), gpu_inflate=True),
                bq.process_bam_parallel(empty, str(tmp_path / 'f.pkl')))


def test_cli_mq_plot_gpu_inflate(native, golden_bam, tmp_path):   # noqa: F811
  from click.testing import CliRunner
  from mitty_amd import cli
  out = {}
  for flag in ([], ['--gpu-inflate']):
    csv = str(tmp_path / ('mq{}.csv'.format(len(flag))))
    res = CliRunner().invoke(cli.cli, ['mq-plot', golden_bam, csv, str(tmp_path / 'mq.png'), '--threads', '3'] + flag)
    assert res.exit_code == 0, res.output
    with open(csv, 'rb') as f:
      out[len(flag)] = f.read()
  assert len(out[0]) > 0 and out[1] == out[0]
