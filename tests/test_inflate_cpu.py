"""The device inflater's decoder core (mitty_amd/csrc/mh_inflate.h) run on the host by tests/inflate_host.cpp, built
with the address and undefined-behaviour sanitizers: named valid streams inflate to zlib's bytes, named malformed ones
(each first shown to be refused by zlib) are refused, and a few thousand seeded corruptions of valid members get zlib's
verdict, all without a sanitizer report.  Then the --gpu-inflate option's presence on the commands and entry points (no
device is used here)."""
import gzip
import inspect

import numpy as np
import pytest

from tests import deflate_cases as D
from tests import inflate_cases as I

FUZZ_SEED, FUZZ_BITS, FUZZ_BYTES = 20240607, 2400, 1600   # 4000 corruptions in all


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
  return I.build_tool(tmp_path_factory)


@pytest.fixture(scope='module')
def valid(tmp_path_factory):
  ref = D.Reference(D.build_tool(tmp_path_factory), tmp_path_factory.mktemp('ref'))
  return I.valid_cases(ref)


NAMES = ['stored', 'fixed', 'dynamic1', 'dynamic6', 'dynamic9', 'zeros', 'one_byte', 'empty', 'eof_marker', 'full_64k',
         'small_blocks', 'far_distance', 'len_285', 'len_284_max_extra', 'stored_after_dynamic', 'single_distance_code',
         'device_grid', 'device_wide_tokens', 'device_fibonacci']


def test_case_list_is_complete(valid):
  assert sorted(valid) == sorted(NAMES)


@pytest.mark.parametrize('name', NAMES)
def test_valid_case(tool, valid, tmp_path, name):
  z, data = valid[name]
  assert gzip.decompress(z) == data                       # zlib's bytes
  members = [(raw, isize, crc) for _, raw, isize, crc in I.split(z)]
  got = I.run_core(tool, tmp_path, members)
  assert [st for st, _ in got] == [I.ST_OK] * len(members)
  assert b''.join(b for _, b in got) == data


def test_valid_cases_have_their_shapes(valid):
  """The inputs are what their names say (first block types, member sizes, the device deflate's eight blocks)."""
  def btype(raw):
    return (raw[0] >> 1) & 3
  first = {n: btype(I.split(valid[n][0])[0][1]) for n in NAMES}
  assert first['stored'] == 0 and first['fixed'] == 1 and first['dynamic6'] == 2
  assert first['far_distance'] == 1 and first['len_284_max_extra'] == 2 and first['single_distance_code'] == 2
  assert I.split(valid['full_64k'][0])[0][2] == 65536
  assert [m[2] for m in I.split(valid['empty'][0])] == [0]
  assert len(I.split(valid['small_blocks'][0])) == 21
  assert len(valid['far_distance'][1]) == 32768 + 3 + 2 + 200
  for n in ('device_grid', 'device_wide_tokens'):
    assert all(btype(m[1]) == 2 and not (m[1][0] & 1) for m in I.split(valid[n][0]))   # dynamic, more blocks follow


MALFORMED = ['btype3', 'len_nlen_mismatch', 'oversubscribed_litlen', 'incomplete_litlen', 'repeat16_first', 'hlit_287',
             'symbol_286', 'distance_code_30', 'distance_too_far', 'cut_mid_symbol', 'one_byte_short', 'one_byte_more',
             'crc_bit_flipped', 'wrong_isize']


def test_malformed_cases(tool, tmp_path):
  cases = I.malformed_cases()
  assert sorted(cases) == sorted(MALFORMED)
  for name in MALFORMED:                                  # zlib alone defines the list
    assert not I.zlib_verdict(*cases[name])[0], name
  got = I.run_core(tool, tmp_path, [cases[n] for n in MALFORMED])
  for name, (st, out) in zip(MALFORMED, got):
    assert st != I.ST_OK and out == b'', name
  status = dict(zip(MALFORMED, (st for st, _ in got)))
  assert status['crc_bit_flipped'] == I.ST_CRC
  assert status['one_byte_short'] == status['one_byte_more'] == status['wrong_isize'] == I.ST_LENGTH
  assert status['btype3'] == status['distance_too_far'] == status['hlit_287'] == I.ST_BAD_STREAM


def test_zlib_verdict_accepts_the_valid_members(valid):
  for name in NAMES:
    for _, raw, isize, crc in I.split(valid[name][0]):
      assert I.zlib_verdict(raw, isize, crc)[0], name


def test_fuzz_matches_zlib(tool, valid, tmp_path):
  """FUZZ_BITS single-bit and FUZZ_BYTES single-byte corruptions (payload or trailer) of valid members, seeded: the
  core's good / bad equals zlib's for every one, and a good one's bytes are equal."""
  rng = np.random.default_rng(FUZZ_SEED)
  pool = []
  for name in ('stored', 'fixed', 'dynamic6', 'one_byte', 'len_284_max_extra', 'stored_after_dynamic',
               'single_distance_code', 'small_blocks', 'device_fibonacci', 'device_grid'):
    pool += [(raw, isize, crc) for _, raw, isize, crc in I.split(valid[name][0])][:3]
  # short members are drawn more often than their share of the bytes: headers and tables are where a flip matters
  members = []
  for k in range(FUZZ_BITS + FUZZ_BYTES):
    raw, isize, crc = pool[int(rng.integers(0, len(pool)))]
    blob = bytearray(raw + isize.to_bytes(4, 'little') + crc.to_bytes(4, 'little'))
    # half of the hits land in the first 64 bytes (block headers, code lengths)
    at = int(rng.integers(0, min(64, len(blob)))) if rng.integers(0, 2) else int(rng.integers(0, len(blob)))
    if k < FUZZ_BITS:
      blob[at] ^= 1 << int(rng.integers(0, 8))
    else:
      blob[at] = int(rng.integers(0, 256))
    n = len(raw)
    isz = int.from_bytes(blob[n:n + 4], 'little')
    if isz > 65536:                                       # the header walk refuses these before any inflate
      isz = isize
    members.append((bytes(blob[:n]), isz, int.from_bytes(blob[n + 4:n + 8], 'little')))
  assert len(members) == 4000
  got = I.run_core(tool, tmp_path, members)
  good = 0
  for k, (m, (st, out)) in enumerate(zip(members, got)):
    ok, ref = I.zlib_verdict(*m)
    assert (st == I.ST_OK) == ok, (k, st, ok)
    if ok:
      assert out == ref, k
      good += 1
  assert 0 < good < len(members)                          # both verdicts occur


# ---- the option ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('command', ['mq-plot', 'derr-plot', 'bam2illumina', 'gc-cov', 'bq'])
def test_cli_has_gpu_inflate(command):
  from click.testing import CliRunner
  from mitty_amd import cli
  res = CliRunner().invoke(cli.cli, [command, '--help'])
  assert res.exit_code == 0, res.output
  assert '--gpu-inflate' in res.output


def test_entry_points_take_gpu_inflate():
  from mitty_amd.benchmarking import derr, mq, score
  from mitty_amd.empirical import bam2illumina, bq, gc
  for fn in (score.score_bam, mq.process_bam, derr.process_bam, bam2illumina.process_bam_parallel,
             gc.process_bam_parallel, bq.process_bam_parallel):
    p = inspect.signature(fn).parameters
    assert 'gpu_inflate' in p and p['gpu_inflate'].default is False, fn


def test_native_declares_the_new_symbols():
  from mitty_amd import _native
  assert 'mh_bamfile_open_gpu' in _native.EXPORTS and 'mh_bgzf_inflate_gpu' in _native.EXPORTS
  assert 'device' in inspect.signature(_native.BamFile.__init__).parameters
  assert callable(_native.bgzf_inflate_gpu)
