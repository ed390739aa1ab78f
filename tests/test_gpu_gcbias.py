"""GC-bias thinning on the device (mh_gc_thin, mh_gcbias.hip) against its NumPy restatement (tests/gcbias_ref.py), by
exact equality: imported sets at the lane-group, workgroup and scan-tile edges with spans at every alignment and
across both ends of the haplotype; the extremes; sampled sets (start nodes carried) through both emission paths; the
state errors; and generate-reads end to end on the golden genome, one process and the distributed driver."""
import numpy as np
import pytest

from tests import gcbias_ref as GR
from tests import golden_io as G
from tests import splice_ref as R

pytestmark = pytest.mark.gpu

CID, SLOT_A, SLOT_B, SLOT_S = 900, 40, 41, 42
RS = 1001                                   # ref_start_pos of the hand-built haplotypes
SEED, UNIT_KEY = (0x1234 << 32) | 77, (0x9 << 32) | 0xdeadbeef
FULL = np.full(GR.N_BINS, 1 << 32, np.uint64)
G_RUN = (30000, 32000)                      # an all-'G' stretch of haplotype A's reference (offsets)


def _curve(name):
  from mitty_amd.simulation import gcbias
  b = np.arange(GR.N_BINS)
  w = {'step': np.where(b < 45, 1.0, 0.25), 'ramp': 0.05 + 0.9 * b / 100.0, 'flat': np.ones(GR.N_BINS)}[name]
  return w, gcbias.thresholds(w)


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


def _ref_a():
  """~70 kB: a low-GC half and a high-GC half (different base frequencies), a lower-case stretch, an N run and an
  all-'G' stretch."""
  rng = np.random.default_rng(5)
  acgt = np.frombuffer(b'ACGT', np.uint8)
  lo = acgt[rng.choice(4, 35000, p=[0.35, 0.15, 0.15, 0.35])]
  hi = acgt[rng.choice(4, 35011, p=[0.17, 0.33, 0.33, 0.17])]
  s = np.concatenate([lo, hi])
  s[12000:12700] = np.frombuffer(bytes(s[12000:12700]).lower(), np.uint8)
  s[50000:50900] = ord('N')
  s[G_RUN[0]:G_RUN[1]] = ord('G')
  return s.tobytes()


@pytest.fixture(scope='module')
def hap_a(ctx):
  ref = _ref_a()
  v = R.soa_of([(RS + 2000, 'X', 0, b'T'), (RS + 8000, 'I', 7, b'A' + b'GGCCGGC'), (RS + 20000, 'D', 33, b'A'),
                (RS + 44000, 'I', 300, b'C' + b'GC' * 150), (RS + 61000, 'D', 5, b'A')])
  ctx.upload_contig(CID, ref)
  n_nodes, p_min, p_max = ctx.build_haplotype(SLOT_A, CID, RS, v)
  hap = ctx.get_nodes(SLOT_A, n_nodes)[4]
  assert len(hap) == len(ref) + 7 - 33 + 300 - 5 and p_min == RS
  return hap, p_min


@pytest.fixture(scope='module')
def hap_b(ctx):
  """A deletion running past the region end: hap_len < p_max - p_min."""
  ref = R.contig(5003, 17)
  v = R.soa_of([(RS + 100, 'X', 0, b'G'), (RS + len(ref) - 4, 'D', 5, ref[-4:-3])])
  ctx.upload_contig(CID + 1, ref)
  n_nodes, p_min, p_max = ctx.build_haplotype(SLOT_B, CID + 1, RS, v)
  hap = ctx.get_nodes(SLOT_B, n_nodes)[4]
  assert len(hap) < p_max - p_min
  return hap, p_min


def _templates(n, hap_len, p_min, rlen, seed):
  """n templates whose spans [pos0, pos1 + rlen) cycle through: 1, 15, 16, 17 and ~500 bytes at a start of every
  residue mod 16; ending exactly at hap_len; reaching past it; starting before p_min; wholly outside (L == 0)."""
  rng = np.random.default_rng(seed)
  i = np.arange(n)
  kind = i % 10
  long_l = rng.integers(300, 600, n)
  L = np.choose(np.minimum(kind, 5), [np.full(n, 1), np.full(n, 15), np.full(n, 16), np.full(n, 17), long_l, long_l])
  L = np.maximum(L, rlen)
  start = (rng.integers(0, hap_len - 700, n) // 16) * 16 + (i + i // 10) % 16
  start = np.where(kind == 5, hap_len - L, start)                       # ends exactly at hap_len
  start = np.where(kind == 6, hap_len - rng.integers(1, 250, n), start)  # reaches past it
  start = np.where(kind == 7, -rng.integers(1, 250, n), start)           # starts before p_min
  start = np.where(kind == 8, hap_len + 5 + rng.integers(0, 50, n), start)   # wholly outside
  pos0 = (p_min + start).astype(np.int64)
  pos1 = (pos0 + L - rlen).astype(np.int64)
  return rng.integers(0, 2, n).astype(np.int8), pos0, pos1


def _thin_and_compare(ctx, tid, slot, hap, p_min, fo0, pos0, pos1, rlen, T, seed, unit_key, t0=0):
  n = len(fo0)
  idx, b, seen, kept = GR.thin(hap, p_min, fo0, pos0, pos1, rlen, T, seed, unit_key, t0=t0)
  ctx.templates_import(tid, n, rlen, fo0, pos0, pos1)
  if t0:
    return idx   # (a part thinned on its own has its own indices: only the restatement is asked)
  got_n, got_seen, got_kept = ctx.gc_thin(tid, slot, T, seed, unit_key)
  assert got_n == len(idx) == ctx.template_count(tid)
  R.same(got_seen, seen, 'templates seen per bin')
  R.same(got_kept, kept, 'templates kept per bin')
  e_fo0, e_pos0, e_pos1 = ctx.templates_export(tid)
  R.same(e_fo0, fo0[idx], 'fo0')
  R.same(e_pos0, pos0[idx], 'pos0')
  R.same(e_pos1, pos1[idx], 'pos1')
  return idx


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]


@pytest.mark.parametrize('curve', ['step', 'ramp'])
@pytest.mark.parametrize('n', SIZES)
def test_imported_sets_equal_the_restatement(ctx, hap_a, n, curve):
  hap, p_min = hap_a
  _, T = _curve(curve)
  fo0, pos0, pos1 = _templates(n, len(hap), p_min, 1, 100 + n)
  idx = _thin_and_compare(ctx, 50, SLOT_A, hap, p_min, fo0, pos0, pos1, 1, T, SEED, UNIT_KEY)
  if n >= 63:
    assert 0 < len(idx) < n
    b = GR.bins(hap, p_min, pos0, pos1, 1)
    assert b.min() == 0 and b.max() == 100 and len(np.unique(b)) > 20   # (1-byte spans: bins 0 and 100)


@pytest.mark.parametrize('n', [257, 4097])
def test_imported_sets_read_length_150(ctx, hap_a, n):
  hap, p_min = hap_a
  _, T = _curve('step')
  fo0, pos0, pos1 = _templates(n, len(hap), p_min, 150, 7 + n)
  idx = _thin_and_compare(ctx, 50, SLOT_A, hap, p_min, fo0, pos0, pos1, 150, T, SEED, UNIT_KEY)
  assert 0 < len(idx) < n


@pytest.mark.parametrize('n', [65, 2049])
def test_haplotype_shorter_than_its_span(ctx, hap_b, n):
  """hap_len < p_max - p_min: spans sampled up to p_max end past the haplotype's bytes and are clamped."""
  hap, p_min = hap_b
  _, T = _curve('ramp')
  fo0, pos0, pos1 = _templates(n, len(hap), p_min, 1, 300 + n)
  # the last positions a sampler could draw: up to p_max = p_min + hap_len + 4
  pos0[::7] = p_min + len(hap) + 4 - np.arange(len(pos0[::7])) % 9
  pos1[::7] = pos0[::7] + 100
  idx = _thin_and_compare(ctx, 51, SLOT_B, hap, p_min, fo0, pos0, pos1, 1, T, SEED, 5)
  assert 0 < len(idx) < n


def test_extremes(ctx, native, hap_a):
  hap, p_min = hap_a
  n = 3000
  fo0, pos0, pos1 = _templates(n, len(hap), p_min, 1, 11)
  # every weight 1: nothing changes
  idx = _thin_and_compare(ctx, 52, SLOT_A, hap, p_min, fo0, pos0, pos1, 1, FULL, SEED, UNIT_KEY)
  assert len(idx) == n
  # every threshold 0: an empty set, and its emission writes nothing
  zero = np.zeros(GR.N_BINS, np.uint64)
  idx = _thin_and_compare(ctx, 52, SLOT_A, hap, p_min, fo0, pos0, pos1, 1, zero, SEED, UNIT_KEY)
  assert len(idx) == 0
  ctx.reset_output()
  ctx.use_templates(52)
  assert ctx.emit_reads(SLOT_A, 'S:0:0', '1', 0, True, 9) == (0, 0, 0)
  assert ctx.output_size() == (0, 0)
  # only bin 100 open: the templates inside the all-'G' stretch (which no variant of haplotype A precedes closely:
  # its offset in the haplotype is the reference's + 7 - 33) and nothing else
  only = zero.copy()
  only[100] = 1 << 32
  g0, g1 = G_RUN[0] + 7 - 33, G_RUN[1] + 7 - 33
  assert hap[g0:g1] == b'G' * (g1 - g0)
  rng = np.random.default_rng(3)
  L = rng.integers(15, 400, n)
  start = np.where(np.arange(n) % 3 == 0, g0 + rng.integers(0, g1 - g0 - 400, n), rng.integers(0, len(hap) - 400, n))
  pos0 = (p_min + start).astype(np.int64)
  pos1 = pos0 + L - 1
  idx = _thin_and_compare(ctx, 52, SLOT_A, hap, p_min, fo0, pos0, pos1, 1, only, SEED, UNIT_KEY)
  inside = (start >= g0) & (start + L <= g1)
  b = GR.bins(hap, p_min, pos0, pos1, 1)
  assert inside.sum() >= n // 3 and np.all(b[inside] == 100) and np.array_equal(idx, np.flatnonzero(b == 100))
  assert len(idx) < n // 2


def test_geometry_independence_is_per_set(ctx, hap_a):
  """A template's draw is keyed by its index in the set handed in: the halves of a set thinned as sets of their own
  keep other templates than the whole does, unless the second half's indices are offset.  (Why the distributed
  driver thins before it slices.)"""
  hap, p_min = hap_a
  _, T = _curve('ramp')
  n, h = 2500, 1237
  fo0, pos0, pos1 = _templates(n, len(hap), p_min, 1, 21)
  whole = _thin_and_compare(ctx, 53, SLOT_A, hap, p_min, fo0, pos0, pos1, 1, T, SEED, UNIT_KEY)
  a = _thin_and_compare(ctx, 54, SLOT_A, hap, p_min, fo0[:h], pos0[:h], pos1[:h], 1, T, SEED, UNIT_KEY)
  b0 = _thin_and_compare(ctx, 55, SLOT_A, hap, p_min, fo0[h:], pos0[h:], pos1[h:], 1, T, SEED, UNIT_KEY)
  b_off = _thin_and_compare(ctx, 55, SLOT_A, hap, p_min, fo0[h:], pos0[h:], pos1[h:], 1, T, SEED, UNIT_KEY, t0=h)
  assert np.array_equal(whole, np.concatenate([a, b_off + h]))
  assert not np.array_equal(whole, np.concatenate([a, b0 + h]))


# ---- sampled sets: the start nodes ride along ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sampled(ctx, native):
  from mitty_amd import synth
  seq = synth.contig(90_000, 41, n_gaps=False)
  seq = seq[:20000] + b'N' * 600 + seq[20600:]
  soa = synth.copies_soa(synth.variants(seq, 42))[1]
  ctx.upload_contig(CID + 2, seq)
  n_nodes, p_min, p_max = ctx.build_haplotype(SLOT_S, CID + 2, 1, soa)
  assert n_nodes > 20
  hap = ctx.get_nodes(SLOT_S, n_nodes)[4]
  p, _ = native.read_model_params(150, 30.0)
  return hap, p_min, p, G.model('hiseq-X-v2.5-Garvan')['cum_tlen']


def _emit(ctx, tid, use_async):
  ctx.reset_output()
  ctx.use_templates(tid)
  if use_async:
    ctx.emit_async(SLOT_S, 'S:0:3', '2', 1, True, 4242)
    res = ctx.emit_collect()
    assert len(res) == 1
    res = res[0]
  else:
    res = ctx.emit_reads(SLOT_S, 'S:0:3', '2', 1, True, 4242)
  return tuple(res), ctx.fetch_output()


@pytest.mark.parametrize('use_async', [False, True])
def test_sampled_set_thinned_on_the_device_emits_what_the_restated_set_does(ctx, sampled, use_async):
  hap, p_min, p, cum_tlen = sampled
  _, T = _curve('step')
  ns = ctx.sample_units([60, 61], [SLOT_S, SLOT_S], [1234, 1234], p, 150, cum_tlen)
  assert ns[0] == ns[1] > 1000
  fo0, pos0, pos1 = (x.copy() for x in ctx.templates_export(61))
  idx, _, seen, kept = GR.thin(hap, p_min, fo0, pos0, pos1, 150, T, SEED, 1234)
  assert 0 < len(idx) < len(fo0)
  n, d_seen, d_kept = ctx.gc_thin(60, SLOT_S, T, SEED, 1234)
  assert n == len(idx)
  R.same(d_seen, seen, 'templates seen per bin')
  R.same(d_kept, kept, 'templates kept per bin')
  for got, want, what in zip(ctx.templates_export(60), (fo0[idx], pos0[idx], pos1[idx]), ('fo0', 'pos0', 'pos1')):
    R.same(got, want, what)
  res_b, (b1, b2) = _emit(ctx, 60, use_async)
  ctx.templates_import(62, len(idx), 150, fo0[idx], pos0[idx], pos1[idx])   # (no start nodes: the writer searches)
  res_a, (a1, a2) = _emit(ctx, 62, use_async)
  assert res_a == res_b and 0 < res_b[0] <= len(idx) and res_b[1] == len(b1) and res_b[2] == len(b2)
  G.check_same(b1, a1, 'file 1 of the device-thinned set')
  G.check_same(b2, a2, 'file 2 of the device-thinned set')
  ctx.reset_output()


def test_engine_two_pass_path_thins_as_the_queued_path(native):
  """Engine.run_units thins before use_templates on both of its emission flows (emit_mode 0: units queued with no
  host wait; 2: measure passes ahead of their writers): the same bytes, totals and per-bin sums."""
  from mitty_amd import synth
  from mitty_amd.engine import Engine
  seq = synth.contig(60_000, 51, n_gaps=False)
  copies = synth.copies_soa(synth.variants(seq, 52))
  p, passes = native.read_model_params(150, 30.0)
  units = [(ps, ri, cpy, s) for ps, (ri, cpy, s) in enumerate(native.work_units(5, [2], 3))]
  w, _ = _curve('step')
  got = []
  for mode in (0, 2):
    eng = Engine(0, mode)
    try:
      eng.set_gc_bias(w, 17)
      eng.load_region(0, ('5', 0, len(seq)), seq)
      res = eng.run_units(units, lambda r, c: copies[c], p, 150, G.model(MODEL)['cum_tlen'], 'SYN')
      got.append((res, eng.ctx.fetch_output(), list(eng.gc_seen), list(eng.gc_kept)))
    finally:
      eng.close()
  assert got[0] == got[1]
  res, (d1, d2), seen, kept = got[0]
  assert len(res) == 6 and sum(r[0] for r in res) == sum(kept) and 0 < sum(kept) < sum(seen) and len(d1) > 0


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors(ctx, native, hap_a):
  hap, p_min = hap_a
  rng = np.random.default_rng(31)   # (this set is emitted: every read inside the haplotype)
  pos0 = p_min + rng.integers(0, len(hap) - 1000, 500).astype(np.int64)
  fo0, pos1 = rng.integers(0, 2, 500).astype(np.int8), pos0 + rng.integers(0, 400, 500)
  ctx.templates_import(56, 500, 150, fo0, pos0, pos1)
  over = FULL.copy()
  over[17] = (1 << 32) + 1
  with pytest.raises(ValueError, match='2\\^32'):
    ctx.gc_thin(56, SLOT_A, over, 1, 2)
  with pytest.raises(ValueError):
    ctx.gc_thin(56, SLOT_A, FULL[:100], 1, 2)
  with pytest.raises(native.NativeError, match='unknown template set'):
    ctx.gc_thin(777777, SLOT_A, FULL, 1, 2)
  with pytest.raises(native.NativeError, match='empty haplotype slot'):
    ctx.gc_thin(56, 63, FULL, 1, 2)
  assert ctx.template_count(56) == 500        # (the refused calls changed nothing)
  ctx.reset_output()
  ctx.use_templates(56)
  ctx.emit_prepare(SLOT_A, 'S:0:0', '1', 0, True, 9)
  with pytest.raises(native.NativeError, match='already being emitted') as e:
    ctx.gc_thin(56, SLOT_A, FULL, 1, 2)
  assert 'error {}'.format(native.MH_E_STATE) in str(e.value)
  kept, b1, b2 = ctx.emit_reads(SLOT_A, 'S:0:0', '1', 0, True, 9)   # (the prepared unit is written as it was)
  assert kept > 0 and ctx.template_count(56) == 500
  ctx.sync()
  ctx.reset_output()


# ---- end to end on the golden genome -----------------------------------------------------------------------------------
MODEL = 'hiseq-X-v2.5-Garvan'


def _run(tmp_path, name, **kw):
  from mitty_amd.readmodel import get_read_model
  from mitty_amd.simulation import readgenerate
  c = G.load_json('e2e_config.json')[MODEL]
  mod, mdl = get_read_model(MODEL + '.pkl')
  f1, f2 = str(tmp_path / (name + '.r1.fq')), str(tmp_path / (name + '.r2.fq'))
  st = readgenerate.process_multi_threaded(G.path(c['fasta']), G.path(c['vcf']), c['sample'], G.path(c['bed']), mod,
                                           mdl, c['coverage'], f1, f2, seed=c['seed'], **kw)
  return st, open(f1, 'rb').read(), open(f2, 'rb').read()


def test_e2e_flat_curve_is_the_golden_output(native, tmp_path):
  w, _ = _curve('flat')
  st, d1, d2 = _run(tmp_path, 'flat', gc_bias=w)
  G.check_same(d1, G.fastq_bytes('e2e_{}.r1.fq.gz'.format(MODEL)))
  G.check_same(d2, G.fastq_bytes('e2e_{}.r2.fq.gz'.format(MODEL)))
  assert st['gc_seen'] == st['gc_kept'] == st['templates'] > 0 and st['gc_bin_seen'] == st['gc_bin_kept']
  plain, p1, p2 = _run(tmp_path, 'plain')
  assert 'gc_seen' not in plain and plain['templates'] == st['templates'] and (p1, p2) == (d1, d2)


def _restated_sums(native, T, gc_seed):
  """The restatement's seen / kept sums over the job's units, each sampled and exported through a context here."""
  from mitty_amd.engine import Engine
  from mitty_amd.lib import fasta as mfasta, vcfio
  from mitty_amd.readmodel import get_read_model
  from mitty_amd.simulation import readgenerate
  c = G.load_json('e2e_config.json')[MODEL]
  mod, mdl = get_read_model(MODEL + '.pkl')
  rm = mod.read_model_params(mdl, c['coverage'])
  vdf = vcfio.load_variants_soa(G.path(c['vcf']), c['sample'], G.path(c['bed']))
  seqs = mfasta.read_fasta(G.path(c['fasta']))
  seen, kept = np.zeros(GR.N_BINS, np.int64), np.zeros(GR.N_BINS, np.int64)
  eng = Engine(0)
  try:
    for ri, reg in enumerate(vdf):
      eng.load_region(ri, reg['region'], mfasta.fetch(seqs, *reg['region']))
    for u in readgenerate.get_data_for_workers(rm, vdf, c['seed']):
      ri, cpy, useed = u['region_idx'], u['region_cpy'], u['rng_seed']
      slot, n_nodes, p_min, _ = eng.haplotype(ri, cpy, vdf[ri]['copies'][cpy])
      hap = eng.ctx.get_nodes(slot, n_nodes)[4]
      eng.ctx.sample_units([7], [slot], [useed], rm['p'], rm['rlen'], rm['cum_tlen'])
      fo0, pos0, pos1 = eng.ctx.templates_export(7)
      _, _, s, k = GR.thin(hap, p_min, fo0, pos0, pos1, int(rm['rlen']), T, gc_seed, useed)
      seen += s
      kept += k
  finally:
    eng.close()
  return seen, kept


def test_e2e_step_curve_counts_and_distributed_driver(native, tmp_path):
  from mitty_amd import distributed as D
  from mitty_amd.readmodel import get_read_model
  w, T = _curve('step')
  c = G.load_json('e2e_config.json')[MODEL]
  seen, kept = _restated_sums(native, T, c['seed'])
  assert 0 < kept.sum() < seen.sum()
  st, d1, d2 = _run(tmp_path, 'step', gc_bias=w)
  assert st['gc_bin_seen'] == seen.tolist() and st['gc_bin_kept'] == kept.tolist()
  assert st['gc_seen'] == int(seen.sum()) and st['gc_kept'] == int(kept.sum()) == st['templates']
  assert 0 < len(d1) < len(G.fastq_bytes('e2e_{}.r1.fq.gz'.format(MODEL)))
  # another seed for the draws: another thinning of the same sampled sets
  seen2, kept2 = _restated_sums(native, T, 99)
  st2, e1, _ = _run(tmp_path, 'step99', gc_bias=w, gc_seed=99)
  assert st2['gc_bin_kept'] == kept2.tolist() and seen2.tolist() == seen.tolist() and e1 != d1
  # the distributed driver with no process group (one rank): the same files
  mod, mdl = get_read_model(MODEL + '.pkl')
  g1, g2 = str(tmp_path / 'dist.r1.fq'), str(tmp_path / 'dist.r2.fq')
  ds = D.generate_reads_distributed(G.path(c['fasta']), G.path(c['vcf']), c['sample'], G.path(c['bed']), mod, mdl,
                                    c['coverage'], g1, g2, seed=c['seed'], backend=D.DeviceBackend(0), gc_bias=w)
  G.check_same(open(g1, 'rb').read(), d1, 'file 1 of the distributed driver')
  G.check_same(open(g2, 'rb').read(), d2, 'file 2 of the distributed driver')
  assert ds['gc_bin_kept'] == kept.tolist() and ds['gc_bin_seen'] == seen.tolist() and ds['templates'] == st['templates']
