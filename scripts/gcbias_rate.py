"""The cost of generate-reads --gc-bias on a chr1-sized unit of the synthetic genome (mitty_amd/synth.py):
  (a) thin     mh_gc_thin alone per unit: a host clock around the synchronous call on a freshly sampled set, a warm-up
               then --reps repetitions (min - max), next to the same unit's measure pass + writer (mh_emit_reads and a
               synchronisation, host clock) in the same process.  Bytes are derived from shapes: the haplotype bytes
               the templates span (sum of L) + 17 B per template read (21 B with start nodes) + as many per kept
               template written; the rate is a gather rate, not a share of the streaming peak.
  (b) generate the whole job (haplotypes spliced, units sampled and written, as bench.py --workload chr1 steps) with a
               flat curve against no curve, alternating in one process, --reps rounds: the thin forces a host wait per
               unit that the default path does not have.
python scripts/gcbias_rate.py [--length 249250621] [--coverage 30] [--reps 3] [--seed 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def note(msg):
  print('gcbias_rate: ' + msg, file=sys.stderr, flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--length', type=int, default=249250621)
  ap.add_argument('--coverage', type=float, default=30.0)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--seed', type=int, default=7)
  a = ap.parse_args()
  from mitty_amd import _native, synth
  from mitty_amd.engine import Engine
  from mitty_amd.readmodel import get_read_model
  from mitty_amd.simulation import gcbias

  _, model = get_read_model('hiseq-X-v2.5-Garvan.pkl')
  rlen = int(model['mean_rlen'])
  p, passes = _native.read_model_params(rlen, a.coverage)
  note('synthetic contig and variants')
  seq = synth.contig(a.length, 1000)
  copies = synth.copies_soa(synth.variants(seq, 2000))
  units = [(ps, ri, cpy, s) for ps, (ri, cpy, s) in enumerate(_native.work_units(a.seed, [2], passes))]
  b = np.arange(gcbias.N_BINS)
  step_w = np.where(b < 45, 1.0, 0.25)
  out = {'length': a.length, 'coverage': a.coverage, 'units': len(units), 'reps': a.reps}
  eng = Engine(0)
  try:
    eng.load_region(0, ('1', 0, a.length), seq)
    for cpy in range(len(copies)):
      eng.upload_variants(0, cpy, copies[cpy])
    ctx = eng.ctx

    # ---- (a) the thin alone, on unit 0 -----------------------------------------------------------------------------
    ps, ri, cpy, useed = units[0]
    slot, n_nodes, p_min, _ = eng.haplotype(ri, cpy, copies[cpy])
    hap_len = len(ctx.get_nodes(slot, n_nodes)[4])
    rows = {}
    for name, w in (('step', step_w), ('flat', np.ones(gcbias.N_BINS))):
      T = gcbias.thresholds(w)
      thin_s, emit_s, shape = [], [], None
      for rep in range(a.reps + 1):   # (rep 0: warm-up)
        ctx.reset_output()
        n = int(ctx.sample_units([9], [slot], [useed], p, rlen, model['cum_tlen'])[0])
        if shape is None:
          _, pos0, pos1 = ctx.templates_export(9)
          s = np.clip(pos0 - p_min, 0, hap_len)
          e = np.minimum(np.maximum(pos1 + rlen - p_min, s), hap_len)
          shape = {'templates': n, 'sum_L': int((e - s).sum())}
        ctx.sync()
        t0 = time.perf_counter()
        kept, _, _ = ctx.gc_thin(9, slot, T, a.seed, useed)
        t1 = time.perf_counter()
        ctx.use_templates(9)
        ctx.emit_reads(slot, 'SYN:0:{}'.format(ps), '1', cpy, True, useed)
        ctx.sync()
        t2 = time.perf_counter()
        if rep:
          thin_s.append(t1 - t0)
          emit_s.append(t2 - t1)
      per_tpl = 21   # fo0 1 + pos0 8 + pos1 8 + start node 4 (a sampled set carries them)
      nbytes = shape['sum_L'] + per_tpl * (shape['templates'] + kept) + shape['templates']   # + the keep flags
      rows[name] = dict(shape, kept=int(kept), bytes=int(nbytes),
                        thin_ms=[round(1e3 * min(thin_s), 3), round(1e3 * max(thin_s), 3)],
                        measure_writer_ms=[round(1e3 * min(emit_s), 3), round(1e3 * max(emit_s), 3)],
                        gather_GBps=[round(nbytes / max(thin_s) / 1e9, 1), round(nbytes / min(thin_s) / 1e9, 1)])
      note('{}: {}'.format(name, rows[name]))
    out['thin'] = rows
    ctx.release_templates(9)

    # ---- (b) the whole job, flat curve against no curve, alternating -----------------------------------------------
    def job():
      eng.drop_haplotypes()
      ctx.reset_output()
      t0 = time.perf_counter()
      eng.run_units(units, lambda r, c: copies[c], p, rlen, model['cum_tlen'], 'SYN', 0, True, 'mitty', lazy=True)
      res = eng.collect()
      ctx.sync()
      return time.perf_counter() - t0, sum(r[1] for r in res)

    gen = {'none': [], 'flat': []}
    for rnd in range(a.reps + 1):   # (round 0: warm-up)
      for name in ('none', 'flat'):
        eng.set_gc_bias(None if name == 'none' else np.ones(gcbias.N_BINS), a.seed)
        dt, kept = job()
        if rnd:
          gen[name].append(dt)
    eng.set_gc_bias(None, a.seed)
    out['generate'] = {k: {'ms': [round(1e3 * min(v), 2), round(1e3 * max(v), 2)],
                           'M_templates_per_s': [round(kept / max(v) / 1e6, 1), round(kept / min(v) / 1e6, 1)]}
                       for k, v in gen.items()}
    out['generate']['kept_templates'] = int(kept)
  finally:
    eng.close()
  print(json.dumps(out))


if __name__ == '__main__':
  main()
