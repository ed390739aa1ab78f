"""bq: the base-quality distribution per contig of a BAM (reference mitty/empirical/bq.py).  The per-record loop
(:28-33, per contig of the header's first 24 by :38-54) runs on the device: the host reader streams the file
(mh_bamread.cpp) into the read model's histogram pass with a table per contig (mh_model.hip)."""
import logging
import pickle
import time

from mitty_amd.lib import bamsession
from mitty_amd.lib.bamsession import CHUNK_BYTES, MAX_CHROMS   # (:42)

logger = logging.getLogger(__name__)


def _results(ctx, sq):
  bq_data = {'seq_info': sq}
  counts = None
  for i, s in enumerate(sq[:MAX_CHROMS]):
    bq_data[s['SN']], counts = ctx.bq_result(i)
  return bq_data, counts


def count_bam(bam_fname, threads=4, device=0, chunk_bytes=CHUNK_BYTES, gpu_inflate=False):
  """(bq_data dict, counts) of `bam_fname`: chunk k is counted on the device while the reader inflates chunk k + 1.
  gpu_inflate: the BGZF blocks are inflated on `device` instead of on the `threads` pool."""
  with bamsession.opened(bam_fname, threads, device, gpu_inflate, bamsession.header_sq) as (bam, ctx, sq):
    ctx.bq_begin(len(sq))
    bamsession.feed(bam, ctx.bq_add_raw, chunk_bytes)
    return _results(ctx, sq)


def from_store(ctx, sq):
  """(bq_data dict, counts) of the context's own god-aligner record store, no file in between."""
  ctx.bq_begin(len(sq))
  ctx.bq_add_store()
  return _results(ctx, sq)


def process_bam_parallel(bam_fname, pkl, threads=4, device=0, chunk_bytes=CHUNK_BYTES, gpu_inflate=False):
  """Write the per-contig (500, 100) uint64 matrices of `bam_fname` to `pkl` and return them (:38-54)."""
  t0 = time.time()
  bq_data, counts = count_bam(bam_fname, threads, device, chunk_bytes, gpu_inflate)
  dt = max(time.time() - t0, 1e-9)
  logger.debug('Processed {} records ({} r/s); {}'.format(counts and counts['seen'], (counts or {}).get('seen', 0) / dt,
                                                          counts))
  with open(pkl, 'wb') as fp:
    pickle.dump(bq_data, fp)
  return bq_data
