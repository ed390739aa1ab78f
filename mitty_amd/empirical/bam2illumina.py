"""bam2illumina: an empirical read model (base qualities per mate and base position, template lengths) from a BAM
(reference mitty/empirical/bam2illumina.py).  The per-record loop (:17-59, summed over the header's first 24 contigs by
:84-105) runs on the device: the host reader streams the file (mh_bamread.cpp) into the histogram pass (mh_model.hip);
the model's cumulative tables are then computed here with the reference's own NumPy expressions (:110-129)."""
import logging
import pickle
import time

import numpy as np

from mitty_amd import readmodel
from mitty_amd.lib import bamsession
from mitty_amd.lib.bamsession import CHUNK_BYTES

logger = logging.getLogger(__name__)


def count_bam(bam_fname, every=1, min_mq=0, threads=4, max_bq=94, max_bp=300, max_tlen=1000, device=0,
              chunk_bytes=CHUNK_BYTES, gpu_inflate=False):
  """(bq_mat, tlen_mat, counts) of `bam_fname`: chunk k is counted on the device while the reader inflates chunk
  k + 1.  `threads` sizes the inflate pool; gpu_inflate: the BGZF blocks are inflated on `device` instead."""
  with bamsession.opened(bam_fname, threads, device, gpu_inflate) as (bam, ctx, _):
    ctx.model_begin(bam.names_blob.count(b'\0'), every, min_mq, max_bq, max_bp, max_tlen)
    bamsession.feed(bam, ctx.model_add_raw, chunk_bytes)
    return ctx.model_result()


def model_from_counts(bq_mat, tlen_mat, r_cnt, min_rlen, max_rlen, model_description='Test model', min_mq=0):
  """The model dict of bam2illumina.py:110-129 from the summed counts.  min_rlen None: no record was used."""
  cum_bq_mat = np.zeros(bq_mat.shape, dtype=float)
  for p in [0, 1]:
    cum_bq_mat[p, :, :] = bq_mat[p, :, :].cumsum(axis=1) / bq_mat[p, :, :].sum(axis=1).clip(1)[:, None]
  with np.errstate(invalid='ignore', divide='ignore'):   # an empty tlen histogram: all NaN, as the reference's
    cum_tlen = tlen_mat.cumsum() / tlen_mat.sum()
  return {
    'model_class': 'illumina',
    'model_description': model_description,
    'min_mq': min_mq,
    'bq_mat': bq_mat,
    'cum_bq_mat': cum_bq_mat,
    'tlen': tlen_mat,
    'r_cnt': int(r_cnt),
    'cum_tlen': cum_tlen,
    'mean_rlen': max_rlen,   # (:125: the read length used is the longest seen)
    'min_rlen': 1e13 if min_rlen is None else min_rlen,
    'max_rlen': max_rlen
  }


def process_bam_parallel(bam_fname, pkl, model_description='Test model', every=1, min_mq=0, threads=4, max_bq=94,
                         max_bp=300, max_tlen=1000, device=0, chunk_bytes=CHUNK_BYTES, gpu_inflate=False):
  """Write the read model of `bam_fname` to `pkl` (a path ending in .npz: the pickle-free form) and return it."""
  t0 = time.time()
  bq_mat, tlen_mat, counts = count_bam(bam_fname, every, min_mq, threads, max_bq, max_bp, max_tlen, device, chunk_bytes,
                                       gpu_inflate)
  dt = max(time.time() - t0, 1e-9)
  logger.debug('Processed {} templates ({} t/s); {}'.format(counts['used'], counts['used'] / dt, counts))
  model = model_from_counts(bq_mat, tlen_mat, counts['used'], counts['min_rlen'], counts['max_rlen'],
                            model_description, min_mq)
  if pkl.endswith('.npz'):
    readmodel.save_model_npz(model, pkl)
  else:
    with open(pkl, 'wb') as fp:
      pickle.dump(model, fp)
  return model
