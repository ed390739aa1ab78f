"""The pass both scorers share: a BAM file streamed through the host reader into the device scoring kernel
(mh_bamread.cpp -> mh_score.hip), which fills the MQ matrix and the d_err matrix together."""
import logging
import time

from mitty_amd.lib import bamsession
from mitty_amd.lib.bamsession import CHUNK_BYTES

logger = logging.getLogger(__name__)


def score_bam(bam_fname, max_d=200, max_v_len=200, strict=False, sample_name=None, processes=2, device=0,
              chunk_bytes=CHUNK_BYTES, gpu_inflate=False):
  """(mq_mat, d_err_mat, counts) of every record of `bam_fname` placed on a reference (mq.py:50-68, derr.py:53-76
  summed over the header's @SQ lines).  `processes` sizes the inflate pool; chunk k is scored on the device while the
  reader inflates chunk k + 1.  gpu_inflate: the BGZF blocks are inflated on `device` instead of on the pool."""
  t0 = time.time()
  with bamsession.opened(bam_fname, processes, device, gpu_inflate) as (bam, ctx, _):
    ctx.score_begin(bam.names_blob, max_d, max_v_len, strict, sample_name)
    bamsession.feed(bam, ctx.score_add_raw, chunk_bytes)
    mq_mat, d_err_mat, counts = ctx.score_result()
  dt = max(time.time() - t0, 1e-9)
  logger.debug('{} records scored in {:0.2f}s ({:0.2f} records/sec); {}'.format(counts['scored'], dt,
                                                                                 counts['scored'] / dt, counts))
  return mq_mat, d_err_mat, counts
