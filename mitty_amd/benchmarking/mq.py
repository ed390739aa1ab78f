"""mq-plot (reference mitty/benchmarking/mq.py): score every aligned read of a BAM of simulated reads against its
qname and count reads by (MAPQ, d_err).  The per-record loop of the reference runs as one device pass
(mitty_amd/benchmarking/score.py)."""
import logging

import numpy as np

from mitty_amd.benchmarking.score import score_bam

logger = logging.getLogger(__name__)


def process_bam(bam_fname, max_d=200, strict=False, sample_name=None, processes=2, out_csv=None, device=0,
                gpu_inflate=False):
  """mq.process_bam (mq.py:20-43): mq_mat u64[100, 2 max_d + 1], mq_mat[mapq, d_err + max_d] = reads."""
  mq_mat, _, _ = score_bam(bam_fname, max_d=max_d, strict=strict, sample_name=sample_name, processes=processes,
                           device=device, gpu_inflate=gpu_inflate)
  if out_csv is not None:
    logger.debug('Saving MQ matrix to {}'.format(out_csv))
    np.savetxt(out_csv, mq_mat, delimiter=',', fmt='%d')
  return mq_mat


def compute_p_err(mq_mat, d_margin=0):
  """Per MAPQ row, the fraction of its reads placed further than d_margin from the truth (|d_err| > d_margin); 0 for
  a MAPQ no read has.  The counterpart of the reference's mq.compute_p_err (mq.py:101-105)."""
  half = (mq_mat.shape[1] - 1) // 2
  far = np.abs(np.arange(-half, half + 1)) > d_margin
  total = mq_mat.sum(axis=1).astype(float)
  wrong = mq_mat[:, far].sum(axis=1).astype(float)
  return np.divide(wrong, total, out=np.zeros_like(total), where=total > 0)


def _pyplot():
  """matplotlib.pyplot on the file-only backend, or None when matplotlib is not installed."""
  try:
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    return plt
  except ImportError:
    return None


def plot_mq(mq_mat, plot):
  """A two-panel figure of the MQ matrix: how honest the aligner's MAPQ is (the empirical error rate of each MAPQ, as a
  phred value, against the MAPQ it claimed; marker area by read count) and the matrix itself as a log-count image.
  Returns False, and draws nothing, when matplotlib is not installed."""
  plt = _pyplot()
  if plt is None:
    logger.warning('matplotlib is not installed: {} not drawn (the CSV holds the matrix)'.format(plot))
    return False
  half = (mq_mat.shape[1] - 1) // 2
  reads = mq_mat.sum(axis=1).astype(float)
  used = np.flatnonzero(reads)
  fig, (ax_cal, ax_img) = plt.subplots(1, 2, figsize=(12, 5), constrained_layout=True)
  for margin, colour in ((0, 'tab:blue'), (min(10, half), 'tab:orange')):
    p = compute_p_err(mq_mat, margin)[used]
    floor = 1.0 / np.maximum(reads[used], 1.0)          # no error seen: at best one in the reads seen
    ax_cal.scatter(used, -10 * np.log10(np.maximum(p, floor)), s=10 + 40 * reads[used] / max(reads.max(), 1.0),
                   color=colour, alpha=0.7, label='wrong when |d_err| > {}'.format(margin))
  ax_cal.plot([0, 70], [0, 70], color='0.5', linewidth=1, label='MAPQ as claimed')
  ax_cal.set_xlabel('MAPQ reported')
  ax_cal.set_ylabel('MAPQ observed: -10 log10(fraction wrong)')
  ax_cal.set_xlim(-1, 70)
  ax_cal.legend(loc='upper left', fontsize='small')
  img = ax_img.imshow(np.log10(mq_mat.astype(float) + 1.0), origin='lower', aspect='auto', cmap='viridis',
                      extent=(-half - 0.5, half + 0.5, -0.5, mq_mat.shape[0] - 0.5))
  ax_img.set_xlabel('d_err (bases from the true position; the ends collect everything further)')
  ax_img.set_ylabel('MAPQ reported')
  fig.colorbar(img, ax=ax_img, label='log10(reads + 1)')
  fig.savefig(plot)
  plt.close(fig)
  return True
