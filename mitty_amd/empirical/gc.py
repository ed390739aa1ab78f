"""gc-cov: GC content against coverage per block of the reference (reference mitty/empirical/gc.py).  The pileup of
every block (:37-38) is replaced by one pass over the BAM on the device (mh_cov.hip): a depth track over the header's
first 24 contigs and per-block sums; the FASTA's blocks are counted there too (:32-36).  The reference's float
expressions are then applied here to the integer counts.

Per block [a, b) the reference's `[b.n for b in pileup(region)]` (pysam's defaults: stepper 'all', truncate=False)
walks every column of every record that overlaps the block, so sum(cov_l) is the records' summed reference spans S and
len(cov_l) the covered columns U = covered positions inside the block + the overhang of the overlapping records on
either side.  Three documented divergences from pysam: htslib's max_depth (8000) is not modelled; a FASTA contig that
is missing or whose length differs from the header's LN is an error (pysam would clip the region); a record without a
reference span (no CIGAR, or only I/S/H/P) contributes nothing.
"""
import logging
import pickle
import time

import numpy as np

from mitty_amd import _native
from mitty_amd.lib import bamsession
from mitty_amd.lib.bamsession import CHUNK_BYTES, MAX_CHROMS   # (:66)

logger = logging.getLogger(__name__)

DTYPE = [('gc', float), ('coverage', float)]
# the contig id the one resident contig is uploaded under: negative, so that it is none of an Engine's regions
# (Engine.load_region uploads region ri as contig ri >= 0); released when the counts are done
SCRATCH_CONTIG_ID = -1


def block_bounds(ln, block_len):
  """(a, b) of the blocks of a contig of length ln: range(1, ln, block_len) as 0-based half-open intervals."""
  a = np.arange(len(range(1, ln, block_len)), dtype=np.int64) * block_len
  return a, np.minimum(a + block_len + 1, ln)


def gc_cov_from_counts(ln, block_len, n_n, n_gc, covered, span_sum, min_pos, max_end):
  """The structured array of gc_and_coverage_for_chromosome (:56-59) from a contig's per-block integers.
  np.true_divide of int64 values is the correctly rounded quotient, as Python's float(x) / y is."""
  a, b = block_bounds(ln, block_len)
  n = b - a
  n_n, n_gc, covered, span_sum, min_pos, max_end = (np.asarray(x).astype(np.int64) for x in
                                                    (n_n, n_gc, covered, span_sum, min_pos, max_end))
  out = np.empty(len(a), dtype=DTYPE)
  masked = np.true_divide(n_n, n) > 0.1                       # (:33) probably centromere or telomere
  u = covered + np.maximum(0, a - min_pos) + np.maximum(0, max_end - b)   # (no record: min_pos is the largest int64)
  out['gc'] = np.where(masked, np.nan, np.true_divide(n_gc, n))          # (:36)
  out['coverage'] = np.where(masked, np.nan, np.true_divide(span_sum, np.maximum(u, 1)))   # (:38)
  return out


def check_fasta(sq, seqs):
  """Every visited contig is in the FASTA with the header's length, else ValueError naming it (pysam would clip)."""
  for s in sq[:MAX_CHROMS]:
    seq = seqs.get(s['SN'])
    if seq is None:
      raise ValueError('contig {} of the BAM header is not in the FASTA'.format(s['SN']))
    if len(seq) != s['LN']:
      raise ValueError('contig {}: {} bases in the FASTA, LN:{} in the BAM header'.format(s['SN'], len(seq), s['LN']))


def _upload_gc(ctx, sq, seqs, contig_id=SCRATCH_CONTIG_ID):
  """N / GC counts of the visited contigs, one upload at a time under `contig_id`, which is released at the end (so
  it must be an id the context's owner does not use)."""
  check_fasta(sq, seqs)
  try:
    for i, s in enumerate(sq[:MAX_CHROMS]):
      ctx.upload_contig(contig_id, seqs[s['SN']])
      ctx.cov_gc(i, contig_id)
  finally:
    ctx.release_contig(contig_id)


def _results(ctx, sq, block_len):
  gc_cov = {'block_len': block_len, 'seq_info': sq}
  counts = None
  for i, s in enumerate(sq[:MAX_CHROMS]):
    r, counts = ctx.cov_result(i)
    gc_cov[s['SN']] = gc_cov_from_counts(s['LN'], block_len, **r)
  return gc_cov, counts


def count_bam(bam_fname, fasta_fname, block_len=10000, threads=4, device=0, chunk_bytes=CHUNK_BYTES,
              gpu_inflate=False):
  """(gc_cov dict, counts) of `bam_fname`: chunk k is counted on the device while the reader inflates chunk k + 1.
  gpu_inflate: the BGZF blocks are inflated on `device` instead of on the `threads` pool."""
  def header_and_fasta(bam):   # (before a device is touched)
    sq = bamsession.header_sq(bam)
    seqs = _native.read_fasta(fasta_fname, [s['SN'] for s in sq[:MAX_CHROMS]])
    check_fasta(sq, seqs)
    return sq, seqs

  with bamsession.opened(bam_fname, threads, device, gpu_inflate, header_and_fasta) as (bam, ctx, (sq, seqs)):
    ctx.cov_begin(bam.lengths, block_len)
    _upload_gc(ctx, sq, seqs)
    bamsession.feed(bam, ctx.cov_add_raw, chunk_bytes)
    return _results(ctx, sq, block_len)


def from_store(ctx, sq, seqs, block_len=10000, contig_id=SCRATCH_CONTIG_ID):
  """(gc_cov dict, counts) of the context's own god-aligner record store (bam_set_refs / bam_add_fastq /
  bam_add_output), no file in between.  sq: the @SQ list (dicts with SN and LN, as bam_set_refs got them); seqs:
  {SN: bytes} of the reference.  The reference goes up one contig at a time under `contig_id` and is released again:
  the default is negative and so none of an Engine's regions (contig ri is region ri's reference there); a caller
  that uploads contigs under ids of its own passes one it does not use."""
  check_fasta(sq, seqs)
  ctx.cov_begin([s['LN'] for s in sq], block_len)
  _upload_gc(ctx, sq, seqs, contig_id)
  ctx.cov_add_store()
  return _results(ctx, sq, block_len)


def process_bam_parallel(bam_fname, fasta_fname, pkl, block_len=10000, threads=4, device=0, chunk_bytes=CHUNK_BYTES,
                         gpu_inflate=False):
  """Write the GC / coverage arrays of `bam_fname` to `pkl` and return them (:62-78)."""
  t0 = time.time()
  gc_cov, counts = count_bam(bam_fname, fasta_fname, block_len, threads, device, chunk_bytes, gpu_inflate)
  dt = max(time.time() - t0, 1e-9)
  logger.debug('Processed {} records ({} r/s); {}'.format(counts and counts['seen'], (counts or {}).get('seen', 0) / dt,
                                                          counts))
  with open(pkl, 'wb') as fp:
    pickle.dump(gc_cov, fp)
  return gc_cov
