"""What the drivers that stream a BAM file into a device session share (score, bam2illumina, bq, gc-cov)."""
import contextlib

from mitty_amd import _native
from mitty_amd.benchmarking.god_aligner import seq_info

CHUNK_BYTES = 64 << 20   # uncompressed record bytes per upload
MAX_CHROMS = 24          # the reference's loops visit the header's first 24 contigs


def header_sq(bam):
  """The @SQ list of an open BamFile (seq_info); ValueError when the header text disagrees with the reference list."""
  sq = seq_info(bam.text, bam.names, bam.lengths)
  if [(s['SN'], s['LN']) for s in sq] != list(zip(bam.names, bam.lengths)):
    raise ValueError('the @SQ lines of the header text are not the BAM\'s reference list')
  return sq


@contextlib.contextmanager
def opened(bam_fname, threads, device=0, gpu_inflate=False, check=None):
  """(bam, ctx, checked): the BamFile read by `threads` inflate threads (gpu_inflate: its BGZF blocks are inflated on
  `device` instead) and a Context on `device`; the context is closed first, then the file.  check(bam) runs before the
  context is made (a bad header or FASTA fails before a device is touched); its value is `checked`."""
  bam = _native.BamFile(bam_fname, threads=max(1, int(threads)), device=device if gpu_inflate else None)
  try:
    checked = check(bam) if check else None
    ctx = _native.Context(device)
    try:
      yield bam, ctx, checked
    finally:
      ctx.close()
  finally:
    bam.close()


def feed(bam, add_raw, chunk_bytes=CHUNK_BYTES):
  """Every record of the file through add_raw: the device works on chunk k while the reader inflates chunk k + 1."""
  while True:
    recs, nbytes, roff, n = bam.next_raw(chunk_bytes)
    if n == 0:
      break
    add_raw(recs, nbytes, roff, n)
