"""filter-bam (a stub in the reference, mitty/cli.py:207-221): keep or discard the records of a BAM of simulated reads
by how wrong their alignment is.  The BAM is streamed through the host reader into the device filter
(mh_bamread.cpp -> mh_filter.hip), which scores each record as mq-plot does, compacts the kept ones in HBM, deflates
them into BGZF blocks and hands them back for the file: one pass, input order preserved."""
import logging
import time

from mitty_amd.benchmarking.god_aligner import __version__
from mitty_amd.lib import bamsession
from mitty_amd.lib.bamsession import CHUNK_BYTES

logger = logging.getLogger(__name__)

PG_ID = 'mitty-filter-bam'


def output_header_text(text, command_line):
  """The input header text with one @PG line appended (a missing final newline supplied first).  The ID is
  mitty-filter-bam, or mitty-filter-bam.1, .2, ... when the text already has that ID.  @HD and its SO are left as they
  are: the records keep their order."""
  if text and not text.endswith('\n'):
    text += '\n'
  ids = set()
  for line in text.split('\n'):
    if line.startswith('@PG'):
      ids.update(f[3:] for f in line.split('\t')[1:] if f.startswith('ID:'))
  pg_id, k = PG_ID, 0
  while pg_id in ids:
    k += 1
    pg_id = '{}.{}'.format(PG_ID, k)
  return text + '@PG\tID:{}\tPN:mitty\tVN:{}\tCL:{}\n'.format(pg_id, __version__, command_line)


def check_ranges(max_d, min_derr, max_derr, min_mq, max_mq):
  """(d_lo, d_hi) of the |d_err| range (max_derr None: max_d); ValueError naming the option that is out of range."""
  if not 0 <= max_d <= 1 << 20:
    raise ValueError('--max-d must be 0..2^20')
  d_hi = max_d if max_derr is None else max_derr
  if min_derr < 0:
    raise ValueError('--min-derr must be 0 or more')
  if d_hi > max_d:
    raise ValueError('--max-derr must be at most --max-d (|d_err| is clamped there)')
  if min_derr > d_hi:
    raise ValueError('--min-derr must be at most --max-derr')
  if not 0 <= min_mq <= max_mq <= 255:
    raise ValueError('need 0 <= --min-mq <= --max-mq <= 255')
  return min_derr, d_hi


def filter_bam(bam_in, bam_out, max_d=200, strict=False, sample_name=None, min_derr=1, max_derr=None, min_mq=0,
               max_mq=255, unscored='drop', processes=2, device=0, gpu_inflate=False, chunk_bytes=CHUNK_BYTES,
               command_line=None):
  """Writes to `bam_out` the records of `bam_in` with min_derr <= |d_err| <= max_derr (None: max_d; |d_err| == max_d
  means another chromosome, or max_d or further away) and min_mq <= MAPQ <= max_mq; records that are not scored
  (unplaced, or not of `sample_name`) are kept when unscored == 'keep'.  The defaults keep exactly the records mq-plot
  counts outside its d_err = 0 column.  Returns the counts dict (Context.FILTER_COUNTS)."""
  if unscored not in ('drop', 'keep'):
    raise ValueError("unscored must be 'drop' or 'keep'")
  d_lo, d_hi = check_ranges(max_d, min_derr, max_derr, min_mq, max_mq)
  if command_line is None:
    command_line = 'filter-bam {} {} --max-d {}{} --min-derr {} --max-derr {} --min-mq {} --max-mq {} --unscored {}{}'.format(
      bam_in, bam_out, max_d, ' --strict-scoring' if strict else '', d_lo, d_hi, min_mq, max_mq, unscored,
      ' --sample-name {}'.format(sample_name) if sample_name else '')
  t0 = time.time()
  with bamsession.opened(bam_in, processes, device, gpu_inflate) as (bam, ctx, _):
    ctx.filter_begin(bam.names_blob, bam.lengths, output_header_text(bam.text, command_line), bam_out, max_d=max_d,
                     strict=strict, sample_prefix=sample_name, d_lo=d_lo, d_hi=d_hi, mq_lo=min_mq, mq_hi=max_mq,
                     keep_unscored=unscored == 'keep')
    try:
      bamsession.feed(bam, ctx.filter_add_raw, chunk_bytes)
      counts = ctx.filter_finish()
    except BaseException:
      ctx.filter_abort()
      raise
  dt = max(time.time() - t0, 1e-9)
  logger.debug('{} of {} records kept in {:0.2f}s ({:0.2f} records/sec); {}'.format(counts['kept'], counts['seen'], dt,
                                                                                   counts['seen'] / dt, counts))
  return counts
