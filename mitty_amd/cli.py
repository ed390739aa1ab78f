"""`mitty` command line (reference mitty/cli.py), MI355X build.

Implemented: generate-reads (GPU), corrupt-reads (GPU), god-aligner (GPU), mq-plot and derr-plot (GPU scoring, host
BAM reader; additive --device), bam2illumina (GPU histograms, host BAM reader; additive --device), gc-cov and bq (GPU
depth track, block sums and histograms, host BAM reader; additive --device), all five with the additive --gpu-inflate
(the reader's BGZF blocks inflated on the --device GPU instead of on the host threads), filter-bam (GPU: the
records scored as mq-plot scores them, the kept ones compacted and deflated on the device; a stub in the reference, its
options are this build's), filter-variants (host C++), qname, list-read-models.  Additive options on generate-reads: --device,
--rng {mitty,philox}, --corrupt-seed (fused Philox corruption), --gc-bias CURVE / --gc-seed (the sampled templates
thinned on the GPU by the GC content of the haplotype bytes they span; CURVE from the new gc-bias-model command, which
fits it to a gc-cov result: the reference has neither); on corrupt-reads: --device, --rng {mitty,philox}.  Multi-GPU: launch generate-reads under
`python -m torch.distributed.run --nproc-per-node N -m mitty_amd.cli generate-reads ...` (one process per GPU,
RCCL); the output files are identical to the one-GPU run.  Out of scope for this build (not on the
generate-reads path): describe-read-model (plotting only).
"""
import logging
import os

import click


@click.group()
@click.version_option('2.7.3.dev0+mi355x')
@click.option('-v', '--verbose', type=int, default=0)
def cli(verbose):
  """A genomic data simulator for testing and debugging bio-informatics tools"""
  logging.basicConfig(level=[logging.ERROR, logging.WARNING, logging.INFO, logging.DEBUG][min(verbose, 3)])


@cli.command('filter-variants', short_help='Remove complex variants from VCF')
@click.argument('vcfin', type=click.Path(exists=True))
@click.argument('sample')
@click.argument('bed')
@click.argument('vcfout', type=click.Path())
def filter_vcf(vcfin, sample, bed, vcfout):
  """Subset VCF for given sample, apply BED file and filter out complex variants
   making it suitable to use for read generation (reference cli.py:20-35)"""
  from mitty_amd.lib import vcfio
  vcfio.prepare_variant_file(vcfin, sample, bed, vcfout)


@cli.command('gc-cov')
@click.argument('bam', type=click.Path(exists=True))
@click.argument('fasta', type=click.Path(exists=True))
@click.argument('pkl')
@click.option('-b', '--block-len', type=int, default=10000, help='Block size for GC/cov computation')
@click.option('-t', '--threads', type=int, default=1, help='Threads to use')
@click.option('--device', default=0, help='HIP device ordinal')
@click.option('--gpu-inflate', is_flag=True, help="Inflate the BAM's BGZF blocks on the GPU (additive option)")
def gc_cov(bam, fasta, pkl, block_len, threads, device, gpu_inflate):
  """Calculate GC content vs coverage from a BAM. Save in pickle file (reference cli.py:32-42)"""
  from mitty_amd.empirical import gc
  gc.process_bam_parallel(bam, fasta, pkl, block_len=block_len, threads=threads, device=device,
                          gpu_inflate=gpu_inflate)


@cli.command('bq')
@click.argument('bam', type=click.Path(exists=True))
@click.argument('pkl')
@click.option('-t', '--threads', type=int, default=1, help='Threads to use')
@click.option('--device', default=0, help='HIP device ordinal')
@click.option('--gpu-inflate', is_flag=True, help="Inflate the BAM's BGZF blocks on the GPU (additive option)")
def sample_bq(bam, pkl, threads, device, gpu_inflate):
  """BQ distribution from BAM (reference cli.py:45-51)"""
  from mitty_amd.empirical import bq
  bq.process_bam_parallel(bam, pkl, threads=threads, device=device, gpu_inflate=gpu_inflate)


@cli.command('bam2illumina', short_help='Create read model from BAM file')
@click.argument('bam', type=click.Path(exists=True))
@click.argument('pkl')
@click.argument('desc')
@click.option('--every', type=int, default=1, help='Sample every nth read')
@click.option('--min-mq', type=int, default=0, help='Discard reads with MQ less than this')
@click.option('-t', '--threads', type=int, default=2, help='Threads to use')
@click.option('--max-bp', type=int, default=300, help='Maximum length of read')
@click.option('--max-tlen', type=int, default=1000, help='Maximum size of insert')
@click.option('--device', default=0, help='HIP device ordinal')
@click.option('--gpu-inflate', is_flag=True, help="Inflate the BAM's BGZF blocks on the GPU (additive option)")
def bam2illumina(bam, pkl, desc, every, min_mq, threads, max_bp, max_tlen, device, gpu_inflate):
  """Process BAM file and create an empirical model of template length and base quality
  distribution. The model is saved to a Python pickle file usable by Mitty read generation programs
  (reference cli.py:54-68)."""
  from mitty_amd.empirical import bam2illumina as b2m
  b2m.process_bam_parallel(bam, pkl, model_description=desc, every=max(1, every), min_mq=min_mq,
                           threads=threads, max_bq=94, max_bp=max_bp, max_tlen=max_tlen, device=device,
                           gpu_inflate=gpu_inflate)


@cli.command('list-read-models')
@click.option('-d', type=click.Path(exists=True), help='List models in this directory')
def list_read_models(d):
  """List read models"""
  import glob
  from mitty_amd import readmodel
  if d is None:
    files = [os.path.join(readmodel.BUILTIN_DIR, f) for f in sorted(os.listdir(readmodel.BUILTIN_DIR))]
  else:
    files = glob.glob(os.path.join(d, '*'))
  for f in files:
    try:
      m = readmodel.load_model_file(f)
      name = os.path.basename(f)
      if name.endswith('.npz'):
        name = name[:-4] + '.pkl'
      click.echo('\n----------\n{}:\n{}\n=========='.format(name, m['model_description']))
    except Exception:
      logging.debug('Skipping {}. Not a read model file'.format(f))


@cli.command()
def qname():
  """Display qname format"""
  from mitty_amd.simulation import readgenerate
  click.echo(readgenerate.__qname_format_details__)


def print_qname(ctx, param, value):
  if not value or ctx.resilient_parsing:
    return
  from mitty_amd.simulation import readgenerate
  click.echo(readgenerate.__qname_format_details__)
  ctx.exit()


@cli.command('generate-reads', short_help='Generate simulated reads.')
@click.argument('fasta')
@click.argument('vcf')
@click.argument('sample_name')
@click.argument('bed')
@click.argument('modelfile')
@click.argument('coverage', type=float)
@click.argument('seed', type=int)
@click.argument('fastq1', type=click.Path())
@click.option('--fastq2', type=click.Path())
@click.option('--threads', default=2, help='Accepted for compatibility; the work runs on the GPU')
@click.option('--qname', is_flag=True, callback=print_qname, expose_value=False, is_eager=True,
              help='Print documentation for information encoded in qname')
@click.option('--device', default=0, help='HIP device ordinal')
@click.option('--rng', type=click.Choice(['mitty', 'philox']), default='mitty',
              help='mitty: bit-exact with the reference; philox: counter-based fast mode')
@click.option('--corrupt-seed', type=int, default=None, help='Apply the BQ corruption model while writing')
@click.option('--gc-bias', type=click.Path(), default=None,
              help='Thin the sampled templates by GC content: a curve file made by gc-bias-model (additive option)')
@click.option('--gc-seed', type=int, default=None, help='Seed of the GC-bias draws (default: SEED)')
def generate_reads(fasta, vcf, sample_name, bed, modelfile, coverage, seed, fastq1, fastq2, threads, device, rng,
                   corrupt_seed, gc_bias, gc_seed):
  """Generate simulated reads"""
  from mitty_amd.readmodel import get_read_model
  from mitty_amd.simulation import readgenerate
  if gc_bias is not None:   # (a malformed curve fails here, before any input is parsed or a device touched)
    from mitty_amd.simulation import gcbias
    try:
      gc_bias = gcbias.load_curve(gc_bias)
    except ValueError as e:
      raise click.BadParameter(str(e), param_hint='--gc-bias')
  read_module, model = get_read_model(modelfile)
  if int(os.environ.get('WORLD_SIZE', '1')) > 1:
    import torch
    import torch.distributed as dist
    from mitty_amd import distributed
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
    dist.init_process_group('nccl')
    try:
      stats = distributed.generate_reads_distributed(fasta, vcf, sample_name, bed, read_module, model, coverage,
                                                     fastq1, fastq2, seed=seed, rng=rng, corrupt_seed=corrupt_seed,
                                                     gc_bias=gc_bias, gc_seed=gc_seed)
    finally:
      dist.destroy_process_group()
    logging.info('generate-reads: {}'.format(stats))
    return
  stats = readgenerate.process_multi_threaded(fasta, vcf, sample_name, bed, read_module, model, coverage, fastq1,
                                              fastq2, threads=threads, seed=seed, device=device, rng=rng,
                                              corrupt_seed=corrupt_seed, gc_bias=gc_bias, gc_seed=gc_seed)
  logging.info('generate-reads: {}'.format(stats))


@cli.command('gc-bias-model', short_help='Create a GC-bias curve from a gc-cov result')
@click.argument('gccov_pkl', type=click.Path(exists=True))
@click.argument('curve_json', type=click.Path())
@click.option('--min-blocks', type=int, default=20, help='A GC bin with fewer blocks takes its nearest neighbour\'s mean')
@click.option('--smooth', type=int, default=5, help='Width (odd) of the moving average over the bins')
@click.option('--desc', default='', help='Description stored in the curve file')
def gc_bias_model(gccov_pkl, curve_json, min_blocks, smooth, desc):
  """Turn the pickle written by gc-cov into a GC-bias curve for generate-reads --gc-bias: the mean coverage per
  GC percent, smoothed and scaled to a maximum of 1.

  GCCOV_PKL is unpickled as it is: it is trusted input, so only give this command a file you made with gc-cov."""
  import pickle
  from mitty_amd.simulation import gcbias
  with open(gccov_pkl, 'rb') as fp:
    gc_cov = pickle.load(fp)
  try:
    if not isinstance(gc_cov, dict) or 'seq_info' not in gc_cov:
      raise ValueError('{} is not a gc-cov result (no seq_info)'.format(gccov_pkl))
    w = gcbias.fit_curve(gc_cov, min_blocks=min_blocks, smooth=smooth)
  except ValueError as e:
    raise click.ClickException(str(e))
  gcbias.save_curve(curve_json, w, desc)


@cli.command('corrupt-reads', short_help='Apply corruption model to FASTQ file of reads')
@click.argument('modelfile')
@click.argument('fastq1_in', type=click.Path(exists=True))
@click.argument('fastq1_out', type=click.Path())
@click.argument('seed', type=int)
@click.option('--fastq2-in', type=click.Path(exists=True))
@click.option('--fastq2-out', type=click.Path())
@click.option('--threads', default=2)
@click.option('--device', default=0, help='HIP device ordinal')
@click.option('--rng', type=click.Choice(['mitty', 'philox']), default='mitty',
              help='mitty: the reference\'s --threads 1 MT19937 stream, byte for byte; philox: counter-based')
def read_corruption(modelfile, fastq1_in, fastq1_out, seed, fastq2_in, fastq2_out, threads, device, rng):
  """Apply corruption model to FASTQ file of reads (reference cli.py:144-157)"""
  from mitty_amd.readmodel import get_read_model
  from mitty_amd.simulation import readcorrupt as rc
  read_module, read_model = get_read_model(modelfile)
  rc.multi_process(read_module, read_model, fastq1_in, fastq1_out, fastq2_in, fastq2_out, processes=threads, seed=seed,
                   device=device, rng=rng)


@cli.command('god-aligner', short_help='Create a perfect BAM from simulated FASTQs')
@click.argument('fasta', type=click.Path(exists=True))
@click.argument('fastq1', type=click.Path(exists=True))
@click.argument('bam')
@click.option('--fastq2', type=click.Path(exists=True), help='If a paired-end FASTQ, second file goes here')
@click.option('--sample-name', help='If supplied, this is put into the BAM header')
@click.option('--max-templates', type=int, help='For debugging: quits after processing these many templates')
@click.option('--threads', default=2)
@click.option('--device', default=0, help='HIP device ordinal')
@click.option('--gpu-bgzf', is_flag=True, help='Deflate the BAM record blocks on the GPU (additive option)')
@click.option('--hbm-gb', type=float, default=0.0,
              help='BAM records held in HBM before they spill to host memory, GB (0: no limit; additive option, the '
                   'counterpart of the reference\'s samtools sort -m)')
def god_aligner(fasta, bam, sample_name, fastq1, fastq2, max_templates, threads, device, gpu_bgzf, hbm_gb):
  """Given a FASTA.ann file and FASTQ made of simulated reads,
     construct a perfectly aligned BAM from them (reference cli.py:183-204).

     Note: The program uses the fasta.ann file to construct the BAM header"""
  from mitty_amd.benchmarking import god_aligner as god
  god.process_multi_threaded(fasta, bam, fastq1, fastq2, threads, max_templates, sample_name, device=device,
                             gpu_bgzf=gpu_bgzf, hbm_capacity=int(hbm_gb * 1e9))


@cli.command('mq-plot', short_help='Create MQ plot from BAM')
@click.argument('bam', type=click.Path(exists=True))
@click.argument('csv')
@click.argument('plot')
@click.option('--max-d', type=int, default=200, help='Range of d_err to consider')
@click.option('--strict-scoring', is_flag=True, help="Don't consider breakpoints when scoring alignment")
@click.option('--sample-name', help='If the FASTQ contains multiple samples, process reads from only this sample')
@click.option('--threads', default=2)
@click.option('--device', default=0, help='HIP device ordinal')
@click.option('--gpu-inflate', is_flag=True, help="Inflate the BAM's BGZF blocks on the GPU (additive option)")
def mq_plot(bam, csv, plot, max_d, strict_scoring, sample_name, threads, device, gpu_inflate):
  """Given a BAM from simulated reads, construct an MQ plot (reference cli.py:224-236)"""
  from mitty_amd.benchmarking import mq
  mq_mat = mq.process_bam(bam, max_d, strict_scoring, sample_name, threads, csv, device=device,
                          gpu_inflate=gpu_inflate)
  mq.plot_mq(mq_mat, plot)   # (logs and skips the figure when matplotlib is not installed; the CSV is written)


@cli.command('derr-plot', short_help='Create alignment error plot from BAM')
@click.argument('bam', type=click.Path(exists=True))
@click.argument('csv')
@click.argument('plot')
@click.option('--max-v', type=int, default=200, help='Range of variant sizes to consider (51 min)')
@click.option('--max-d', type=int, default=200, help='Range of d_err to consider')
@click.option('--strict-scoring', is_flag=True, help="Don't consider breakpoints when scoring alignment")
@click.option('--sample-name', help='If the FASTQ contains multiple samples, process reads from only this sample')
@click.option('--threads', default=2)
@click.option('--device', default=0, help='HIP device ordinal')
@click.option('--gpu-inflate', is_flag=True, help="Inflate the BAM's BGZF blocks on the GPU (additive option)")
def derr_plot(bam, csv, plot, max_v, max_d, strict_scoring, sample_name, threads, device, gpu_inflate):
  """Given a BAM from simulated reads, show pattern of alignment errors (reference cli.py:239-252)"""
  from mitty_amd.benchmarking import derr
  derr_mat = derr.process_bam(bam, max_v, max_d, strict_scoring, sample_name, threads, csv, device=device,
                              gpu_inflate=gpu_inflate)
  derr.plot_derr(derr_mat, plot)


@cli.command('filter-bam', short_help='Keep the records of a BAM by alignment error')
@click.argument('bamin', type=click.Path(exists=True))
@click.argument('bamout', type=click.Path())
@click.option('--max-d', type=int, default=200, help='Range of d_err to consider')
@click.option('--strict-scoring', is_flag=True, help="Don't consider breakpoints when scoring alignment")
@click.option('--sample-name', help='Score reads from only this sample (the others are unscored)')
@click.option('--min-derr', type=int, default=1, help='Keep records with |d_err| of at least this')
@click.option('--max-derr', type=int, default=None,
              help='Keep records with |d_err| of at most this (default: --max-d).  |d_err| == max_d means another '
                   'chromosome, or max_d or further away')
@click.option('--min-mq', type=int, default=0, help='Keep records with MAPQ of at least this')
@click.option('--max-mq', type=int, default=255, help='Keep records with MAPQ of at most this')
@click.option('--unscored', type=click.Choice(['drop', 'keep']), default='drop',
              help='Records that are not scored: unplaced, or not of --sample-name')
@click.option('--threads', default=2)
@click.option('--device', default=0, help='HIP device ordinal')
@click.option('--gpu-inflate', is_flag=True, help="Inflate the BAM's BGZF blocks on the GPU")
def filter_bam(bamin, bamout, max_d, strict_scoring, sample_name, min_derr, max_derr, min_mq, max_mq, unscored, threads,
               device, gpu_inflate):
  """Given a BAM of aligned simulated reads, write the records whose alignment error |d_err| and MAPQ lie in the given
  ranges to BAMOUT, in input order (the reference has a stub, cli.py:207-221).  With the defaults these are the
  misaligned reads: exactly the records mq-plot counts outside its d_err = 0 column.  |d_err| == max_d means another
  chromosome, or max_d or further away."""
  from mitty_amd.benchmarking import filter_bam as fb
  try:   # (a bad range fails here, before any file or device is touched)
    fb.check_ranges(max_d, min_derr, max_derr, min_mq, max_mq)
  except ValueError as e:
    raise click.BadParameter(str(e))
  counts = fb.filter_bam(bamin, bamout, max_d=max_d, strict=strict_scoring, sample_name=sample_name, min_derr=min_derr,
                         max_derr=max_derr, min_mq=min_mq, max_mq=max_mq, unscored=unscored, processes=threads,
                         device=device, gpu_inflate=gpu_inflate)
  logging.info('filter-bam: {}'.format(counts))


def main():
  cli()


if __name__ == '__main__':
  main()
