"""CPU tests of filter-bam: the output header's @PG line, the command's range checks (no device is touched), the
test-side rule (tests/filter_ref.py) against the reference's golden MQ matrices, and the BAM splitter."""
import os

import pytest

from tests import filter_ref as FR
from tests import score_util as SU


def _pg(text):
  return [ln for ln in text.split('\n') if ln.startswith('@PG')]


def test_output_header_text_appends_one_pg_line():
  from mitty_amd.benchmarking.filter_bam import output_header_text
  from mitty_amd.benchmarking.god_aligner import __version__
  text = '@HD\tVN:1.4\tSO:coordinate\n@SQ\tSN:1\tLN:100\n'
  out = output_header_text(text, 'filter-bam a.bam b.bam')
  assert out == text + '@PG\tID:mitty-filter-bam\tPN:mitty\tVN:{}\tCL:filter-bam a.bam b.bam\n'.format(__version__)


def test_output_header_text_supplies_the_final_newline():
  from mitty_amd.benchmarking.filter_bam import output_header_text
  out = output_header_text('@HD\tVN:1.4\n@SQ\tSN:1\tLN:100', 'x')
  assert out.startswith('@HD\tVN:1.4\n@SQ\tSN:1\tLN:100\n@PG\tID:mitty-filter-bam\t') and out.endswith('\tCL:x\n')
  assert out.count('\n') == 3


def test_output_header_text_of_an_empty_text():
  from mitty_amd.benchmarking.filter_bam import output_header_text
  out = output_header_text('', 'x')
  assert out.startswith('@PG\tID:mitty-filter-bam\tPN:mitty\tVN:') and out.endswith('\tCL:x\n') and out.count('\n') == 1


def test_output_header_text_id_collisions():
  from mitty_amd.benchmarking.filter_bam import output_header_text
  once = output_header_text('@HD\tVN:1.4\n', 'one')
  twice = output_header_text(once, 'two')
  thrice = output_header_text(twice, 'three')
  assert [ln.split('\t')[1] for ln in _pg(thrice)] == ['ID:mitty-filter-bam', 'ID:mitty-filter-bam.1',
                                                      'ID:mitty-filter-bam.2']
  assert thrice.startswith(twice) and twice.startswith(once)
  # another program's @PG line, and an ID that only contains ours, do not collide
  other = '@PG\tID:bwa\tPN:bwa\n@PG\tPN:x\tID:mitty-filter-bam-old\n'
  assert _pg(output_header_text(other, 'c'))[-1].split('\t')[1] == 'ID:mitty-filter-bam'
  # the ID is found wherever it stands in its line
  assert _pg(output_header_text('@PG\tPN:mitty\tID:mitty-filter-bam\n', 'c'))[-1].split('\t')[1] == 'ID:mitty-filter-bam.1'


@pytest.mark.parametrize('args,word', [
  (['--min-derr', '-1'], '--min-derr'),
  (['--min-derr', '10', '--max-derr', '5'], '--min-derr'),
  (['--max-d', '50', '--max-derr', '51'], '--max-derr'),
  (['--max-d', '-1'], '--max-d'),
  (['--max-d', str((1 << 20) + 1)], '--max-d'),
  (['--min-mq', '-1'], '--min-mq'),
  (['--max-mq', '256'], '--max-mq'),
  (['--min-mq', '30', '--max-mq', '20'], '--min-mq'),
])
def test_cli_refuses_bad_ranges_before_any_file_or_device(tmp_path, monkeypatch, args, word):
  from click.testing import CliRunner
  from mitty_amd import _native, cli

  def no_device(*a, **k):
    raise AssertionError('a device or a BAM was touched')
  monkeypatch.setattr(_native, 'Context', no_device)
  monkeypatch.setattr(_native, 'BamFile', no_device)
  bam_in, bam_out = str(tmp_path / 'in.bam'), str(tmp_path / 'out.bam')
  with open(bam_in, 'wb') as fp:
    fp.write(b'not a BAM')
  res = CliRunner().invoke(cli.cli, ['filter-bam', bam_in, bam_out] + args)
  assert res.exit_code == 2, res.output
  assert word in res.output
  assert not os.path.exists(bam_out)


def test_cli_help_says_what_max_d_means():
  from click.testing import CliRunner
  from mitty_amd import cli
  res = CliRunner().invoke(cli.cli, ['filter-bam', '--help'])
  assert res.exit_code == 0
  text = ' '.join(res.output.split())
  assert 'another chromosome, or max_d or further away' in text
  for opt in ('--max-d', '--strict-scoring', '--sample-name', '--min-derr', '--max-derr', '--min-mq', '--max-mq',
              '--unscored', '--threads', '--device', '--gpu-inflate'):
    assert opt in res.output


@pytest.mark.parametrize('strict,max_d,want', [(0, 200, 2266), (0, 5, 2266), (1, 200, 2196), (1, 5, 2196)])
def test_default_rule_keeps_what_the_golden_mq_matrix_holds_outside_d_err_0(strict, max_d, want):
  g = SU.golden()
  assert len(g['records']) == 4882 and sum(1 for r in g['records'] if r[2] is not None) == 4587
  kept, counts = FR.verdicts(g['records'], max_d=max_d, strict=bool(strict), sizes=[len(r) for r in g['recs']])
  mq = SU.dense(g['mq']['s{}_d{}'.format(strict, max_d)], (100, 2 * max_d + 1))
  assert len(kept) == int(mq.sum()) - int(mq[:, max_d].sum()) == want
  assert counts['kept'] == want and counts['seen'] == 4882 and counts['skipped_unplaced'] == 295
  assert counts['kept'] + counts['dropped_score'] + counts['dropped_mapq'] + counts['skipped_unplaced'] == 4882
  assert counts['bytes_kept'] == sum(len(g['recs'][i]) for i in kept)
  # everything kept (min_derr 0) is every placed record: the matrix's total
  kept_all, _ = FR.verdicts(g['records'], max_d=max_d, strict=bool(strict), min_derr=0)
  assert len(kept_all) == int(mq.sum()) == 4587


def test_rule_order_and_ranges():
  q1 = 'a:0|1|0|0|100|4|4=|'           # one read group, placed truth: chrom 1, pos 100
  q2 = q1 + '|1|300|4|4=|'             # two groups
  recs = [(q1, 0, '1', 99, 60),        # d_err 0
          (q1, 0, '1', 102, 60),       # d_err 3
          (q1, 0, '2', 99, 60),        # another chromosome: max_d
          (q2, 0x80, '1', 301, 255),   # mate: d_err 2, MAPQ 255
          ('junk', 0, None, 0, 0),     # unplaced: never parsed
          ('other|x', 0, '1', 5, 3)]   # not of the sample: never parsed
  kept, c = FR.verdicts(recs, max_d=10, sample='a')
  assert kept == [1, 2, 3] and c['dropped_score'] == 1 and c['skipped_unplaced'] == 1 and c['skipped_sample'] == 1
  assert FR.verdicts(recs, max_d=10, sample='a', unscored='keep')[0] == [1, 2, 3, 4, 5]
  assert FR.verdicts(recs, max_d=10, sample='a', min_derr=10, max_derr=10)[0] == [2]
  kept, c = FR.verdicts(recs, max_d=10, sample='a', min_derr=0, max_mq=60)
  assert kept == [0, 1, 2] and c['dropped_mapq'] == 1 and c['dropped_score'] == 0
  with pytest.raises(FR.RecordError) as e:
    FR.verdicts(recs[:5] + [('other|x', 0, '1', 5, 3)], max_d=10)
  assert e.value.index == 5
  with pytest.raises(FR.RecordError) as e:
    FR.verdicts([recs[0], (q1, 0x80, '1', 99, 60)], max_d=10)   # read2 record, one group
  assert e.value.index == 1
  with pytest.raises(FR.RecordError) as e:
    FR.verdicts([recs[0], recs[0], (q1, 0, '9', 99, 60)], max_d=10, known_refs={'1', '2'})
  assert e.value.index == 2


def test_split_bam_round_trip_and_checks():
  g = SU.golden()
  recs = g['recs'][:50]
  data = SU.bgzf_bytes(SU.bam_bytes(recs, g['sq'], text='@HD\tVN:1.4\n'), block=700)
  text, refs, got = FR.split_bam(data)
  assert text == '@HD\tVN:1.4\n' and refs == [(s['SN'], s['LN']) for s in g['sq']] and got == recs
  assert sum(FR.member_sizes(data)) == len(SU.bam_bytes(recs, g['sq'], text='@HD\tVN:1.4\n'))
  with pytest.raises(AssertionError):
    FR.split_bam(data[:-28])                                   # no EOF marker
  bad = bytearray(data)
  bad[len(data) - 28 - 6] ^= 1                                 # the last data member's CRC32
  with pytest.raises(AssertionError):
    FR.split_bam(bytes(bad))
