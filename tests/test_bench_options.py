"""bench.py's command line: a plain run measures the headline step alone; the baselines, block,
attention, HIP-graph and CPU records run only with --full."""
import pytest

import bench

RECORDS = ('no_baselines', 'no_block', 'no_attention', 'no_cpu', 'no_graph')


def skipped(*argv):
    args = bench.parse_args(list(argv))
    return {name for name in RECORDS if getattr(args, name)}


def test_a_plain_run_is_the_headline_step_alone():
    assert skipped('--gpus', '1', '--steps', '20', '--warmup', '10') == set(RECORDS)
    assert skipped('--config', 'opt-1.3b') == set(RECORDS)
    assert not bench.parse_args([]).no_gemm_events     # the roofline rides on the timed steps


def test_full_runs_every_record():
    assert skipped('--full') == set()
    assert skipped('--full', '--no-cpu', '--no-graph') == {'no_cpu', 'no_graph'}
    assert skipped('--full', '--only') == set(RECORDS)
    # the other configs have their baselines, the headline's block-level records stay off
    assert skipped('--full', '--config', 'llama-7b') == set(RECORDS) - {'no_baselines'}


def test_bad_command_lines_are_refused():
    with pytest.raises(SystemExit):
        bench.parse_args(['--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse_args(['--config', 'tiny-rehearsal'])
