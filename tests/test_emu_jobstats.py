"""sss_job_stats (csrc/sss_jobstats.h; `VecSparkSchedSimEnv.job_stats`, `metrics.batch_*`) under the CPU wave emulator - the
plain-loop form of the same device functions: every column and percentile against the host functions on live envs and against
numpy on crafted arena blocks, bit for bit; what the call writes; its argument checks (tests/jobstats_util.py)."""
import pytest

import jobstats_util as ju
from emu_util import load_emu


@pytest.mark.parametrize("num_executors,cap,chunk", [(10, 8, 6), (50, 20, 40)])
def test_live_envs_carry_the_host_functions_bits(num_executors, cap, chunk):
    ju.check_live("cpu", load_emu(), num_executors, cap, chunk=chunk)


@pytest.mark.parametrize("pattern", ju.PATTERNS)
def test_crafted_blocks_against_numpy(pattern):
    ju.check_crafted("cpu", load_emu(), patterns=(pattern,))


def test_only_the_outputs_of_active_envs_are_written():
    ju.check_writes("cpu", load_emu())


def test_argument_checks():
    ju.check_argument_errors("cpu", load_emu())
