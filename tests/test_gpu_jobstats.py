"""GPU leg of tests/test_emu_jobstats.py: the sss_job_stats kernel on the gfx950 build against the host functions and numpy, bit
for bit (tests/jobstats_util.py), with one case at the largest job capacity (1024: the sort's and the sums' largest shapes)."""
import pytest

import jobstats_util as ju

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("num_executors,cap,chunk", [(10, 8, 6), (50, 20, 40)])
def test_live_envs_carry_the_host_functions_bits(num_executors, cap, chunk):
    ju.check_live(DEV, None, num_executors, cap, chunk=chunk)


def test_crafted_blocks_against_numpy():
    ju.check_crafted(DEV, None)


def test_crafted_blocks_at_the_largest_job_capacity():
    ju.check_crafted(DEV, None, cap=1024, sizes=(1024, 1023, 513, 512, 300, 0), patterns=("wide", "duplicates", "general"))


def test_only_the_outputs_of_active_envs_are_written():
    ju.check_writes(DEV, None)


def test_argument_checks():
    ju.check_argument_errors(DEV, None)
