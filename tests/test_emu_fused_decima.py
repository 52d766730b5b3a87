"""The fused Decima rollout (include/sss.h sss_rollout_decima; csrc/sss_sim_decima.h) and what is built on it - DecimaPolicy.rollout_env,
evaluation.run_episodes / continuations with fused=True, lookahead.LookaheadScheduler with a Decima candidate - under the CPU wave
emulator: the checks of tests/fused_decima_util.py with the kernel source run lane by lane. tests/test_gpu_fused_decima.py runs the same
checks with the gfx950 kernels, where the two things the emulator cannot show - the carved dynamic LDS and the visibility of the
wave's own observation rows - are real."""
import pytest

import fused_decima_util as FU
from emu_util import load_emu

UNITS = ["narrow", "wide"]  # 5 executors: the unit for up to 64; 100 executors: the wide one (two executor counts per lane)
GREEDY = [True, False]


@pytest.mark.parametrize("greedy", GREEDY, ids=["greedy", "sampled"])
@pytest.mark.parametrize("which", UNITS)
def test_one_launch_equals_many(which, greedy, pack):
    FU.check_one_launch_equals_many(which, greedy, pack, "cpu", load_emu())


@pytest.mark.parametrize("greedy", GREEDY, ids=["greedy", "sampled"])
@pytest.mark.parametrize("which", UNITS)
def test_every_decision_is_the_lock_step_kernels_and_the_strides_ran(which, greedy, pack):
    FU.check_decisions_equal_lock_step(which, greedy, pack, "cpu", load_emu())


@pytest.mark.parametrize("which", UNITS)
def test_per_env_policies(which, pack):
    FU.check_per_env_policies(which, pack, "cpu", load_emu())


@pytest.mark.parametrize("base", [None, ("decima", 0)], ids=["switching", "over_decima"])
def test_lookahead_with_a_decima_candidate_against_a_composition_of_the_existing_calls(base, pack):
    FU.check_lookahead_first_decisions(base, 2, pack, "cpu", load_emu())  # (the first decisions: the lock-step side is slow on the emulator)


@pytest.mark.parametrize("which", UNITS)
def test_run_episodes_fused_equals_lock_step(which, pack):
    FU.check_run_episodes(which, 60, pack, "cpu", load_emu())


def test_continuations_with_a_decima_policy(pack):
    FU.check_continuations(pack, "cpu", load_emu())


def test_refusals_and_arguments(pack):
    FU.check_refusals(pack, "cpu", load_emu())
