"""The fused Decima rollout on the GPU (include/sss.h sss_rollout_decima; csrc/sss_sim_decima.h, csrc/sss_hip_sim.hip, csrc/sss_hip_wide.hip):
the checks of tests/fused_decima_util.py with the gfx950 kernels - here the dynamic LDS is one allocation that the simulator's pool
and Decima's work space share, and the policy reads observation rows its own wave wrote a moment earlier. tests/test_emu_fused_decima.py
runs the same checks under the CPU wave emulator."""
import pytest

import fused_decima_util as FU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNITS = ["narrow", "wide"]
GREEDY = [True, False]


@pytest.mark.parametrize("greedy", GREEDY, ids=["greedy", "sampled"])
@pytest.mark.parametrize("which", UNITS)
def test_one_launch_equals_many(which, greedy, pack):
    FU.check_one_launch_equals_many(which, greedy, pack, DEV, None)


@pytest.mark.parametrize("greedy", GREEDY, ids=["greedy", "sampled"])
@pytest.mark.parametrize("which", UNITS)
def test_every_decision_is_the_lock_step_kernels_and_the_strides_ran(which, greedy, pack):
    FU.check_decisions_equal_lock_step(which, greedy, pack, DEV, None)


@pytest.mark.parametrize("which", UNITS)
def test_per_env_policies(which, pack):
    FU.check_per_env_policies(which, pack, DEV, None)


@pytest.mark.parametrize("base", [None, ("decima", 0)], ids=["switching", "over_decima"])
def test_lookahead_with_a_decima_candidate_against_a_composition_of_the_existing_calls(base, pack):
    FU.check_lookahead_first_decisions(base, 3, pack, DEV, None)


def test_lookahead_never_ends_above_a_candidate(pack):
    FU.check_lookahead_never_ends_above_a_candidate(pack, DEV, None)


@pytest.mark.parametrize("which", UNITS)
def test_run_episodes_fused_equals_lock_step(which, pack):
    FU.check_run_episodes(which, 2000, pack, DEV, None)


def test_continuations_with_a_decima_policy(pack):
    FU.check_continuations(pack, DEV, None)


def test_refusals_and_arguments(pack):
    FU.check_refusals(pack, DEV, None)
