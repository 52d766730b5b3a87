"""The lookahead over actions on the GPU - sss_decima_topk, sss_rollout_action (include/sss.h; csrc/sss_hip.hip, csrc/sss_hip_sim.hip,
csrc/sss_hip_wide.hip), DecimaPolicy.topk_env / rollout_action_env, VecSparkSchedSimEnv.rollout_action and
lookahead.ActionLookaheadScheduler: the checks of tests/action_lookahead_util.py with the gfx950 kernels, where the staged weights, the
four envs per workgroup and the carved dynamic LDS are real, and the guarantee over whole episodes.
tests/test_emu_action_lookahead.py runs the same checks under the CPU wave emulator."""
import pytest

import action_lookahead_util as AU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNITS = ["narrow", "wide"]
FOLLOWERS = ["fair", "sjfcp", "decima_greedy", "decima_sampled"]


@pytest.mark.parametrize("which", UNITS)
def test_slot_0_is_the_policy(which, pack):
    AU.check_slot0_is_the_policy(which, pack, DEV, None)


@pytest.mark.parametrize("which", UNITS)
def test_order_and_padding(which, pack):
    AU.check_order_and_padding(which, pack, DEV, None)


@pytest.mark.parametrize("which", UNITS)
def test_ties_go_to_the_lower_index(which, pack):
    AU.check_ties(which, pack, DEV, None)


@pytest.mark.parametrize("which", UNITS)
def test_executor_counts_of_the_other_slots(which, pack):
    AU.check_exec_counts(which, pack, DEV, None)


@pytest.mark.parametrize("follower", FOLLOWERS)
@pytest.mark.parametrize("which", UNITS)
def test_a_forced_action_is_a_step(which, follower, pack):
    AU.check_forced_action(which, follower, pack, DEV, None)


@pytest.mark.parametrize("which", UNITS)
def test_a_refused_action_is_the_steps_error(which, pack):
    AU.check_refused_action(which, pack, DEV, None)


@pytest.mark.parametrize("samples,reseed", [(1, None), (2, 2 ** 63 + 11)], ids=["exact", "reseeded"])
def test_the_scheduler_is_its_composition(samples, reseed, pack):
    AU.check_scheduler_against_composition(samples, reseed, 3, pack, DEV, None)


def test_the_guarantee_over_whole_episodes(pack):
    AU.check_guarantee(None, pack, DEV, None)


def test_heuristic_base_and_run_lookahead(pack):
    AU.check_heuristic_base_and_evaluation(pack, DEV, None)


def test_refusals_and_arguments(pack):
    AU.check_refusals(pack, DEV, None)
