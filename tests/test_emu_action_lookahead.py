"""The lookahead over actions - sss_decima_topk, sss_rollout_action (include/sss.h; csrc/sss_decima_policy.h decima_topk_wave,
csrc/sss_sim_action.h), DecimaPolicy.topk_env / rollout_action_env, VecSparkSchedSimEnv.rollout_action and
lookahead.ActionLookaheadScheduler - under the CPU wave emulator: the checks of tests/action_lookahead_util.py with the kernel source
run lane by lane. tests/test_gpu_action_lookahead.py runs the same checks with the gfx950 kernels, and the whole episodes of the
guarantee."""
import pytest

import action_lookahead_util as AU
from emu_util import load_emu

UNITS = ["narrow", "wide"]  # 5 executors: the unit for up to 64; 100 executors: the wide one (two executor counts per lane)
FOLLOWERS = ["fair", "sjfcp", "decima_greedy", "decima_sampled"]


@pytest.mark.parametrize("which", UNITS)
def test_slot_0_is_the_policy(which, pack):
    AU.check_slot0_is_the_policy(which, pack, "cpu", load_emu())


@pytest.mark.parametrize("which", UNITS)
def test_order_and_padding(which, pack):
    AU.check_order_and_padding(which, pack, "cpu", load_emu())


@pytest.mark.parametrize("which", UNITS)
def test_ties_go_to_the_lower_index(which, pack):
    AU.check_ties(which, pack, "cpu", load_emu())


@pytest.mark.parametrize("which", UNITS)
def test_executor_counts_of_the_other_slots(which, pack):
    AU.check_exec_counts(which, pack, "cpu", load_emu())


@pytest.mark.parametrize("follower", FOLLOWERS)
@pytest.mark.parametrize("which", UNITS)
def test_a_forced_action_is_a_step(which, follower, pack):
    AU.check_forced_action(which, follower, pack, "cpu", load_emu())


@pytest.mark.parametrize("which", UNITS)
def test_a_refused_action_is_the_steps_error(which, pack):
    AU.check_refused_action(which, pack, "cpu", load_emu())


@pytest.mark.parametrize("samples,reseed", [(1, None), (2, 2 ** 63 + 11)], ids=["exact", "reseeded"])
def test_the_scheduler_is_its_composition(samples, reseed, pack):
    AU.check_scheduler_against_composition(samples, reseed, 1, pack, "cpu", load_emu())  # (the first decision: the lock-step side is slow on the emulator)


def test_the_guarantee_over_the_last_decisions(pack):
    AU.check_guarantee(AU.EMU_PREFIX, pack, "cpu", load_emu())  # (the parents play most of the episode under greedy Decima first)


def test_heuristic_base_and_run_lookahead(pack):
    AU.check_heuristic_base_and_evaluation(pack, "cpu", load_emu())


def test_refusals_and_arguments(pack):
    AU.check_refusals(pack, "cpu", load_emu())
