"""The lookahead scheduler and its two entry points (include/sss.h sss_rollout_each, sss_lookahead_pick; lookahead.LookaheadScheduler,
evaluation.run_lookahead, evaluation.continuations with fused=True) under the CPU wave emulator: the checks of tests/lookahead_util.py
with the kernel source of csrc/sss_sim_each.h run lane by lane and the plain-loop form of the pick (csrc/sss_lookahead.h) -
tests/test_gpu_lookahead.py runs the same checks with the gfx950 kernels."""
import pytest

import lookahead_util as LU
from emu_util import load_emu

EXECUTORS = [5, 65]  # the narrow instantiation; the smallest case of the wide one


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_rollout_each_equals_the_fused_rollout(num_executors, pack):
    LU.check_each_equals_rollout(num_executors, pack, "cpu", load_emu())


def test_first_step_policy(pack):
    LU.check_first_step_policy(pack, "cpu", load_emu())


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_an_env_stops_at_the_end_of_its_episode(num_executors, pack):
    LU.check_stops_at_the_end(num_executors, pack, "cpu", load_emu())


@pytest.mark.parametrize("samples", [1, 3])
def test_pick_against_the_host_definition(samples, pack):
    LU.check_pick(samples, pack, "cpu", load_emu())


def test_scheduler_against_a_composition_of_the_existing_calls(pack):
    LU.check_scheduler_against_composition([0], pack, "cpu", load_emu())  # (one parent: the lock-step side is slow on the emulator)


def test_lookahead_never_ends_above_a_candidate(pack):
    LU.check_exact_improvement(pack, "cpu", load_emu())


def test_fused_continuations_equal_the_lock_step_ones(pack):
    LU.check_fused_continuations(pack, "cpu", load_emu())


def test_refusals_and_arguments(pack):
    LU.check_refusals(pack, "cpu", load_emu())


def test_reseeded_samples_share_their_noise(pack):
    LU.check_reseeded_samples(pack, "cpu", load_emu())
