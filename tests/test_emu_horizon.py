"""The lookahead with a time horizon and its two entry points (include/sss.h sss_rollout_until, sss_lookahead_pick_horizon;
lookahead.LookaheadScheduler with `horizon`, evaluation.horizon_cost) under the CPU wave emulator: the checks of tests/horizon_util.py
with the kernel source of csrc/sss_sim_until.h run lane by lane and the plain-loop form of the horizon pick (csrc/sss_lookahead.h) -
tests/test_gpu_horizon.py runs the same checks with the gfx950 kernels."""
import pytest

import horizon_util as HU
from emu_util import load_emu

EXECUTORS = [5, 65]  # the narrow instantiation; the smallest case of the wide one
PICK_HORIZON = 20000.0  # children of the pick check: some overshoot it past an arrival, all hold unfinished work, 4 to 6 steps each
WARM = 50  # fair steps before the scheduler takes over in the two checks that run whole full-episode lookaheads (none on the GPU, and two parents there)
SCHED_HORIZON = 60000.0  # the scheduler checks: a fraction of a TINY episode (0.5 .. 2.6 million time units)


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_an_infinite_horizon_is_rollout_each(num_executors, pack):
    HU.check_inf_equals_each(num_executors, pack, "cpu", load_emu())


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_a_finite_horizon_is_lock_step_and_rem_work_is_job_work(num_executors, pack):
    HU.check_finite_equals_lock_step(num_executors, pack, "cpu", load_emu())


@pytest.mark.parametrize("samples", [1, 3])
def test_horizon_pick_against_the_host_definition(samples, pack):
    HU.check_pick(samples, PICK_HORIZON, pack, "cpu", load_emu())


def test_scheduler_with_an_infinite_horizon_is_the_scheduler_without(pack):
    HU.check_scheduler_inf_equals_none([0], WARM, pack, "cpu", load_emu())


def test_scheduler_with_a_horizon_against_a_composition_of_the_existing_calls(pack):
    HU.check_scheduler_against_composition([0], SCHED_HORIZON, "srpt", pack, "cpu", load_emu())  # (one parent: the lock-step side is slow on the emulator)


def test_a_finite_horizon_takes_fewer_child_steps(pack):
    HU.check_fewer_child_steps([0], SCHED_HORIZON, WARM, pack, "cpu", load_emu())


def test_reseeded_samples_share_their_noise_with_a_horizon(pack):
    HU.check_reseeded_samples(SCHED_HORIZON, pack, "cpu", load_emu())


def test_horizon_refusals_and_arguments(pack):
    HU.check_refusals(pack, "cpu", load_emu())
