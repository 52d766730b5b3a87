"""-m gpu: the lookahead with a time horizon and its two kernels on a real MI355X - the checks of tests/horizon_util.py with
sss_rollout_until_kernel (narrow and wide, csrc/sss_sim_until.h) and sss_lookahead_pick_horizon_kernel (csrc/sss_lookahead.h);
tests/test_emu_horizon.py runs the same checks on the CPU wave emulator."""
import pytest

import horizon_util as HU
from test_emu_horizon import EXECUTORS, PICK_HORIZON, SCHED_HORIZON

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_an_infinite_horizon_is_rollout_each_gpu(num_executors, pack):
    HU.check_inf_equals_each(num_executors, pack, "cuda:0", None)


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_a_finite_horizon_is_lock_step_and_rem_work_is_job_work_gpu(num_executors, pack):
    HU.check_finite_equals_lock_step(num_executors, pack, "cuda:0", None)


@pytest.mark.parametrize("samples", [1, 3])
def test_horizon_pick_against_the_host_definition_gpu(samples, pack):
    HU.check_pick(samples, PICK_HORIZON, pack, "cuda:0", None)


def test_scheduler_with_an_infinite_horizon_is_the_scheduler_without_gpu(pack):
    HU.check_scheduler_inf_equals_none([0, 1], 0, pack, "cuda:0", None)


def test_scheduler_with_a_horizon_against_a_composition_of_the_existing_calls_gpu(pack):
    HU.check_scheduler_against_composition([0, 1], SCHED_HORIZON, "srpt", pack, "cuda:0", None)


def test_a_finite_horizon_takes_fewer_child_steps_gpu(pack):
    HU.check_fewer_child_steps([0, 1], SCHED_HORIZON, 0, pack, "cuda:0", None)


def test_reseeded_samples_share_their_noise_with_a_horizon_gpu(pack):
    HU.check_reseeded_samples(SCHED_HORIZON, pack, "cuda:0", None)


def test_horizon_refusals_and_arguments_gpu(pack):
    HU.check_refusals(pack, "cuda:0", None)
