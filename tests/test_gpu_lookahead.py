"""-m gpu: the lookahead scheduler and its two kernels on a real MI355X - the checks of tests/lookahead_util.py with
sss_rollout_each_kernel (narrow and wide, csrc/sss_sim_each.h) and sss_lookahead_pick_kernel (csrc/sss_lookahead.h);
tests/test_emu_lookahead.py runs the same checks on the CPU wave emulator."""
import pytest

import lookahead_util as LU
from test_emu_lookahead import EXECUTORS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_rollout_each_equals_the_fused_rollout_gpu(num_executors, pack):
    LU.check_each_equals_rollout(num_executors, pack, "cuda:0", None)


def test_first_step_policy_gpu(pack):
    LU.check_first_step_policy(pack, "cuda:0", None)


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_an_env_stops_at_the_end_of_its_episode_gpu(num_executors, pack):
    LU.check_stops_at_the_end(num_executors, pack, "cuda:0", None)


@pytest.mark.parametrize("samples", [1, 3])
def test_pick_against_the_host_definition_gpu(samples, pack):
    LU.check_pick(samples, pack, "cuda:0", None)


def test_scheduler_against_a_composition_of_the_existing_calls_gpu(pack):
    LU.check_scheduler_against_composition([0, 1], pack, "cuda:0", None)


def test_lookahead_never_ends_above_a_candidate_gpu(pack):
    LU.check_exact_improvement(pack, "cuda:0", None)


def test_fused_continuations_equal_the_lock_step_ones_gpu(pack):
    LU.check_fused_continuations(pack, "cuda:0", None)


def test_refusals_and_arguments_gpu(pack):
    LU.check_refusals(pack, "cuda:0", None)


def test_reseeded_samples_share_their_noise_gpu(pack):
    LU.check_reseeded_samples(pack, "cuda:0", None)
