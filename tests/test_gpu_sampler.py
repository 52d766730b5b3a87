"""GPU leg of tests/test_emu_sampler.py: the Decima samplers against an fp64 softmax on the gfx950 build, with N large enough for
power - 2M draws per score profile (tests/sampler_util.py; test_emu_sampler.py checks at these sizes that wrong samplers are
rejected)."""
import pytest

import sampler_util as su

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from spark_sched_sim_amd.binding import Binding

    return Binding()


@pytest.mark.parametrize("n", su.STAGE_COUNTS)
def test_stage_draw_follows_the_fp64_softmax(hip, n):
    for name in su.PROFILES:
        su.check_stage_profile(hip, DEV, name, n, su.N_GPU)


@pytest.mark.parametrize("E", su.EXEC_COUNTS)
def test_exec_draw_follows_the_fp64_softmax(hip, E):
    for name in su.PROFILES:
        su.check_exec_profile(hip, DEV, name, E, su.N_GPU)


def test_masked_and_stale_slots_are_never_drawn(hip):
    su.check_masked_and_stale(hip, DEV, su.N_GPU)


def test_empty_draws(hip):
    su.check_empty_cases(hip, DEV)


def test_joint_stage_and_count_draw(hip):
    su.check_joint(hip, DEV, su.N_GPU)


def test_draws_of_neighbouring_keys_are_independent(hip):
    su.check_independence(hip, DEV, su.N_GPU)


def test_crafted_seeds_never_draw_a_candidate_far_below_the_best(hip):
    su.check_crafted_seeds(hip, DEV)


@pytest.mark.parametrize("E", [10, 64, 65, 128])
def test_policy_kernel_draws_follow_the_fp64_softmax(E):
    su.check_policy_kernel(DEV, None, E, B=64, K=3000)


def test_policy_kernel_crafted_seeds():
    su.check_policy_kernel_crafted(DEV, None, E=100, B=16)


def test_segment_categorical_against_fp64(hip):
    su.check_segcat64(hip, DEV)
