"""The Decima samplers against an fp64 softmax under the CPU wave emulator (smoke-level N; the GPU leg, test_gpu_sampler.py,
has the statistical power): sss_decima_sample's stage and executor-count draws on synthetic score tables through the C ABI, the
draw phase of the one-launch policy kernel on real observations, sss_segment_categorical against fp64, the crafted-seed edge of
the uniform stream in full, and the power of the goodness-of-fit checks against deliberately wrong samplers (tests/sampler_util.py)."""
import numpy as np
import pytest

import sampler_util as su
from emu_util import load_emu

N = 1500  # draws per profile here


@pytest.fixture(scope="module")
def emu():
    from spark_sched_sim_amd.binding import Binding

    return Binding(load_emu())


def test_stage_draw_follows_the_fp64_softmax_on_every_profile(emu):
    for name in su.PROFILES:
        for n in (3, 65, 129):
            su.check_stage_profile(emu, "cpu", name, n, N)


@pytest.mark.parametrize("n", su.STAGE_COUNTS)
def test_stage_draw_at_every_candidate_count(emu, n):
    su.check_stage_profile(emu, "cpu", "random", n, N if n < 1000 else 400)


def test_exec_draw_follows_the_fp64_softmax(emu):
    for name in su.PROFILES:
        su.check_exec_profile(emu, "cpu", name, 65, N)
    for E in su.EXEC_COUNTS:
        su.check_exec_profile(emu, "cpu", "ramp", E, N)


def test_masked_and_stale_slots_are_never_drawn(emu):
    su.check_masked_and_stale(emu, "cpu", 3000)


def test_empty_draws(emu):
    su.check_empty_cases(emu, "cpu")


def test_joint_stage_and_count_draw(emu):
    su.check_joint(emu, "cpu", 4000)


def test_draws_of_neighbouring_keys_are_independent(emu):
    su.check_independence(emu, "cpu", 4000)


@pytest.mark.parametrize("draw", [0, 1], ids=["stage", "count"])
def test_crafted_seeds_never_draw_a_candidate_far_below_the_best(emu, draw):
    """fails before dp_gumbel's clamp: the top 24-bit value gave u = 1.0 and an infinite key"""
    su.check_crafted_seeds(emu, "cpu", draws=(draw,))


def test_crafted_seed_helpers():
    """the splitmix64 inverse is exact, and the stream restated in decima_util._gumbel maps the extremes to finite values"""
    from decima_util import _gumbel

    rng = np.random.default_rng(0)
    for z in [0, su.M64, *map(int, rng.integers(0, 1 << 63, 20, dtype=np.int64))]:
        assert su.splitmix(su.splitmix_inverse(z)) == z
    for draw in (0, 1):
        for u24, g in (((1 << 24) - 1, su.GUMBEL_MAX), (0, su.GUMBEL_MIN)):
            s = su.crafted_seed(99, 7, 42, draw, u24)
            assert abs(_gumbel(s, 99, 7, 42, draw) - g) < 1e-5


def test_chi_square_helpers_reject_wrong_samplers_at_the_gpu_sizes(capsys):
    """power: samples from deliberately wrong samplers at the GPU leg's N and histogram shapes are rejected at P_REJECT, and the
    exact sampler at the same sizes is not"""
    res = su.wrong_sampler_pvalues()
    with capsys.disabled():
        print()
        for k, p in res.items():
            print(f"  {k:36s} p = {p:.3g}")
    for k, p in res.items():
        if k.startswith("exact"):
            assert p >= su.P_REJECT, (k, p)
        else:
            assert p < su.P_REJECT, (k, p)


@pytest.mark.parametrize("E", [10, 65])
def test_policy_kernel_draws_follow_the_fp64_softmax(E):
    su.check_policy_kernel("cpu", load_emu(), E, B=4, K=150)


def test_policy_kernel_crafted_seeds():
    su.check_policy_kernel_crafted("cpu", load_emu(), E=100, B=6)


def test_segment_categorical_against_fp64(emu):
    su.check_segcat64(emu, "cpu")
