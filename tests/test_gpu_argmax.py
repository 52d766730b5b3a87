"""GPU leg of tests/test_emu_argmax.py: the arg-max Decima decisions on the gfx950 build (tests/argmax_util.py), and the greedy
step's on-device route under torch.cuda.set_sync_debug_mode("error") - no device->host transfer."""
import pytest

import argmax_util as au

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from spark_sched_sim_amd.binding import Binding

    return Binding()


def test_selection_is_the_arg_max_of_the_candidates(hip):
    au.check_random_scores(hip, DEV)
    au.check_both_decisions(hip, DEV)


def test_ties_go_to_the_lowest_index(hip):
    au.check_ties(hip, DEV)


def test_masked_slots_and_nans_never_win(hip):
    au.check_masking(hip, DEV)


def test_greedy_policy_routes_make_no_device_to_host_transfer(hip):
    au.check_policy_greedy(DEV, None, no_transfer=True)
