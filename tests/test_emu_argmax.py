"""The arg-max Decima decisions (sss_decima_argmax, sss_decima_policy_argmax: second instantiations of the draw kernels,
csrc/sss_decima_policy.h) under the CPU wave emulator: the selection against np.argmax over the candidates, the tie rule, what is
masked, lgprob against fp64 and against the draw's own bits, and the greedy routes of DecimaPolicy (tests/argmax_util.py)."""
import pytest

import argmax_util as au
from emu_util import load_emu


@pytest.fixture(scope="module")
def emu():
    from spark_sched_sim_amd.binding import Binding

    return Binding(load_emu())


def test_selection_is_the_arg_max_of_the_candidates(emu):
    au.check_random_scores(emu, "cpu")
    au.check_both_decisions(emu, "cpu")


def test_ties_go_to_the_lowest_index(emu):
    au.check_ties(emu, "cpu")


def test_masked_slots_and_nans_never_win(emu):
    au.check_masking(emu, "cpu")


def test_greedy_policy_routes_use_the_kernels_and_leave_the_draw_counter(emu):
    au.check_policy_greedy("cpu", load_emu())
