"""`spark_sched_sim_amd.evaluation` and the trainer's held-out evaluation under the CPU wave emulator (tests/evaluation_util.py):
`run_episodes` against a hand-written loop for an on-device heuristic and for a DecimaPolicy, `compare`, and that evaluating while
training leaves the training run's parameters bit for bit what they are without it."""
import pytest

import evaluation_util as E
from emu_util import load_emu

B = 6


def test_run_episodes_under_an_on_device_policy_equals_a_hand_written_loop():
    E.check_on_device_policy("cpu", load_emu(), B, "fair", chunk=16)


@pytest.mark.parametrize("greedy", [True, False])
def test_run_episodes_under_a_decima_policy_equals_a_hand_written_loop(greedy):
    E.check_decima("cpu", load_emu(), B, greedy)


def test_evaluating_while_training_leaves_the_run_bit_for_bit(tmp_path):
    E.check_evaluating_while_training("cpu", load_emu(), tmp_path)
