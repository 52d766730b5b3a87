"""GPU leg of tests/test_emu_evaluation.py (tests/evaluation_util.py) at 96 envs - more than one wave's worth, episodes that end in
different windows of the 64-step done-mask check, capacity graphs, work space kept per stream: `run_episodes` under two on-device
heuristics and under a DecimaPolicy (greedy and sampled) against hand-written loops, the greedy loop's actions replayed through the C
oracle, the greedy route without a device->host transfer between the done-mask reads, and evaluation inside a deterministic training run."""
import pytest

import evaluation_util as E

pytestmark = pytest.mark.gpu

DEV, B = "cuda:0", 96


@pytest.mark.parametrize("actor", ["fair", "sjfcp"])
def test_run_episodes_under_an_on_device_policy_equals_a_hand_written_loop(actor):
    E.check_on_device_policy(DEV, None, B, actor, chunk=16)


@pytest.mark.parametrize("greedy", [True, False])
def test_run_episodes_under_a_decima_policy_equals_a_hand_written_loop(greedy):
    E.check_decima(DEV, None, B, greedy, oracle_envs=(0, 1, 63, 64, 95) if greedy else (), no_transfer=greedy)


def test_evaluating_while_training_leaves_the_run_bit_for_bit(tmp_path):
    E.check_evaluating_while_training(DEV, None, tmp_path)
