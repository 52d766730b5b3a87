"""Copies of running envs (VecSparkSchedSimEnv.fork / snapshot / restore, SparkSchedSimEnv.__deepcopy__, evaluation.continuations;
include/sss.h sss_env_copy) under the CPU wave emulator: the checks of tests/fork_util.py with the plain-loop form of the copy
(csrc/sss_fork.h) - tests/test_gpu_fork.py runs the same checks with the kernel."""
import pytest

import fork_util as F
from emu_util import load_emu
from golden_util import Golden

CASES = [("c1_fair", 0), ("e100_hash", 2), ("tiny_fair_tlimit", 0)]  # E = 10: a grown common pool; the wide instantiation; time-limit mode


@pytest.mark.parametrize("name,seed,which", [(n, s, w) for n, s in CASES for w in range(3)])
def test_fork_continues_the_recorded_trajectory(name, seed, which, pack):
    F.check_fork_continues(name, seed, F.fork_points(Golden(name), seed)[which], pack, "cpu", load_emu())


@pytest.mark.parametrize("name", ["c1", "e100"])
def test_fork_diverges_as_the_references_deepcopy(name, pack):
    F.check_fork_diverges(name, pack, "cpu", load_emu())


@pytest.mark.parametrize("seed_value", [0, 777, 2 ** 63 + 5])
def test_reseed_is_numpys_fresh_generator(seed_value, pack):
    F.check_reseed(seed_value, pack, "cpu", load_emu())


def test_image_definition(pack):
    F.check_image_definition(pack, "cpu", load_emu())


def test_fork_in_the_middle_of_a_step(pack):
    F.check_mid_step_fork(pack, "cpu", load_emu())


def test_snapshot_and_restore(pack):
    F.check_snapshot_restore(pack, "cpu", load_emu())


def test_argument_structures_match_the_header(tmp_path):
    F.check_abi(load_emu(), tmp_path)


def test_facade_deepcopy():
    F.check_facade_deepcopy("cpu", load_emu())


def test_continuations(pack):
    F.check_continuations(pack, "cpu", load_emu())
