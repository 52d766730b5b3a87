"""-m gpu: copies of running envs on a real MI355X - the checks of tests/fork_util.py with the copy kernel (csrc/sss_fork.h
sss_env_copy_kernel); tests/test_emu_fork.py runs the same checks with the emulator library's plain loops."""
import ctypes as C

import pytest

import fork_util as F
from golden_util import Golden
from test_emu_fork import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,seed,which", [(n, s, w) for n, s in CASES for w in range(3)])
def test_fork_continues_the_recorded_trajectory_gpu(name, seed, which, pack):
    F.check_fork_continues(name, seed, F.fork_points(Golden(name), seed)[which], pack, "cuda:0", None)


@pytest.mark.parametrize("name", ["c1", "e100"])
def test_fork_diverges_as_the_references_deepcopy_gpu(name, pack):
    F.check_fork_diverges(name, pack, "cuda:0", None)


@pytest.mark.parametrize("seed_value", [0, 777, 2 ** 63 + 5])
def test_reseed_is_numpys_fresh_generator_gpu(seed_value, pack):
    F.check_reseed(seed_value, pack, "cuda:0", None)


def test_image_definition_gpu(pack):
    F.check_image_definition(pack, "cuda:0", None)


def test_fork_in_the_middle_of_a_step_gpu(pack):
    F.check_mid_step_fork(pack, "cuda:0", None)


def test_snapshot_and_restore_gpu(pack):
    F.check_snapshot_restore(pack, "cuda:0", None)


def test_argument_structures_match_the_header_gpu(tmp_path):
    from spark_sched_sim_amd import build
    F.check_abi(C.CDLL(build.OUT), tmp_path)


def test_facade_deepcopy_gpu():
    F.check_facade_deepcopy("cuda:0", None)


def test_continuations_gpu(pack):
    F.check_continuations(pack, "cuda:0", None)
