"""-m gpu: the lookahead's pick kernels and rem_work at the sizes where lanes stride, on a real MI355X - the checks of
tests/pick_util.py with sss_lookahead_pick_kernel and sss_lookahead_pick_horizon_kernel (csrc/sss_lookahead.h: the 64-strides over
children, candidates and sort keys, the barriers between them) and sss_rollout_until_kernel's until_rem_work (narrow and wide,
csrc/sss_sim_until.h); tests/test_emu_pick.py runs the same checks on the CPU wave emulator."""
import pytest

import pick_util as PU
from test_emu_pick import EXECUTORS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", ["horizon", "plain"])
def test_pick_kernels_on_crafted_blocks_gpu(which, pack):
    print(PU.check_crafted(which, pack, "cuda:0", None))


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_rem_work_over_more_than_two_strides_of_active_jobs_gpu(num_executors, pack):
    print(PU.check_dense_rem_work(num_executors, pack, "cuda:0", None))


def test_horizon_pick_on_dense_children_gpu(pack):
    print(PU.check_dense_pick(pack, "cuda:0", None))
