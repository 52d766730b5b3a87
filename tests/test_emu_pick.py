"""The lookahead's pick kernels and rem_work at the sizes where lanes stride (tests/pick_util.py) under the CPU wave emulator: the
plain-loop form of the two picks (csrc/sss_lookahead.h) on crafted blocks at K x S = 1024 and job_cap = 1024, and the kernel source
of until_rem_work (csrc/sss_sim_until.h) run lane by lane over more than two strides of active jobs - tests/test_gpu_pick.py runs
the same checks with the gfx950 kernels, the only build that holds the picks' strided and barrier form."""
import pytest

import pick_util as PU
from emu_util import load_emu

EXECUTORS = [5, 65]  # the narrow instantiation; the smallest case of the wide one


@pytest.mark.parametrize("which", ["horizon", "plain"])
def test_pick_kernels_on_crafted_blocks(which, pack):
    print(PU.check_crafted(which, pack, "cpu", load_emu()))


@pytest.mark.parametrize("num_executors", EXECUTORS)
def test_rem_work_over_more_than_two_strides_of_active_jobs(num_executors, pack):
    print(PU.check_dense_rem_work(num_executors, pack, "cpu", load_emu()))


def test_horizon_pick_on_dense_children(pack):
    print(PU.check_dense_pick(pack, "cpu", load_emu()))
