"""-m gpu: the hash policy's launch with a thread per env (csrc/sss_sim.h sss_policy_hash_kernel, 256 envs per workgroup) on a real
MI355X, against the Python recomputation of tests/test_emu_policy_hash_direct.py, and what the launch writes beyond its envs:
nothing."""
import numpy as np
import pytest
import torch

from spark_sched_sim_amd import VecSparkSchedSimEnv
from spark_sched_sim_amd.binding import POLICY_IDS
from test_emu_policy_hash_direct import C2, SHORT_EPISODES, WIDE, compare_trajectory, reference_actions

pytestmark = pytest.mark.gpu

SENTINEL = -77777
GUARD = 256  # entries behind the envs' own: more than a workgroup of the launch could reach if its bound were off


def check_launch_bounds(env, param: int):
    """`sss_policy` into caller tensors of B + GUARD entries: [0, B) is the reference, [B, B + GUARD) is not touched"""
    B = env.num_envs
    si = torch.full((B + GUARD,), SENTINEL, dtype=torch.int32, device=env.device)
    ne = torch.full((B + GUARD,), SENTINEL, dtype=torch.int32, device=env.device)
    env._b.check(env._b.lib.sss_policy(env._h, POLICY_IDS["hash"], param, si.data_ptr(), ne.data_ptr(), env._stream()))
    torch.cuda.synchronize()
    r_si, r_ne = reference_actions(env, param)
    assert np.array_equal(si[:B].cpu().numpy(), r_si) and np.array_equal(ne[:B].cpu().numpy(), r_ne)
    assert bool((si[B:] == SENTINEL).all()) and bool((ne[B:] == SENTINEL).all())


# one thread; a partial workgroup; one thread into the second workgroup; several workgroups
@pytest.mark.parametrize("B", [1, 255, 257, 600])
def test_hash_actions_thread_per_env(B, pack):
    env = VecSparkSchedSimEnv(C2, B, device="cuda:0", pack=pack, auto_reset=True)
    options = {"time_limit": SHORT_EPISODES}
    env.reset(seed=9000, options=options)
    check_launch_bounds(env, 300)
    compare_trajectory(env, 300, 60, also=(0, 1000), revive=dict(seed=9000, options=options))
    check_launch_bounds(env, 0)
    env.close()


def test_hash_actions_thread_per_env_wide(pack):
    env = VecSparkSchedSimEnv(WIDE, 65, device="cuda:0", pack=pack)
    env.reset(seed=500)
    compare_trajectory(env, 300, 20, also=(0,), revive=dict(seed=500))
    check_launch_bounds(env, 300)
    env.close()
