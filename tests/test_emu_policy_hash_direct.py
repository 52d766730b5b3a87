"""The hash policy read straight from an env's HBM image (csrc/sss_sim.h policy_hash_direct), under the CPU wave emulator.

`sss_policy` with the hash policy no longer stages an env: one lane loads four header words and one pool record of the image and
maps them to an action (hash_action). The emulator runs that function through sss_policy_kernel, a wave per env; the gfx950 build
runs it with a thread per env (tests/test_gpu_policy_hash_direct.py).

The reference is a recomputation, in Python integers under a 64-bit mask, of `hash_policy` as tests/golden/make_golden.py defines
it. Its inputs are the env's header fields `seed` and `ep_steps` and the two observation fields the policy must see,
`n_schedulable` (obs_i32[:, 3]) and `num_committable_execs` (obs_i32[:, 4]) - never an action that another path of the kernels
produced."""
import numpy as np
import pytest
import torch

from emu_util import load_emu
from spark_sched_sim_amd import VecSparkSchedSimEnv
from spark_sched_sim_amd.binding import POLICY_IDS

M64 = (1 << 64) - 1
POOL_NONE = -1  # SssHdr::curr_source == 0xFFFFFFFF as header_field's int32
C2 = dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
WIDE = dict(num_executors=100, job_arrival_cap=200, job_arrival_rate=8.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
# Episodes at C2 sizing last 500 - 750 steps under this policy, the emulator takes about 0.2 s per batched step of 70 envs, and the
# run has to meet ends of episodes and auto-resets within 150 steps: the envs get a time limit (ms of simulated time) that ends an
# episode after some tens of steps. Checked with these seeds: every property asserted below is met dozens of times.
SHORT_EPISODES = 40000.0


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def reference_actions(env, param: int):
    """(stage_idx, num_exec) int32 arrays: hash_policy(obs, seed, step, p_none_permille=param) of every env as it stands"""
    seed = env.header_field("seed").cpu().numpy().astype(np.int64)
    step = env.header_field("ep_steps").cpu().numpy().astype(np.int64)
    oi = env.obs_i32.cpu().numpy()
    si, ne = np.empty(env.num_envs, np.int32), np.empty(env.num_envs, np.int32)
    for k in range(env.num_envs):
        n_sched, ncommit = int(oi[k, 3]), int(oi[k, 4])
        h = _splitmix64((((int(seed[k]) & M64) << 32) & M64) ^ int(step[k]))
        h2 = _splitmix64(h)
        h3 = _splitmix64(h2)
        si[k] = -1 if (n_sched == 0 or (h3 % 1000) < param) else h % n_sched
        ne[k] = 1 + h2 % max(1, ncommit)
    return si, ne


def device_actions(env, param: int):
    act = env.policy_actions("hash", param)  # (buffers the env re-uses: copies)
    return act["stage_idx"].clone(), act["num_exec"].clone()


def compare_trajectory(env, param: int, steps: int, also=(), revive=None):
    """`policy_actions("hash", param)` against the reference on the state as it stands and after each of `steps` step_async calls
    fed with those actions; `also`: further params compared on every state (the policy launch changes nothing). Returns how often
    the states met: no source or nothing committable, nothing schedulable, an env right after an auto-reset. `revive`: {"seed", "options"}
    for the `reset` of envs that failed."""
    met = dict(no_commit=0, no_sched=0, after_reset=0)
    for t in range(steps + 1):
        si, ne = device_actions(env, param)
        for p in (param, *also):
            d_si, d_ne = (si, ne) if p == param else device_actions(env, p)
            r_si, r_ne = reference_actions(env, p)
            assert np.array_equal(d_si.cpu().numpy(), r_si), (p, t, np.flatnonzero(d_si.cpu().numpy() != r_si)[:8])
            assert np.array_equal(d_ne.cpu().numpy(), r_ne), (p, t, np.flatnonzero(d_ne.cpu().numpy() != r_ne)[:8])
            if p == 1000:
                assert (r_si == -1).all(), t
        oi = env.obs_i32.cpu().numpy()
        src = env.header_field("curr_source").cpu().numpy()
        no_commit = (src == POOL_NONE) | (oi[:, 4] == 0)
        no_sched = oi[:, 3] == 0
        ne_h, si_h = ne.cpu().numpy(), si.cpu().numpy()
        assert (ne_h[no_commit] == 1).all() and (si_h[no_sched] == -1).all(), t
        fresh = (env.header_field("ep_steps").cpu().numpy() == 0) & (env.header_field("episodes").cpu().numpy() > 0)
        met["no_commit"] += int(no_commit.sum())
        met["no_sched"] += int(no_sched.sum())
        met["after_reset"] += int(fresh.sum())
        if t < steps:
            env.step_async(si, ne)
            # With stage_idx = -1 draws an env can stall as the reference does (AssertionError "[step]", SSS_ERR_STALLED) and
            # stays failed from then on: such envs start over with seeds of their own, so that the run keeps moving
            failed = env.obs_i32[:, 7] != 0
            if revive is not None and bool(failed.any()):
                env.reset(seed=revive["seed"] + 1000 * (t + 1), options=revive.get("options"), mask=failed)
    return met


@pytest.mark.parametrize("param", [0, 300])
def test_hash_actions_c2_with_auto_reset(param, pack):
    """C2 sizing, 70 envs (not a multiple of 64), auto-reset; param = 1000 (every stage_idx -1, num_exec as the reference's) rides
    on the same states"""
    env = VecSparkSchedSimEnv(C2, 70, device="cpu", pack=pack, _lib=load_emu(), auto_reset=True)
    options = {"time_limit": SHORT_EPISODES}
    env.reset(seed=4000, options=options)
    met = compare_trajectory(env, param, 150, also=(1000,), revive=dict(seed=4000, options=options))
    env.close()
    assert met["no_commit"] > 0 and met["no_sched"] > 0 and met["after_reset"] > 0, met


def test_hash_actions_wide(pack):
    """the wide instantiation (100 executors, 200 jobs): its own SssHot, so its own offsets of the pool records"""
    env = VecSparkSchedSimEnv(WIDE, 3, device="cpu", pack=pack, _lib=load_emu())
    env.reset(seed=[11, 12, 13])
    compare_trajectory(env, 300, 40, also=(0,), revive=dict(seed=11))
    env.close()


@pytest.mark.parametrize("param", [0, 300])
def test_first_action_of_fused_rollout_is_the_policy_launch_action(param, pack):
    """one definition of the arithmetic: the first action of a one-step fused rollout under the hash policy (policy_hash, from
    the staged env) is what `policy_actions("hash")` returns on the same state (policy_hash_direct, from the HBM image)"""
    B = 6
    env = VecSparkSchedSimEnv(C2, B, device="cpu", pack=pack, _lib=load_emu())
    env.reset(seed=70)
    pol = torch.full((B,), POLICY_IDS["hash"], dtype=torch.int32)
    par = torch.full((B,), param, dtype=torch.int32)
    for rnd in range(4):
        assert int((env.obs_i32[:, 6:8] != 0).sum()) == 0, rnd  # every env takes part: none over, none failed
        snap = env.snapshot()
        si, ne = device_actions(env, param)
        out = env.rollout_each(pol, par, 1)
        assert (out["steps"] == 1).all(), rnd
        assert torch.equal(out["first_stage_idx"], si) and torch.equal(out["first_num_exec"], ne), rnd
        env.restore(snap)
        si2, ne2 = device_actions(env, param)
        assert torch.equal(si2, si) and torch.equal(ne2, ne), rnd
        r_si, r_ne = reference_actions(env, param)
        assert np.array_equal(si.numpy(), r_si) and np.array_equal(ne.numpy(), r_ne), rnd
        env.rollout("hash", 9, param)  # on to another state
        failed = env.obs_i32[:, 7] != 0  # (stage_idx = -1 draws can stall an env, as they stall the reference)
        if bool(failed.any()):
            env.reset(seed=70 + 100 * (rnd + 1), mask=failed)
    env.close()
