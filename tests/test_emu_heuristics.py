"""The on-device weighted-fair and SJF-CP policies (csrc/sss_sim.h policy_wfair / policy_sjfcp) under the CPU wave emulator: they
reproduce the action streams the host plugins produced on the reference env (tests/golden/make_heuristic_golden.py), with the
recorded rewards and wall times, in both instantiations (<= 64 executors and the wide one); weighted fair with alpha = 0 is the
fair policy; the fused rollout lands in the recorded final state; the C ABI rejects an alpha outside [-4, 4]."""
import ctypes as C

import pytest

from emu_util import load_emu
from golden_util import Golden, bits
from spark_sched_sim_amd import VecSparkSchedSimEnv
from test_emu_policies import run_policy_episode


def run_set(name, seeds, pack, max_steps=None, fused=0, device="cpu", lib=None, policy=None, param=None):
    g = Golden(name)
    policy = g.policy if policy is None else policy
    param = int(g.z["param"]) if param is None else param
    return run_policy_episode(name, policy, param, seeds, g.pack(pack), device=device, lib=lib, max_steps=max_steps, fused=fused)


@pytest.mark.parametrize("name,seeds,max_steps", [
    ("c1_wfair_m1", [0, 1], None),
    ("c1_wfair_p1", [4], None),
    ("c1_sjfcp", [0, 3], None),
    ("c3_wfair_m1", [0], 400),
    ("c3_sjfcp", [1], 400),
    ("e100_wfair_m1", [0], 300),
    ("e100_sjfcp", [2], 300),
    ("deep_c1_sjfcp", [0], 150),
])
def test_device_heuristic_reproduces_recorded_actions(name, seeds, max_steps, pack):
    bad = run_set(name, seeds, pack, max_steps=max_steps, lib=load_emu())
    assert not bad, "\n".join(bad[:10])


def run_time_limited(name, seeds, pack, device="cpu", lib=None):
    """run_policy_episode's step-wise leg for a set bounded by a time limit instead of a job cap (the env needs a job capacity
    and the limit; tests/replay_util.py does the same for recorded action streams)"""
    g = Golden(name)
    env = VecSparkSchedSimEnv(dict(g.cfg, max_jobs=64), len(seeds), device=device, pack=g.pack(pack), _lib=lib)
    env.reset(seed=seeds, options={"time_limit": g.time_limit})
    n_rec = [len(g.ep(s, "reward")) for s in seeds]
    bad = []
    for i in range(1, max(n_rec)):
        act = env.policy_actions(g.policy, int(g.z["param"]))
        si, ne = act["stage_idx"].cpu().numpy().copy(), act["num_exec"].cpu().numpy().copy()
        env.step(act)
        of = env.obs_f64.cpu().numpy()
        for k, s in enumerate(seeds):
            if i >= n_rec[k]:
                continue
            exp = (int(g.ep(s, "stage_idx")[i]), int(g.ep(s, "num_exec")[i]))
            if (int(si[k]), int(ne[k])) != exp or bits(of[k, 0]) != int(g.ep(s, "reward")[i]) or bits(of[k, 1]) != int(g.ep(s, "wall_time")[i]):
                bad.append(f"{name} seed {s} step {i}: action {(int(si[k]), int(ne[k]))} expected {exp}")
    env.close()
    return bad


def test_device_heuristic_time_limited_set(pack):
    bad = run_time_limited("tiny_wfair_p2_tlimit", list(range(6)), pack, lib=load_emu())
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("name,seeds,max_steps", [
    ("c1_fair", [1234, 0], None),
    ("c3_fair", [0], 400),
    ("e100_fair", [0], 300),
])
def test_wfair_alpha_zero_reproduces_fair(name, seeds, max_steps, pack):
    bad = run_set(name, seeds, pack, max_steps=max_steps, lib=load_emu(), policy="wfair", param=0)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("name,seeds", [("c1_wfair_m1", [2]), ("c1_sjfcp", [1]), ("e100_sjfcp", [3])])
def test_fused_rollout_ends_in_recorded_state(name, seeds, pack):
    bad = run_set(name, seeds, pack, lib=load_emu(), fused=1)
    assert not bad, "\n".join(bad[:10])


def test_abi_rejects_alpha_out_of_range(pack):
    g = Golden("c1_fair")
    env = VecSparkSchedSimEnv(g.cfg, 2, device="cpu", pack=pack, _lib=load_emu())
    env.reset(seed=[0, 1])
    for alpha in (5, -5):
        with pytest.raises(ValueError, match="alpha"):
            env.policy_actions("wfair", alpha)
        with pytest.raises(ValueError, match="alpha"):
            env.rollout("wfair", 3, alpha)
    # the library itself, past the Python check: -23 with a message that names alpha; unknown ids stay -23
    lib = env._b.lib
    rc = lib.sss_policy(env._h, 3, 5, env._act_stage.data_ptr(), env._act_nexec.data_ptr(), env._stream())
    assert rc == -23 and b"alpha" in lib.sss_last_error()
    assert lib.sss_rollout(env._h, 3, -5, 1, 0, C.c_uint64(0), env._stream()) == -23
    assert lib.sss_policy(env._h, 5, 0, env._act_stage.data_ptr(), env._act_nexec.data_ptr(), env._stream()) == -23
    # ... and the env is untouched: alpha in range still runs
    for alpha in range(-4, 5):
        env.policy_actions("wfair", alpha)
    env.policy_actions("sjfcp")
    assert int(env.header(0)["ep_steps"]) == 0
    env.close()
