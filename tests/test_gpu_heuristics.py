"""-m gpu: the on-device weighted-fair and SJF-CP policies on a real MI355X - the recorded action streams of the host plugins on
the reference env (tests/golden/make_heuristic_golden.py), both kernel instantiations (e100_*: the wide one) and the deep trace
regime; weighted fair with alpha = 0 against the fair fixtures; the fused rollout against the recorded episodes; and at full
size (4096 envs, config 3) the device's actions against the host plugins on `obs_view(i)`, and fused against step-wise."""
import numpy as np
import pytest
import torch

from spark_sched_sim_amd import VecSparkSchedSimEnv
from spark_sched_sim_amd.schedulers import SJFCPScheduler, WeightedFairScheduler
from test_emu_heuristics import run_set, run_time_limited

pytestmark = pytest.mark.gpu

C3 = dict(num_executors=50, job_arrival_cap=200, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)


@pytest.mark.parametrize("name,seeds", [
    ("c1_wfair_m1", [0, 1, 2, 3]),
    ("c1_wfair_p1", [4, 5, 6]),
    ("c1_sjfcp", [0, 1, 2, 3]),
    ("c3_wfair_m1", [0]),
    ("c3_sjfcp", [1]),
    ("e100_wfair_m1", [0, 1]),
    ("e100_sjfcp", [2, 3]),
    ("deep_c1_sjfcp", [0]),
])
@pytest.mark.parametrize("fused", [0, 1])
def test_device_heuristic_reproduces_recorded_episodes_gpu(name, seeds, fused, pack):
    bad = run_set(name, seeds, pack, device="cuda:0", fused=fused)
    assert not bad, "\n".join(bad[:10])


def test_device_heuristic_time_limited_set_gpu(pack):
    bad = run_time_limited("tiny_wfair_p2_tlimit", list(range(6)), pack, device="cuda:0")
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("name,seeds", [("c1_fair", [1234] + list(range(20))), ("c3_fair", [0, 1]), ("e100_fair", [0, 1])])
def test_wfair_alpha_zero_reproduces_fair_gpu(name, seeds, pack):
    bad = run_set(name, seeds, pack, device="cuda:0", policy="wfair", param=0)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("policy,param", [("wfair", -2), ("wfair", -1), ("wfair", 1), ("sjfcp", 0)])
def test_full_size_batch_matches_host_plugin(policy, param, pack):
    """4096 c3 envs for 200 steps: at every step the device's action for 64 sampled envs equals the host plugin's on
    obs_view(i); then the same batch driven by the fused rollout reaches the same state"""
    B, T = 4096, 200
    a = VecSparkSchedSimEnv(C3, B, device="cuda:0", pack=pack)
    a.reset(seed=0)
    sched = WeightedFairScheduler(C3["num_executors"], param) if policy == "wfair" else SJFCPScheduler(C3["num_executors"])
    sample = np.random.default_rng(7).choice(B, size=64, replace=False).tolist()
    for t in range(T):
        act = a.policy_actions(policy, param)
        si, ne = act["stage_idx"].cpu().numpy(), act["num_exec"].cpu().numpy()
        for i in sample:
            exp, _ = sched.schedule(a.obs_view(i))
            assert (int(si[i]), int(ne[i])) == (int(exp["stage_idx"]), max(1, int(exp["num_exec"]))), (t, i)
        a.step(act)
    assert int((a.obs_i32[:, 7] != 0).sum()) == 0
    b = VecSparkSchedSimEnv(C3, B, device="cuda:0", pack=pack)
    b.reset(seed=0)
    b.rollout(policy, T, param)
    torch.cuda.synchronize()
    for field in ("wall_time", "ep_return", "n_events", "ep_steps"):
        assert torch.equal(a.header_field(field), b.header_field(field)), field
    assert torch.equal(a.obs_i32, b.obs_i32) and torch.equal(a.nodes, b.nodes)
    a.close()
    b.close()
