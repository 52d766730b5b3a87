"""`spark_sched_sim_amd.evaluation` and the trainer's held-out evaluation under the CPU wave emulator: `run_episodes` against a
hand-written loop for an on-device heuristic and for a DecimaPolicy, `compare`, and that evaluating while training leaves the
training run's parameters bit for bit what they are without it."""
import numpy as np
import pytest
import torch

from emu_util import load_emu

CFG = dict(num_executors=10, job_arrival_cap=8, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
B, SEED = 6, 4100


def make_env():
    from spark_sched_sim_amd import VecSparkSchedSimEnv

    return VecSparkSchedSimEnv(CFG, B, device="cpu", _lib=load_emu())


def make_policy():
    from decima_util import AGENT
    from spark_sched_sim_amd.decima import DecimaPolicy

    torch.manual_seed(5)
    return DecimaPolicy(num_executors=10, **AGENT).eval()


def host_stats(env):
    """(avg_num_jobs, the episode's mean job duration, the ring's mean in seconds, percentiles) of every env by the host functions"""
    from spark_sched_sim_amd import metrics

    rows = []
    for i in range(env.num_envs):
        d = metrics.job_durations(env, i)
        rows.append((metrics.avg_num_jobs(env, i), np.mean(d), np.mean(env.job_duration_buff(i)).item() * 1e-3, np.percentile(d, [25, 50, 75, 100])))
    return rows


def check_result(r, env, steps):
    assert bool(r["ok"].all()) and r["ok"].shape == (B,)
    assert r["steps"].tolist() == steps
    for i, (anj, mean, ring_s, pct) in enumerate(host_stats(env)):
        assert float(r["avg_num_jobs"][i]) == anj and float(r["avg_job_duration"][i]) == mean and float(r["avg_job_duration_s"][i]) == ring_s
        assert float(r["episode_avg_job_duration_s"][i]) == mean * 1e-3
        assert r["pct"][i].tolist() == pct.tolist()
        assert int(r["num_jobs"][i]) == 8 and int(r["num_completed_jobs"][i]) == 8 and int(r["num_active_jobs"][i]) == 0


def test_run_episodes_under_an_on_device_policy_equals_a_hand_written_loop():
    from spark_sched_sim_amd.evaluation import run_episodes

    env, ref = make_env(), make_env()
    r = run_episodes(env, "fair", SEED, chunk=16)
    ref.reset(seed=SEED)
    steps = [0] * B
    for _ in range(4000):  # one step at a time, every env until its own end
        term = ref.header_field("terminated").tolist()
        if all(term):
            break
        act = ref.policy_actions("fair")
        stage = torch.where(torch.tensor(term) != 0, torch.full((B,), -2 ** 31, dtype=torch.int32), act["stage_idx"])
        ref.step_async(stage.contiguous(), act["num_exec"])
        steps = [s + (0 if t else 1) for s, t in zip(steps, term)]
    assert all(ref.header_field("terminated").tolist())
    check_result(r, env, steps)
    check_result(r, ref, steps)  # (the same episodes: the same statistics from the other env's arena)
    with pytest.raises(ValueError, match="auto-reset"):
        from spark_sched_sim_amd import VecSparkSchedSimEnv
        run_episodes(VecSparkSchedSimEnv(CFG, 2, device="cpu", _lib=load_emu(), auto_reset=True), "fair", 1)
    env.close(), ref.close()


@pytest.mark.parametrize("greedy", [True, False])
def test_run_episodes_under_a_decima_policy_equals_a_hand_written_loop(greedy):
    from spark_sched_sim_amd.evaluation import compare, run_episodes

    env, ref, policy = make_env(), make_env(), make_policy()
    gen = torch.Generator().manual_seed(3)
    calls = getattr(policy, "_calls", 0)
    r = run_episodes(env, policy, SEED, greedy=greedy, generator=gen)
    n_calls = getattr(policy, "_calls", 0) - calls
    assert (n_calls == 0) if greedy else (n_calls > 0 and n_calls % 64 == 0)
    policy._calls = calls
    ref.reset(seed=SEED)
    steps, done = [0] * B, torch.zeros(B, dtype=torch.bool)
    gen = torch.Generator().manual_seed(3)
    for _ in range(n_calls if not greedy else 4000):  # (a sampled run: the same number of draws, so the same stream)
        if greedy and bool(done.all()):
            break
        act, _ = policy.schedule_env(ref, generator=gen, active=~done, greedy=greedy)
        ref.step_async(torch.where(done, torch.full((B,), -2 ** 31, dtype=torch.int32), act["stage_idx"]).contiguous(), act["num_exec"])
        steps = [s + (0 if d else 1) for s, d in zip(steps, done.tolist())]
        done = done | (ref.obs_i32[:, 6] != 0) | (ref.obs_i32[:, 7] != 0)
    assert bool(done.all())
    check_result(r, env, steps)
    check_result(r, ref, steps)
    fair = run_episodes(ref, "fair", SEED)
    c = compare({"fair": fair, "decima": r})
    assert c["envs_compared"] == B and c["envs_excluded"] == 0 and c["fair"]["minus_fair_s"] == 0.0
    d = (r["avg_job_duration_s"] - fair["avg_job_duration_s"])
    assert c["decima"]["minus_fair_s"] == float(d.mean()) and c["decima"]["steps_per_episode"] == float(np.mean(steps))
    pooled = np.sort(r["sorted"].numpy()[:, :8].ravel())
    assert np.allclose(c["decima"]["job_duration_percentiles"]["pooled"], np.percentile(pooled, [25, 50, 75, 100]), rtol=1e-12)
    env.close(), ref.close()


def test_evaluating_while_training_leaves_the_run_bit_for_bit(tmp_path):
    from training_util import reference_smoke_test_config
    from spark_sched_sim_amd.training import Trainer

    def run(**extra):
        cfg = reference_smoke_test_config(str(tmp_path / "a"))
        cfg["env"].update(num_executors=10, job_arrival_cap=4, mean_time_limit=1.5e5)
        cfg["trainer"].update(num_iterations=2, deterministic=True, num_epochs=1, num_batches=2, **extra)
        tr = Trainer(cfg["agent"], cfg["env"], cfg["trainer"], device="cpu", _lib=load_emu())
        tr.train(verbose=False)
        params = [p.detach().clone() for p in tr.policy.parameters()]
        hist = list(tr.eval_history)
        tr.close()
        return params, hist

    off, none = run()
    assert none == []
    # sampled evaluation: the harder case - it draws (from a generator of its own) and has to put the policy's draw counter back
    on, hist = run(eval_every=1, eval_envs=2, eval_seed=777, eval_greedy=False)
    assert len(hist) == 2 and [h["after_iterations"] for h in hist] == [1, 2]
    assert all(h["envs_compared"] + h["envs_excluded"] == 2 and "decima" in h and "fair" in h and h["greedy"] is False for h in hist)
    assert all(torch.equal(a, b) for a, b in zip(off, on))
