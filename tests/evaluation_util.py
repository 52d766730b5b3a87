"""shared by tests/test_emu_evaluation.py (CPU wave emulator, 6 envs) and tests/test_gpu_evaluation.py (MI355X, 96 envs: several waves,
episodes that end in different windows of the 64-step done-mask check): `spark_sched_sim_amd.evaluation` and the trainer's held-out
evaluation - `run_episodes` against a hand-written loop for an on-device heuristic and for a DecimaPolicy, `compare`, and that
evaluating while training leaves the training run's parameters bit for bit what they are without it."""
import contextlib

import numpy as np
import pytest
import torch

CFG = dict(num_executors=10, job_arrival_cap=8, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
SEED = 4100
SKIP = -2 ** 31  # training.SKIP_ENV: the env sits the step out


def make_env(device, lib, B, **kw):
    from spark_sched_sim_amd import VecSparkSchedSimEnv

    return VecSparkSchedSimEnv(CFG, B, device=device, _lib=lib, **kw)


def make_policy(device):
    from decima_util import AGENT
    from spark_sched_sim_amd.decima import DecimaPolicy

    torch.manual_seed(5)
    return DecimaPolicy(num_executors=10, **AGENT).to(device).eval()


def host_stats(env):
    """(avg_num_jobs, the episode's mean job duration, the ring's mean in seconds, percentiles) of every env by the host functions"""
    from spark_sched_sim_amd import metrics

    rows = []
    for i in range(env.num_envs):
        d = metrics.job_durations(env, i)
        rows.append((metrics.avg_num_jobs(env, i), np.mean(d), np.mean(env.job_duration_buff(i)).item() * 1e-3, np.percentile(d, [25, 50, 75, 100])))
    return rows


def check_result(r, env, steps):
    B = env.num_envs
    assert bool(r["ok"].all()) and r["ok"].shape == (B,)
    assert r["steps"].tolist() == steps
    for i, (anj, mean, ring_s, pct) in enumerate(host_stats(env)):
        assert float(r["avg_num_jobs"][i]) == anj and float(r["avg_job_duration"][i]) == mean and float(r["avg_job_duration_s"][i]) == ring_s
        assert float(r["episode_avg_job_duration_s"][i]) == mean * 1e-3
        assert r["pct"][i].tolist() == pct.tolist()
        assert int(r["num_jobs"][i]) == 8 and int(r["num_completed_jobs"][i]) == 8 and int(r["num_active_jobs"][i]) == 0


def check_on_device_policy(device, lib, B, actor="fair", chunk=16):
    """`run_episodes` under an on-device heuristic against one step at a time, every env until its own end: per-env step counts, `ok`,
    every statistic bit for bit against the host functions of `metrics`; an auto-resetting env is refused"""
    from spark_sched_sim_amd.evaluation import run_episodes

    env, ref = make_env(device, lib, B), make_env(device, lib, B)
    r = run_episodes(env, actor, SEED, chunk=chunk)
    ref.reset(seed=SEED)
    steps = torch.zeros(B, dtype=torch.long)
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=ref.device)
    for _ in range(4000):
        term = ref.header_field("terminated") != 0
        if bool(term.all()):
            break
        act = ref.policy_actions(actor)
        ref.step_async(torch.where(term, skip, act["stage_idx"]).contiguous(), act["num_exec"])
        steps += (~term).cpu().long()
    assert bool((ref.header_field("terminated") != 0).all())
    check_result(r, env, steps.tolist())
    check_result(r, ref, steps.tolist())  # (the same episodes: the same statistics from the other env's arena)
    with pytest.raises(ValueError, match="auto-reset"):
        run_episodes(make_env(device, lib, 2, auto_reset=True), "fair", 1)
    env.close(), ref.close()
    return steps


@contextlib.contextmanager
def no_transfer_inside(*owners_and_names):
    """torch.cuda.set_sync_debug_mode("error") inside every call of the given (object, method name) pairs, from each one's second call
    on (the first sizes work space). Only the inside of those calls is under the mode: what the caller does between them (in
    `run_episodes`, the `torch.where` on the actions and the update of the done mask - tensor ops on the device) is not."""
    seen = {}

    def wrap(obj, name):
        fn = getattr(obj, name)

        def call(*a, **k):
            seen[name] = seen.get(name, 0) + 1
            if seen[name] == 1:
                return fn(*a, **k)
            prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                return fn(*a, **k)
            finally:
                torch.cuda.set_sync_debug_mode(prev)
        setattr(obj, name, call)
    for obj, name in owners_and_names:
        wrap(obj, name)
    try:
        yield seen
    finally:
        for obj, name in owners_and_names:
            delattr(obj, name)


def check_decima(device, lib, B, greedy, oracle_envs=(), no_transfer=False):
    """`run_episodes` under a DecimaPolicy against the hand-written `schedule_env` + `step_async` loop on a second env: the checks of
    `check_on_device_policy` plus `compare`'s paired figures; the draw counter is unmoved after a greedy run. `oracle_envs` (greedy):
    the hand-written loop's actions of these envs replayed through the C oracle - its job completion times give the same
    `avg_job_duration` and percentiles. `no_transfer`: the policy and step launches of `run_episodes` make no device->host transfer
    (`no_transfer_inside`). This is where the greedy route runs under the sync-debug mode; the trainer's own evaluation
    (`check_evaluating_while_training`, sampled and on an env the trainer creates) is not run under it."""
    from spark_sched_sim_amd.evaluation import compare, run_episodes

    env, ref, policy = make_env(device, lib, B), make_env(device, lib, B), make_policy(device)
    gen = torch.Generator().manual_seed(3)
    calls = getattr(policy, "_calls", 0)
    with (no_transfer_inside((policy, "schedule_env"), (env, "step_async")) if no_transfer else contextlib.nullcontext({})) as seen:
        r = run_episodes(env, policy, SEED, greedy=greedy, generator=gen)
    assert not no_transfer or (seen["schedule_env"] == seen["step_async"] and seen["schedule_env"] >= 64)
    n_calls = getattr(policy, "_calls", 0) - calls
    assert (n_calls == 0) if greedy else (n_calls > 0 and n_calls % 64 == 0)
    policy._calls = calls
    ref.reset(seed=SEED)
    steps, done = torch.zeros(B, dtype=torch.long), torch.zeros(B, dtype=torch.bool, device=ref.device)
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=ref.device)
    gen = torch.Generator().manual_seed(3)
    rec = []
    for _ in range(n_calls if not greedy else 4000):  # (a sampled run: the same number of draws, so the same stream)
        if greedy and bool(done.all()):
            break
        act, _ = policy.schedule_env(ref, generator=gen, active=~done, greedy=greedy)
        stage = torch.where(done, skip, act["stage_idx"]).contiguous()
        if oracle_envs:
            rec.append((stage.cpu().numpy().copy(), act["num_exec"].cpu().numpy().copy()))
        ref.step_async(stage, act["num_exec"])
        steps += (~done).cpu().long()
        done = done | (ref.obs_i32[:, 6] != 0) | (ref.obs_i32[:, 7] != 0)
    assert bool(done.all())
    steps = steps.tolist()
    check_result(r, env, steps)
    check_result(r, ref, steps)
    if B > 64:  # episodes end in more than one window of the done-mask check
        assert len({(s - 1) // 64 for s in steps}) > 1, sorted(set(steps))
    for b in oracle_envs:
        check_against_oracle(b, [(int(s[b]), int(n[b])) for s, n in rec][: steps[b]], r)
    fair = run_episodes(ref, "fair", SEED)
    c = compare({"fair": fair, "decima": r})
    assert c["envs_compared"] == B and c["envs_excluded"] == 0 and c["fair"]["minus_fair_s"] == 0.0
    ok = fair["ok"] & r["ok"]  # (all envs; indexed as `compare` does, so that a device reduction adds the same values in the same order)
    d = r["avg_job_duration_s"][ok] - fair["avg_job_duration_s"][ok]
    assert c["decima"]["minus_fair_s"] == float(d.mean()), (c["decima"]["minus_fair_s"], float(d.mean()))
    # (a device reduction takes a mean as sum x (1 / n): one rounding away from numpy's sum / n at most; exact on the CPU)
    got, want = c["decima"]["steps_per_episode"], float(np.mean(steps))
    assert got == want if env.device.type == "cpu" else abs(got - want) <= np.spacing(want), (got, want)
    pooled = np.sort(r["sorted"].cpu().numpy()[:, :8].ravel())
    assert np.allclose(c["decima"]["job_duration_percentiles"]["pooled"], np.percentile(pooled, [25, 50, 75, 100]), rtol=1e-12)
    env.close(), ref.close()


def check_against_oracle(b, actions, r):
    """env `b`'s recorded actions through the C oracle: it terminates with the last one, and its job times give `run_episodes`' mean job
    duration and percentiles of that env"""
    from oracle_binding import OracleEnv
    from spark_sched_sim_amd import workload

    o = OracleEnv(workload.default_pack(), CFG)
    assert o.reset(SEED + b) == 0
    for t, (stage, n_exec) in enumerate(actions):
        err, _, term = o.step(stage, n_exec)
        assert err == 0 and term == (t == len(actions) - 1), (b, t, err, term)
    ta, tc, _, _ = o.job_times()
    assert len(ta) == 8
    d = np.minimum(tc, o.info().wall_time) - ta
    assert float(r["avg_job_duration"][b]) == np.mean(list(d)), b
    assert r["pct"][b].tolist() == np.percentile(list(d), [25, 50, 75, 100]).tolist(), b
    o.close()


def check_evaluating_while_training(device, lib, tmp_path):
    from training_util import reference_smoke_test_config
    from spark_sched_sim_amd.training import Trainer

    def run(**extra):
        cfg = reference_smoke_test_config(str(tmp_path / "a"))
        cfg["env"].update(num_executors=10, job_arrival_cap=4, mean_time_limit=1.5e5)
        cfg["trainer"].update(num_iterations=2, deterministic=True, num_epochs=1, num_batches=2, **extra)
        tr = Trainer(cfg["agent"], cfg["env"], cfg["trainer"], device=device, _lib=lib)
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
