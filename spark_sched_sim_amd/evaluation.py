"""Evaluating schedulers on held-out job sequences: whole episodes of every env of a `VecSparkSchedSimEnv` under an on-device
heuristic or a `DecimaPolicy`, the per-env episode metrics from one kernel launch (`env.job_stats`, include/sss.h sss_job_stats),
and the paired comparison of several schedulers on the same seeds (the reference's one published comparison, README.md:5-7 with
examples.py:84-102). `tools/decima_vs_fair.py`, `tools/heuristic_baselines.py` and `training.Trainer` (`eval_every`) use it."""
from __future__ import annotations

from typing import Any, Sequence

import torch

from .binding import JOB_STATS_COLUMNS

DECISION_CHECK_EVERY = 64  # Decima-in-the-loop steps between two reads of the done mask (one device->host sync each)


def _summarize(env, q: Sequence[float]) -> dict[str, torch.Tensor]:
    r = env.job_stats(q, want_sorted=True)
    out = {name: r["stats"][:, k].clone() for k, name in enumerate(JOB_STATS_COLUMNS)}
    out["avg_job_duration_s"] = out["avg_completed_job_duration"]  # (the tools' key: the reference's env.avg_job_duration)
    # ... and the episode's own mean job duration in seconds: the ring outlives reset() (as the reference's job_duration_buff does), so on
    # an env that played other episodes before and holds fewer than 200 jobs per episode the column above averages those in
    out["episode_avg_job_duration_s"] = out["avg_job_duration"] * 1e-3
    out["pct"], out["sorted"] = r["pct"].clone(), r["sorted"].clone()
    out["q"] = torch.tensor([float(x) for x in q], dtype=torch.float64)
    out["ok"] = ((env.header_field("terminated") != 0) & (env.obs_i32[:, 7] == 0)).clone()
    out["steps"] = env.header_field("ep_steps").clone()  # step() calls of the episode
    return out


@torch.no_grad()
def run_episodes(env, actor, seed, max_steps: int = 200_000, *, param: int = 0, greedy: bool = False, generator: torch.Generator | None = None,
                 q: Sequence[float] = (25, 50, 75, 100), chunk: int = 200, fused: bool = False) -> dict[str, torch.Tensor]:
    """every env of `env` (no auto-reset) plays one whole episode from `reset(seed=seed)` under `actor`:
      - the name of an on-device policy ("fair", "fifo", "wfair", "sjfcp", "hash") with `param`: fused `env.rollout` launches of
        `chunk` steps, the done mask read after each;
      - a `DecimaPolicy` (`greedy`: arg-max actions - they leave the policy's draw counter alone; else draws from `generator`):
        policy and step launches in lock step, finished or failed envs sit the remaining launches out (SSS_SKIP_ENV), the done
        mask read every 64 steps. With `fused=True`: `DecimaPolicy.rollout_env` launches of `chunk` steps instead, the done mask read
        after each - every env at its own pace, the episodes of the lock-step loop under `one_launch=True` bit for bit (`greedy`), or
        draws keyed by `generator`'s seed and the policy's draw counter, which advances by the steps played. Not while a timeline
        is recorded; profiles/fused_decima.md says at which sizes it is the faster route.
    At most `max_steps` steps per env. Returns per-env DEVICE tensors the caller owns: the columns of `env.job_stats`
    (`binding.JOB_STATS_COLUMNS`; `avg_job_duration_s` = the mean over the last <= 200 completed jobs in seconds), `pct` f64[B, len(q)]
    with `q`, `sorted` (the env's sorted job durations, NaN behind them), `ok` (the episode ended without an env error) and `steps`."""
    from .training import SKIP_ENV

    B, dev = env.num_envs, env.device
    if env.auto_reset:
        raise ValueError("run_episodes: the env must not auto-reset (a finished episode's statistics are read from its arena block)")
    env.reset(seed=seed)
    if isinstance(actor, str):
        for _ in range(max(1, -(-int(max_steps) // int(chunk)))):
            env.rollout(actor, int(chunk), param)
            if bool(((env.header_field("terminated") != 0) | (env.obs_i32[:, 7] != 0)).all()):
                break
        return _summarize(env, q)
    if fused:
        c0, t = getattr(actor, "_calls", 0) + 1, 0
        while t < max_steps:
            n = min(int(chunk), int(max_steps) - t)
            actor.rollout_env(env, n, greedy=greedy, seed=generator.initial_seed() if generator is not None else 0, counter=c0 + t)
            t += n
            if bool(((env.header_field("terminated") != 0) | (env.obs_i32[:, 7] != 0)).all()):
                break
        if not greedy:
            actor._calls = c0 - 1 + t
        return _summarize(env, q)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    skip = torch.full((B,), SKIP_ENV, dtype=torch.int32, device=dev)
    t = 0
    while t < max_steps:
        for _ in range(DECISION_CHECK_EVERY):
            act, _ = actor.schedule_env(env, generator=generator, active=~done, greedy=greedy)
            env.step_async(torch.where(done, skip, act["stage_idx"]).contiguous(), act["num_exec"])
            done = done | (env.obs_i32[:, 6] != 0) | (env.obs_i32[:, 7] != 0)
            t += 1
        if bool(done.all()):
            break
    return _summarize(env, q)


@torch.no_grad()
def continuations(env, src, dst, policy, param: int = 0, reseed=None, max_steps: int = 200_000, *, q: Sequence[float] = (25, 50, 75, 100),
                  check_every: int = DECISION_CHECK_EVERY, fused: bool = False, horizon: float | None = None, tail: str = "srpt") -> dict[str, torch.Tensor]:
    """the cost-to-go of env states under an on-device policy: `env.fork(src, dst, reseed)` - `reseed` gives every child its own
    task-duration noise on the parent's job sequence - then ONLY the `dst` envs play to the end of their episodes under `policy` /
    `param` (`VecSparkSchedSimEnv.policy_actions`); every other env sits the launches out (SSS_SKIP_ENV) and keeps its state,
    outputs and counters byte for byte. `src` / `dst`: host-side ids (their number sizes the result). Returns the `run_episodes`
    dict with one row per child, in the order of `dst` (`ok`: the child's episode ended without an env error); the done mask is read
    every `check_every` steps, at most `max_steps` steps are played.
    `fused=True`: the children play in ONE launch of the fused rollout with a policy per env (`env.rollout_each`) instead of a policy
    and a step launch per step of the longest child - the same results, bit for bit, and no done mask to read; not available while
    the env records a timeline.
    `horizon` (with `fused=True` only; simulated time, > 0): the children stop that span after the fork instead (`env.rollout_until`);
    the dict then describes the states they stopped in (`ok`: the episode ENDED without an env error) and also holds `t_stop` f64[n],
    `rem_work` f64[n, job_cap] and `horizon_cost` f64[n]: the child's cost under `tail` as the horizon pick kernel computes it
    (`env.lookahead_pick_horizon`; `horizon_cost` below is the definition), NaN for a child that `max_steps` cut short.
    `policy` may also be a `DecimaPolicy` (with `fused=True` and without a horizon only; ValueError otherwise): the children play its
    arg-max decisions in one launch of `DecimaPolicy.rollout_env`; `param` is ignored."""
    from .binding import POLICY_DECIMA
    from .training import SKIP_ENV

    learned = not isinstance(policy, str)
    if learned and (not fused or horizon is not None):
        raise ValueError("continuations: a DecimaPolicy plays through the fused route only (fused=True) and has no stop time (horizon=None)")

    if horizon is not None and not fused:
        raise ValueError("continuations: a horizon needs fused=True (the lock-step route has no stop time)")

    if env.auto_reset:
        raise ValueError("continuations: the env must not auto-reset (a finished child's statistics are read from its arena block)")
    B, dev = env.num_envs, env.device
    dst_l = [int(dst)] if isinstance(dst, int) else [int(x) for x in dst]
    env.fork(src, dst_l, reseed=reseed)
    idx = torch.tensor(dst_l, dtype=torch.long).to(dev)
    child = torch.zeros(B, dtype=torch.bool, device=dev)
    child[idx] = True
    skip = torch.full((B,), SKIP_ENV, dtype=torch.int32, device=dev)
    done = ~child
    t = 0
    if fused:
        pid = POLICY_DECIMA if learned else env._policy_id(policy, param)
        sit_out = torch.full((B,), -1, dtype=torch.int32, device=dev)
        pol, par = torch.where(child, torch.full_like(sit_out, pid), sit_out), torch.where(child, torch.full_like(sit_out, int(param)), sit_out)
        if learned:
            policy.rollout_env(env, int(max_steps), greedy=True, policy=pol, param=par)
        elif horizon is None:
            env.rollout_each(pol, par, int(max_steps))
        else:
            until = env.rollout_until(pol, par, float(horizon), int(max_steps))
        t = max_steps
    while t < max_steps:
        for _ in range(min(int(check_every), max_steps - t)):
            done = done | (env.obs_i32[:, 6] != 0) | (env.obs_i32[:, 7] != 0)
            act = env.policy_actions(policy, param)
            env.step_async(torch.where(done, skip, act["stage_idx"]).contiguous(), act["num_exec"])
            t += 1
        if bool((done | (env.obs_i32[:, 6] != 0) | (env.obs_i32[:, 7] != 0)).all()):
            break
    r = env.job_stats(q, active=child, want_sorted=True)
    out = {name: r["stats"][idx, k].clone() for k, name in enumerate(JOB_STATS_COLUMNS)}
    out["avg_job_duration_s"] = out["avg_completed_job_duration"]
    out["episode_avg_job_duration_s"] = out["avg_job_duration"] * 1e-3
    out["pct"], out["sorted"] = r["pct"][idx].clone(), r["sorted"][idx].clone()
    out["q"] = torch.tensor([float(x) for x in q], dtype=torch.float64)
    out["ok"] = ((env.header_field("terminated") != 0) & (env.obs_i32[:, 7] == 0))[idx].clone()
    out["steps"] = env.header_field("ep_steps")[idx].clone()
    if horizon is not None:
        # every child as the one child of a parent of its own: score = cost / 1. (The decision goes to arrays nobody reads.)
        n = len(dst_l)
        ids = idx.to(torch.int32)
        one = {k: torch.zeros(1, dtype=torch.int32, device=dev) for k in ("first_policy", "first_param", "policy", "param")}
        scratch = {k: torch.zeros(B, dtype=torch.int32, device=dev) for k in one}
        cost = torch.zeros((n, 1), dtype=torch.float64, device=dev)
        env.lookahead_pick_horizon(ids, ids.reshape(n, 1, 1), one, until["t_stop"], until["rem_work"], tail, torch.zeros(n, dtype=torch.int32, device=dev), cost, scratch)
        out["t_stop"], out["rem_work"], out["horizon_cost"] = until["t_stop"][idx].clone(), until["rem_work"][idx].clone(), cost[:, 0].clone()
    return out


def horizon_cost(t_arrival, t_completed, wall: float, t_stop: float, rem_work, num_executors: int, terminated: bool, tail: str = "srpt") -> float:
    """the cost of ONE child that stopped at a time horizon, in plain Python floats - the definition that
    `env.lookahead_pick_horizon` (include/sss.h sss_lookahead_pick_horizon) computes on the device, bit for bit; the order of every
    sum is part of it. `t_arrival` / `t_completed`: the arrived jobs in id order (`env.job_times(i)` up to the header's
    `next_arrival`; an unfinished job's completion time is inf), `wall`: the child's wall time, `t_stop`: T, the time all children
    of its parent were to reach, `rem_work[j]`: the work job j still holds (`env.rollout_until`), `terminated`: its episode is over.
    NaN for a child that is not valid: it neither ended nor reached T. (An env error makes a child invalid as well; the caller
    knows.) Counted are the jobs that arrived before T - the same jobs in every child of a parent, so the costs are comparable.
      tail "none": every counted job is charged up to min(T, wall) - nothing beyond the common time T;
      tail "srpt": up to the child's own `wall`, plus - unless it is terminated - the flow time the unfinished counted jobs would
                   still accrue if the `num_executors` executors served them as one machine, shortest remaining work first."""
    T, w = float(t_stop), float(wall)
    if not (terminated or w >= T):
        return float("nan")
    if tail not in ("none", "srpt"):
        raise ValueError(f"horizon_cost: tail must be 'none' or 'srpt', got {tail!r}")
    counted = [j for j in range(len(t_arrival)) if float(t_arrival[j]) < T]
    upto = w if tail == "srpt" else min(T, w)
    total = 0.0
    for j in counted:
        total = total + (min(float(t_completed[j]), upto) - float(t_arrival[j]))
    if tail == "none" or terminated:
        return total
    left = sorted(float(rem_work[j]) for j in counted if float(t_completed[j]) > w)
    p, rest = 0.0, 0.0
    for W in left:
        p = p + W
        rest = rest + p / float(num_executors)
    return total + rest


@torch.no_grad()
def run_lookahead(env, scheduler, seed, *, q: Sequence[float] = (25, 50, 75, 100), check_every: int = DECISION_CHECK_EVERY) -> dict[str, torch.Tensor]:
    """the parents of a `lookahead.LookaheadScheduler` - or of a `lookahead.ActionLookaheadScheduler`, whose "candidates" are the top-k
    slots - on `env` play one whole episode under it: parents and children are reset
    (`seed`: an int - parent number i gets seed + i - or one seed per parent; a child gets its parent's; no other env is touched by
    the reset), then `scheduler.decide_and_step()` until every parent's episode is over or `scheduler.max_steps` steps are played;
    the parents' done mask is read every `check_every` decisions (the one device->host sync). Returns the `run_episodes` dict with
    one row per parent, in the scheduler's order - `evaluation.compare` takes it beside the candidates' own `run_episodes` on the
    same seeds - plus `winners` i32[decisions, P] (candidate index per decision and parent, -1 = no candidate was valid; rows past
    `decisions[p]`, the decisions parent p needed, are -1), `decisions` i64[P] and `fallbacks`."""
    if env.auto_reset:
        raise ValueError("run_lookahead: the env must not auto-reset (a finished episode's statistics are read from its arena block)")
    B, dev, P = env.num_envs, env.device, len(scheduler.parents)
    seeds = [int(seed) + i for i in range(P)] if isinstance(seed, int) else [int(s) for s in seed]
    if len(seeds) != P:
        raise ValueError(f"run_lookahead: need one seed per parent ({P}), got {len(seeds)}")
    per_env, mask = [0] * B, [0] * B
    per_child = len(scheduler.children) // P
    for i, p in enumerate(scheduler.parents):
        per_env[p], mask[p] = seeds[i], 1
        for c in scheduler.children[i * per_child: (i + 1) * per_child]:
            per_env[c], mask[c] = seeds[i], 1
    env.reset(seed=per_env, mask=torch.tensor(mask, dtype=torch.uint8).to(dev))
    scheduler.reset()
    idx = torch.tensor(scheduler.parents, dtype=torch.long).to(dev)
    while scheduler.decisions * scheduler.replan_every < scheduler.max_steps:
        for _ in range(int(check_every)):
            scheduler.decide_and_step()
        if bool(((env.obs_i32[idx, 6] != 0) | (env.obs_i32[idx, 7] != 0)).all()):
            break
    parent = torch.zeros(B, dtype=torch.bool, device=dev)
    parent[idx] = True
    r = env.job_stats(q, active=parent, want_sorted=True)
    out = {name: r["stats"][idx, k].clone() for k, name in enumerate(JOB_STATS_COLUMNS)}
    out["avg_job_duration_s"] = out["avg_completed_job_duration"]
    out["episode_avg_job_duration_s"] = out["avg_job_duration"] * 1e-3
    out["pct"], out["sorted"] = r["pct"][idx].clone(), r["sorted"][idx].clone()
    out["q"] = torch.tensor([float(x) for x in q], dtype=torch.float64)
    out["ok"] = ((env.header_field("terminated") != 0) & (env.obs_i32[:, 7] == 0))[idx].clone()
    out["steps"] = env.header_field("ep_steps")[idx].clone()
    out["decisions"] = (out["steps"].long() + scheduler.replan_every - 1) // scheduler.replan_every
    w = scheduler.winners().clone()
    late = torch.arange(w.shape[0], device=dev)[:, None] >= out["decisions"][None, :]
    out["winners"] = torch.where(late, torch.full_like(w, -1), w)
    out["fallbacks"] = int((out["winners"][~late] == -1).sum()) if w.numel() else 0
    return out


def _ci95(v: torch.Tensor, n: int) -> float:
    return float(1.96 * v.std() / n ** 0.5)


def pooled_percentiles(sorted_rows: torch.Tensor, q: Sequence[float]) -> list[float]:
    """percentiles (linear interpolation, as numpy's default) of ALL the job durations in `sorted_rows` f64[n, job_cap] (NaN = no job)"""
    v = sorted_rows.reshape(-1)
    v = v[~torch.isnan(v)].sort().values
    n = v.numel()
    if n == 0:
        return [float("nan")] * len(q)
    pos = torch.tensor([float(x) for x in q], dtype=torch.float64, device=v.device) / 100.0 * (n - 1)
    lo = pos.floor().long().clamp(0, n - 1)
    hi = (lo + 1).clamp(max=n - 1)
    g = pos - lo.to(torch.float64)
    return (v[lo] + (v[hi] - v[lo]) * g).tolist()


def compare(results: dict[str, dict[str, torch.Tensor]], baseline: str = "fair", metric: str = "avg_job_duration_s") -> dict[str, Any]:
    """mean / 95 % confidence interval per scheduler over the envs where EVERY scheduler finished its episode without error (a sampled
    action sequence can run into the reference's own "[step]" stall), the paired difference to `baseline` (key
    `minus_<baseline>_s`), and the percentiles of the job durations pooled over those envs (`job_duration_percentiles`, in the
    simulator's time unit, with the per-env percentiles' mean beside them). `metric`: the per-env figure compared under the key
    `avg_job_duration_s` - `run_episodes`' `avg_job_duration_s` (the reference's env.avg_job_duration) or `episode_avg_job_duration_s`
    (for envs that are reused from one evaluation to the next)"""
    ok = None
    for r in results.values():
        ok = r["ok"] if ok is None else ok & r["ok"]
    n = int(ok.sum())
    out: dict[str, Any] = {"envs_compared": n, "envs_excluded": int((~ok).sum()), "metric": metric}
    base = results[baseline][metric][ok]
    for name, r in results.items():
        v = r[metric][ok]
        d = v - base
        row = {"avg_job_duration_s": float(v.mean()), "ci95": _ci95(v, n), "avg_num_jobs": float(r["avg_num_jobs"][ok].mean()),
               "steps_per_episode": float(r["steps"][ok].double().mean()),
               f"minus_{baseline}_s": float(d.mean()), f"minus_{baseline}_ci95": _ci95(d, n),
               f"envs_better_than_{baseline}": float((d < 0).double().mean())}
        if "sorted" in r:
            qs = r["q"].tolist()
            row["job_duration_percentiles"] = {"q": qs, "pooled": pooled_percentiles(r["sorted"][ok], qs), "mean_over_envs": r["pct"][ok].mean(0).tolist()}
        out[name] = row
    return out
