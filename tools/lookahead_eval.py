#!/usr/bin/env python3
"""The lookahead scheduler against its own candidates on held-out job sequences: `--envs` sequences (seeds --seed0 ...), every
candidate's whole episode (`evaluation.run_episodes`) and the lookahead's (`evaluation.run_lookahead`: fork, fused rollouts of the
children, the pick kernel, a step of the parents - four launches per decision), compared pairwise on the same seeds
(`evaluation.compare`). Writes the table to --out (profiles/lookahead.json) and prints it.

    python tools/lookahead_eval.py [--envs 256] [--samples 1] [--reseed N] [--replan-every 1] [--base name[:param]]
                                   [--policies fair,fifo,sjfcp,wfair:1] [--chunk 64] [--horizon MS[,MS...]] [--tail srpt|none] [--no-full]
                                   [--decima CHECKPOINT] [--topk K[,K...]]

Without --reseed the children continue the parent's own future (exact lookahead: never above a candidate's own episode); with it
every sample draws its own task durations (Monte-Carlo lookahead: what a scheduler that does not know the future can do).
With --horizon every listed horizon (simulated time; `LookaheadScheduler(horizon=, tail=)`) gets a run of its own beside the
candidates and the full-episode lookahead (--no-full leaves that one out): the episode's mean job duration and its paired difference
to the best candidate and to SJF-CP, the children's steps per decision (mean and longest) and the wall time.
With --decima CHECKPOINT (a state dict of `DecimaPolicy`, the reference's models/decima/model.pt as it is) the learned policy's arg-max
decisions are one more candidate, "decima" - it may also be the --base - and one more column: its own episodes (`run_episodes(...,
fused=True)`). Not together with --horizon.
With --topk 2,4 (needs --decima) every listed K gets one more run, "topK": the lookahead over Decima's K best ACTIONS with Decima as the
base policy (`lookahead.ActionLookaheadScheduler`; --samples, --reseed and --replan-every apply), on the same sequences.
The parents are handled `--chunk` at a time: a chunk needs chunk * (1 + candidates * samples) env slots."""
from __future__ import annotations

import argparse
import json
import os.path as osp
import sys
import time

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

from spark_sched_sim_amd import VecSparkSchedSimEnv, evaluation  # noqa: E402
from spark_sched_sim_amd.lookahead import ActionLookaheadScheduler, LookaheadScheduler  # noqa: E402

C1 = dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
TENSOR_KEYS = ("ok", "steps", "avg_num_jobs", "avg_job_duration_s", "episode_avg_job_duration_s", "total_job_time", "pct", "sorted")


def parse_policy(s: str) -> tuple[str, int]:
    return (s.split(":")[0], int(s.split(":")[1]) if ":" in s else 0)


def label(p: tuple[str, int]) -> str:
    return p[0] + (f":{p[1]}" if p[1] else "")


class _Counting:
    """counts the children's steps on the device (no sync): their sum and the longest child over all decisions"""

    def reset(self) -> None:
        super().reset()
        self.child_steps = torch.zeros((), dtype=torch.int64, device=self.env.device)
        self.longest_child = torch.zeros((), dtype=torch.int32, device=self.env.device)

    def decide_and_step(self) -> None:
        super().decide_and_step()
        steps = self.child_out["steps"][self._fork_dst.long()].clamp(min=0)
        self.child_steps += steps.sum()
        self.longest_child = torch.maximum(self.longest_child, steps.max())


class CountingScheduler(_Counting, LookaheadScheduler):
    pass


class CountingActionScheduler(_Counting, ActionLookaheadScheduler):
    pass


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256, help="held-out job sequences")
    ap.add_argument("--seed0", type=int, default=100_000)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--reseed", type=int, default=None, help="Monte-Carlo lookahead: every sample its own task-duration noise")
    ap.add_argument("--replan-every", type=int, default=1)
    ap.add_argument("--base", default=None, help="name[:param]: the rollout algorithm over this base policy (default: policy switching)")
    ap.add_argument("--policies", default="fair,fifo,sjfcp,wfair:1")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=osp.join(ROOT, "profiles", "lookahead.json"))
    ap.add_argument("--horizon", default=None, help="MS[,MS...]: one more lookahead per horizon (simulated time; 'inf' is allowed)")
    ap.add_argument("--tail", default="srpt", choices=("none", "srpt"), help="what a child that stopped at its horizon is charged for the rest")
    ap.add_argument("--no-full", action="store_true", help="with --horizon: leave the full-episode lookahead out")
    ap.add_argument("--tag", default=None, help="key of this run in the output file (default: made of the flags); other keys are kept")
    ap.add_argument("--decima", default=None, metavar="CHECKPOINT", help="a DecimaPolicy state dict: Decima (arg-max) as a candidate and a column of its own")
    ap.add_argument("--topk", default=None, metavar="K[,K...]", help="with --decima: one more run per K, the lookahead over Decima's K best actions (base Decima)")
    args = ap.parse_args()
    topk = [int(k) for k in args.topk.split(",")] if args.topk else []
    if topk and not args.decima:
        ap.error("--topk needs --decima")
    cands = [parse_policy(p) for p in args.policies.split(",")]
    args.policy = None
    if args.decima:
        from spark_sched_sim_amd.decima import DecimaPolicy
        agent = dict(embed_dim=16, gnn_mlp_kwargs=dict(hid_dims=[32, 16], act_cls="LeakyReLU", act_kwargs=dict(negative_slope=0.2)),
                     policy_mlp_kwargs=dict(hid_dims=[64, 64], act_cls="Tanh"))
        args.policy = DecimaPolicy(num_executors=C1["num_executors"], **agent, state_dict_path=args.decima).to(args.device).eval()
        cands = [c for c in cands if c[0] != "decima"] + [("decima", 0)]
    base = parse_policy(args.base) if args.base else None
    N, K, S = args.envs, len(cands), args.samples
    seeds = [args.seed0 + i for i in range(N)]

    solo = VecSparkSchedSimEnv(C1, N, device=args.device)
    results = {label(c): evaluation.run_episodes(solo, args.policy, seeds, greedy=True, fused=True, chunk=4000) if c[0] == "decima"
               else evaluation.run_episodes(solo, c[0], seeds, param=c[1]) for c in cands}
    solo.close()

    horizons = [float(h) for h in args.horizon.split(",")] if args.horizon else []
    chunk = min(args.chunk, N)
    env = VecSparkSchedSimEnv(C1, chunk * (1 + K * S), device=args.device)
    runs = {}
    for horizon in ([] if horizons and args.no_full else [None]) + horizons:
        runs["lookahead" if horizon is None else f"H{horizon:g}"] = run_lookaheads(env, args, cands, base, seeds, chunk, horizon)
    env.close()
    for k in topk:
        env = VecSparkSchedSimEnv(C1, chunk * (1 + k * S), device=args.device)
        runs[f"top{k}"] = run_lookaheads(env, args, cands, base, seeds, chunk, None, topk=k)
        env.close()
    for name, (res, _) in runs.items():
        results[name] = res

    # the best candidate: the one with the lowest mean over the envs where everything finished
    table = evaluation.compare(results, baseline=label(cands[0]), metric="episode_avg_job_duration_s")
    best = min((label(c) for c in cands), key=lambda n: table[n]["avg_job_duration_s"])
    table = evaluation.compare(results, baseline=best, metric="episode_avg_job_duration_s")
    sjfcp = evaluation.compare(results, baseline="sjfcp", metric="episode_avg_job_duration_s") if "sjfcp" in results else None
    run = {"config": "C1", "envs": N, "seed0": args.seed0, "candidates": [label(c) for c in cands], "base": label(base) if base else None, "samples": S,
           "reseed": args.reseed, "replan_every": args.replan_every, "best_candidate": best, "table": table, "tail": args.tail if horizons else None,
           "lookaheads": {name: stats for name, (_, stats) in runs.items()}}
    if sjfcp is not None:
        run["minus_sjfcp_s"] = {name: {"mean": sjfcp[name]["minus_sjfcp_s"], "ci95": sjfcp[name]["minus_sjfcp_ci95"]} for name in runs}
    if "lookahead" in runs:  # (the keys this file had before there were horizons)
        run.update(runs["lookahead"][1])
    tag = args.tag or (f"{'switching' if base is None else 'rollout_' + label(base)}_S{S}_{'exact' if args.reseed is None else 'reseed'}_every{args.replan_every}"
                       + (f"_{args.tail}" if horizons else ""))
    try:
        with open(args.out) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    doc[tag] = run
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(f"[{tag}] {N} sequences, best candidate {best}; mean job duration (s), paired difference to {best} with its 95 % interval:")
    for name in [label(c) for c in cands] + list(runs):
        row = table[name]
        print(f"  {name:10s} {row['avg_job_duration_s']:8.3f} +- {row['ci95']:.3f}   {row['minus_' + best + '_s']:+8.3f} +- {row['minus_' + best + '_ci95']:.3f}"
              + (f"   to sjfcp {sjfcp[name]['minus_sjfcp_s']:+8.3f} +- {sjfcp[name]['minus_sjfcp_ci95']:.3f}" if sjfcp is not None else ""))
    for name, (_, st) in runs.items():
        print(f"  {name:10s} {st['decisions']} decisions in {st['lookahead_wall_s']:.2f} s ({st['decisions_per_s']:.0f} per second), children's steps per decision: "
              f"mean {st['child_steps_mean']:.1f}, longest {st['child_steps_longest']}; {st['fallbacks']} fallbacks")
    print(f"  envs compared {table['envs_compared']}")


def run_lookaheads(env, args, cands, base, seeds, chunk: int, horizon, topk: int | None = None) -> tuple[dict, dict]:
    """the lookahead's episodes on all `seeds`, `chunk` parents at a time -> (the `run_episodes` dict, the run's figures). `topk`: the
    lookahead over Decima's `topk` best actions instead of the one over `cands`"""
    N, K, S = len(seeds), topk or len(cands), args.samples
    parts, decisions, fallbacks, wall, child_steps, longest = [], 0, 0, 0.0, 0, 0
    for at in range(0, N, chunk):
        n = min(chunk, N - at)
        if topk:
            sched = CountingActionScheduler(env, list(range(n)), args.policy, topk, samples=S, reseed=args.reseed, replan_every=args.replan_every,
                                            children=list(range(chunk, chunk + n * K * S)))
        else:
            sched = CountingScheduler(env, list(range(n)), cands, base=base, samples=S, reseed=args.reseed, replan_every=args.replan_every,
                                      children=list(range(chunk, chunk + n * K * S)), horizon=horizon, tail=args.tail, decima=args.policy)
        if env.device.type == "cuda":
            torch.cuda.synchronize(env.device)
        t0 = time.perf_counter()
        r = evaluation.run_lookahead(env, sched, seeds[at: at + n])
        if env.device.type == "cuda":
            torch.cuda.synchronize(env.device)
        wall += time.perf_counter() - t0
        decisions += int(r["decisions"].sum())
        fallbacks += r["fallbacks"]
        child_steps += int(sched.child_steps)
        longest = max(longest, int(sched.longest_child))
        parts.append(r)
    res = {k: torch.cat([p[k] for p in parts]) for k in TENSOR_KEYS}
    res["q"] = parts[0]["q"]
    winners = torch.cat([p["winners"].reshape(-1) for p in parts])
    winners = winners[winners >= 0]
    # (children of a parent that is over take no step: the mean is over the decisions of parents that were still playing)
    stats = {"horizon": horizon, "decisions": decisions, "fallbacks": fallbacks, "lookahead_wall_s": wall, "decisions_per_s": decisions / wall if wall > 0 else None,
             "child_steps_mean": child_steps / max(decisions * K * S, 1), "child_steps_longest": longest,
             "winner_share": {f"slot{k}" if topk else label(c): float((winners == k).double().mean())
                              for k, c in enumerate(range(topk) if topk else cands)} if winners.numel() else {}}
    return res, stats


if __name__ == "__main__":
    main()
