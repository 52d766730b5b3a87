#!/usr/bin/env python3
"""The lookahead scheduler against its own candidates on held-out job sequences: `--envs` sequences (seeds --seed0 ...), every
candidate's whole episode (`evaluation.run_episodes`) and the lookahead's (`evaluation.run_lookahead`: fork, fused rollouts of the
children, the pick kernel, a step of the parents - four launches per decision), compared pairwise on the same seeds
(`evaluation.compare`). Writes the table to --out (profiles/lookahead.json) and prints it.

    python tools/lookahead_eval.py [--envs 256] [--samples 1] [--reseed N] [--replan-every 1] [--base name[:param]]
                                   [--policies fair,fifo,sjfcp,wfair:1] [--chunk 64]

Without --reseed the children continue the parent's own future (exact lookahead: never above a candidate's own episode); with it
every sample draws its own task durations (Monte-Carlo lookahead: what a scheduler that does not know the future can do).
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
from spark_sched_sim_amd.lookahead import LookaheadScheduler  # noqa: E402

C1 = dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
TENSOR_KEYS = ("ok", "steps", "avg_num_jobs", "avg_job_duration_s", "episode_avg_job_duration_s", "total_job_time", "pct", "sorted")


def parse_policy(s: str) -> tuple[str, int]:
    return (s.split(":")[0], int(s.split(":")[1]) if ":" in s else 0)


def label(p: tuple[str, int]) -> str:
    return p[0] + (f":{p[1]}" if p[1] else "")


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
    ap.add_argument("--tag", default=None, help="key of this run in the output file (default: made of the flags); other keys are kept")
    args = ap.parse_args()
    cands = [parse_policy(p) for p in args.policies.split(",")]
    base = parse_policy(args.base) if args.base else None
    N, K, S = args.envs, len(cands), args.samples
    seeds = [args.seed0 + i for i in range(N)]

    solo = VecSparkSchedSimEnv(C1, N, device=args.device)
    results = {label(c): evaluation.run_episodes(solo, c[0], seeds, param=c[1]) for c in cands}
    solo.close()

    chunk = min(args.chunk, N)
    env = VecSparkSchedSimEnv(C1, chunk * (1 + K * S), device=args.device)
    parts, decisions, fallbacks, wall = [], 0, 0, 0.0
    for at in range(0, N, chunk):
        n = min(chunk, N - at)
        sched = LookaheadScheduler(env, list(range(n)), cands, base=base, samples=S, reseed=args.reseed, replan_every=args.replan_every,
                                   children=list(range(chunk, chunk + n * K * S)))
        if env.device.type == "cuda":
            torch.cuda.synchronize(env.device)
        t0 = time.perf_counter()
        r = evaluation.run_lookahead(env, sched, seeds[at: at + n])
        if env.device.type == "cuda":
            torch.cuda.synchronize(env.device)
        wall += time.perf_counter() - t0
        decisions += int(r["decisions"].sum())
        fallbacks += r["fallbacks"]
        parts.append(r)
    env.close()
    results["lookahead"] = {k: torch.cat([p[k] for p in parts]) for k in TENSOR_KEYS}
    results["lookahead"]["q"] = parts[0]["q"]

    # the best candidate: the one with the lowest mean over the envs where everything finished
    table = evaluation.compare(results, baseline=label(cands[0]), metric="episode_avg_job_duration_s")
    best = min((label(c) for c in cands), key=lambda n: table[n]["avg_job_duration_s"])
    table = evaluation.compare(results, baseline=best, metric="episode_avg_job_duration_s")
    winners = torch.cat([p["winners"].reshape(-1) for p in parts])
    winners = winners[winners >= 0]
    run = {"config": "C1", "envs": N, "seed0": args.seed0, "candidates": [label(c) for c in cands], "base": label(base) if base else None, "samples": S,
           "reseed": args.reseed, "replan_every": args.replan_every, "best_candidate": best, "table": table, "decisions": decisions, "fallbacks": fallbacks,
           "lookahead_wall_s": wall, "decisions_per_s": decisions / wall if wall > 0 else None,
           "winner_share": {label(c): float((winners == k).double().mean()) for k, c in enumerate(cands)} if winners.numel() else {}}
    tag = args.tag or f"{'switching' if base is None else 'rollout_' + label(base)}_S{S}_{'exact' if args.reseed is None else 'reseed'}_every{args.replan_every}"
    try:
        with open(args.out) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    doc[tag] = run
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(f"[{tag}] {N} sequences, best candidate {best}; mean job duration (s), paired difference to {best} with its 95 % interval:")
    for name in [label(c) for c in cands] + ["lookahead"]:
        row = table[name]
        print(f"  {name:10s} {row['avg_job_duration_s']:8.3f} +- {row['ci95']:.3f}   {row['minus_' + best + '_s']:+8.3f} +- {row['minus_' + best + '_ci95']:.3f}")
    print(f"  {decisions} decisions in {wall:.2f} s ({run['decisions_per_s']:.0f} per second), {fallbacks} fallbacks, envs compared {table['envs_compared']}")


if __name__ == "__main__":
    main()
