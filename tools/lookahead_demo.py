#!/usr/bin/env python3
"""Lookahead from one state: an env plays `--at` steps of one job sequence under the fair scheduler; from THAT state every candidate
scheduler gets `--samples` forked children (`evaluation.continuations`: same job sequence, each child its own task-duration noise)
which play to the end of the episode on the device. Prints each scheduler's cost-to-go - the episode's mean job duration and the
time-average number of jobs in the system - with a 95 % confidence interval over the samples.

    python tools/lookahead_demo.py [--seed 0] [--at 150] [--samples 64] [--policies fair,fifo,sjfcp,wfair:1] [--horizon MS] [--tail srpt|none]
                                    [--decima CHECKPOINT --topk K]

With --horizon the children stop that span of simulated time after the fork (`continuations(fused=True, horizon=...)`); the figures
describe the states they stopped in, and the cost the horizon lookahead would compare (`evaluation.horizon_cost`) is printed beside them.
With --decima CHECKPOINT --topk K the Q-values of Decima's K best ACTIONS in that state are printed as well: slot r's children take
the r-th best decision of the arg-max policy (`DecimaPolicy.topk_env`) and then follow Decima to the end of the episode
(`DecimaPolicy.rollout_action_env`), each sample with its own task-duration noise - total job time, mean over the samples.
"""
from __future__ import annotations

import argparse
import os.path as osp
import sys

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

from spark_sched_sim_amd import VecSparkSchedSimEnv, evaluation  # noqa: E402

C1 = dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--at", type=int, default=150, help="steps the parent plays before the fork")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--policies", default="fair,fifo,sjfcp,wfair:1", help="on-device policies, name[:param]")
    ap.add_argument("--horizon", type=float, default=None, help="the children stop this span of simulated time after the fork")
    ap.add_argument("--tail", default="srpt", choices=("none", "srpt"))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--decima", default=None, metavar="CHECKPOINT", help="a DecimaPolicy state dict (for --topk)")
    ap.add_argument("--topk", type=int, default=0, help="with --decima: print the Q-values of Decima's K best actions from the state")
    args = ap.parse_args()
    if args.topk and not args.decima:
        ap.error("--topk needs --decima")
    policies = [(p.split(":")[0], int(p.split(":")[1]) if ":" in p else 0) for p in args.policies.split(",")]
    S = args.samples
    env = VecSparkSchedSimEnv(C1, 1 + S, device=args.device)
    env.reset(seed=[args.seed] * (1 + S))
    skip = torch.full((1 + S,), -2147483648, dtype=torch.int32, device=env.device)
    for _ in range(args.at):  # the parent alone
        a = env.policy_actions("fair")
        skip[0] = a["stage_idx"][0]
        env.step_async(skip, a["num_exec"])
    h = env.header(0)
    print(f"state: seed {args.seed} after {args.at} steps of 'fair': wall_time {h['wall_time']:.0f} ms, {h['n_active']} jobs active, {h['n_completed']} of {h['J']} completed")
    children = list(range(1, 1 + S))
    for name, param in policies:
        if args.horizon is not None:
            r = evaluation.continuations(env, [0] * S, children, name, param=param, reseed=[1000 + k for k in range(S)], fused=True, horizon=args.horizon, tail=args.tail)
            cost = r["horizon_cost"]
            cost = cost[~torch.isnan(cost)]
            print(f"{name + (':' + str(param) if param else ''):10s} horizon {args.horizon:g} / {args.tail}: cost {float(cost.mean()):14.1f} over {cost.numel()} of {S} children, "
                  f"{int(r['ok'].sum())} ended their episode, {float(r['steps'].double().mean()) - args.at:.0f} steps each")
            continue
        r = evaluation.continuations(env, [0] * S, children, name, param=param, reseed=[1000 + k for k in range(S)])
        ok = r["ok"]
        n = int(ok.sum())
        dur, jobs = r["episode_avg_job_duration_s"][ok], r["avg_num_jobs"][ok]
        ci = lambda v: float(1.96 * v.std() / max(n, 1) ** 0.5) if n > 1 else float("nan")  # noqa: E731
        print(f"{name + (':' + str(param) if param else ''):10s} mean job duration {float(dur.mean()):8.2f} +- {ci(dur):.2f} s   avg jobs in system {float(jobs.mean()):6.2f} +- {ci(jobs):.2f}   "
              f"({n} of {S} children finished)")
    if args.topk:
        action_values(env, args, children)
    env.close()


def action_values(env, args, children) -> None:
    """Q(state, a) for Decima's --topk best actions a, by Monte Carlo: `--samples // K` children per action, Decima (arg-max) behind it"""
    from spark_sched_sim_amd.binding import POLICY_DECIMA
    from spark_sched_sim_amd.decima import DecimaPolicy
    agent = dict(embed_dim=16, gnn_mlp_kwargs=dict(hid_dims=[32, 16], act_cls="LeakyReLU", act_kwargs=dict(negative_slope=0.2)),
                 policy_mlp_kwargs=dict(hid_dims=[64, 64], act_cls="Tanh"))
    policy = DecimaPolicy(num_executors=C1["num_executors"], **agent, state_dict_path=args.decima).to(env.device).eval()
    B, K = env.num_envs, args.topk
    per = max(1, len(children) // K)
    kids = torch.tensor(children[: per * K], dtype=torch.long, device=env.device).reshape(K, per)
    env.fork([0] * (per * K), children[: per * K], reseed=[1000 + k % per for k in range(per * K)])  # (sample s of every action draws the same noise)
    active = torch.zeros(B, dtype=torch.bool, device=env.device)
    active[0] = True
    top = policy.topk_env(env, K, active=active)
    pol = torch.full((B,), -1, dtype=torch.int32, device=env.device)
    stage, nexec = torch.full_like(pol, -1), torch.full_like(pol, -1)
    pol[kids.reshape(-1)] = POLICY_DECIMA
    stage[kids.reshape(-1)] = top["stage_idx"][0][:, None].expand(K, per).reshape(-1)
    nexec[kids.reshape(-1)] = top["num_exec"][0][:, None].expand(K, per).reshape(-1)
    policy.rollout_action_env(env, 200_000, stage, nexec, greedy=True, policy=pol, param=torch.zeros_like(pol))
    cost = env.job_stats()["stats"][:, 1]
    ok = (env.header_field("terminated") != 0) & (env.obs_i32[:, 7] == 0)
    print(f"Decima's {int(top['count'][0])} best actions of {K} asked for (total job time to the episode's end, {per} samples each, Decima behind the action):")
    for r in range(int(top["count"][0])):
        c = cost[kids[r]][ok[kids[r]]]
        ci = float(1.96 * c.std() / c.numel() ** 0.5) if c.numel() > 1 else float("nan")
        print(f"  slot {r}: stage_idx {int(top['stage_idx'][0, r]):3d} num_exec {int(top['num_exec'][0, r]):3d} log-prob {float(top['lgprob'][0, r]):8.3f}   "
              f"Q = {float(c.mean()) if c.numel() else float('nan'):14.1f} +- {ci:.1f}   ({c.numel()} of {per} children finished)")


if __name__ == "__main__":
    main()
