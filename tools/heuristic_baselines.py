#!/usr/bin/env python3
"""The Decima paper's heuristic baselines (Mao et al., SIGCOMM 2019, 7.2) on the batched env: fair, FIFO, weighted fair over an
alpha grid, and SJF-CP, all as on-device policies (VecSparkSchedSimEnv.policy_actions / rollout; definitions in DESIGN.md 9).

1. quality: whole episodes (no time limit) of `--envs` HELD-OUT seeds at the README's sizing (10 executors, 50 jobs) and at
   config 3 (50 executors, 200 jobs); the same seeds, hence the same job sequences, for every policy. Per env the mean job
   duration (metrics.avg_job_duration: over the last <= 200 completed jobs); per policy its mean and 95 % confidence interval
   over envs and the paired difference to fair (tools/decima_vs_fair.py compare). `--decima-ckpt PATH`: a DecimaPolicy
   state_dict (the architecture of config/decima_tpch.yaml) evaluated on the same seeds, sampled and arg-max;
2. speed: fused-rollout env-steps/s per policy at `--speed-envs` envs (device events around synchronised launches).

    python tools/heuristic_baselines.py --out profiles/heuristics.json
    python tools/heuristic_baselines.py --emu --envs 4 --speed-envs 4   # plumbing check on the CPU wave emulator
"""
import argparse
import json
import os.path as osp
import sys
import time

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, "tools"))
from spark_sched_sim_amd import VecSparkSchedSimEnv, workload  # noqa: E402
from spark_sched_sim_amd.evaluation import compare, run_episodes  # noqa: E402
from decima_vs_fair import AGENT, episodes_under_decima  # noqa: E402

CONFIGS = {
    "c1": dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0),
    "c3": dict(num_executors=50, job_arrival_cap=200, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0),
}


def policies(alphas) -> list[tuple[str, str, int]]:
    """(label, on-device policy, param)"""
    out = [("fair", "fair", 0), ("fifo", "fifo", 0)]
    out += [(f"wfair_{a:+d}", "wfair", a) for a in alphas]
    out.append(("sjfcp", "sjfcp", 0))
    return out


def episodes(env, policy: str, param: int, seed0: int, launch_steps: int = 200) -> dict:
    return run_episodes(env, policy, seed0, max_steps=5000 * launch_steps, param=param, chunk=launch_steps)


def steps_per_second(env, policy: str, param: int, seed0: int, launch_steps: int, launches: int, timed: bool) -> float:
    """env-steps/s of the fused rollout: auto-reset keeps every env busy; one warm-up launch, then `launches` timed ones"""
    env.reset(seed=seed0)
    env.rollout(policy, launch_steps, param)
    if not timed:
        return float("nan")
    torch.cuda.synchronize()
    s0 = env.header_field("n_steps").clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        env.rollout(policy, launch_steps, param)
    e1.record()
    torch.cuda.synchronize()
    steps = int((env.header_field("n_steps") - s0).sum())
    return steps / (e0.elapsed_time(e1) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096, help="held-out episodes per policy and config")
    ap.add_argument("--configs", default="c1,c3")
    ap.add_argument("--alphas", default="-4,-3,-2,-1,0,1,2,3,4")
    ap.add_argument("--eval-seed", type=int, default=10_000_000)
    ap.add_argument("--decima-ckpt", default=None, help="DecimaPolicy state_dict (.pt) to evaluate on the same seeds (config c1 only)")
    ap.add_argument("--speed-envs", type=int, default=4096)
    ap.add_argument("--speed-steps", type=int, default=100, help="steps per fused launch in the speed runs")
    ap.add_argument("--speed-launches", type=int, default=5)
    ap.add_argument("--pack", default="default", choices=list(workload.PROFILES))
    ap.add_argument("--out", default="heuristics.json")
    ap.add_argument("--emu", action="store_true", help="plumbing check without a GPU: the CPU wave-emulator build of the kernels (tests/emu)")
    a = ap.parse_args()
    dev, lib = "cuda:0", None
    if a.emu:
        sys.path.insert(0, osp.join(ROOT, "tests"))
        from emu_util import load_emu
        dev, lib = "cpu", load_emu()
    alphas = [int(x) for x in a.alphas.split(",") if x != ""]
    pack = workload.profile_pack(a.pack)
    rec = {"what": "heuristic baselines of the Decima paper (7.2) as on-device policies: mean job duration over held-out job sequences, "
                   "paired against fair; fused-rollout env-steps/s",
           "pack": a.pack, "envs": a.envs, "eval_seed": a.eval_seed, "configs": {}, "speed": {}}
    if dev != "cpu":
        rec["device"] = torch.cuda.get_device_name(0)
    for cname in a.configs.split(","):
        cfg = CONFIGS[cname]
        # a fresh env per policy: the job-duration deque behind avg_job_duration outlives reset() (as the reference's
        # job_duration_buff does), so a reused env would average in the previous policy's jobs
        fresh = lambda: VecSparkSchedSimEnv(cfg, a.envs, device=dev, pack=pack, _lib=lib)  # noqa: E731
        res, t0 = {}, time.perf_counter()
        for label, pol, param in policies(alphas):
            env = fresh()
            res[label] = episodes(env, pol, param, a.eval_seed)
            env.close()
        if a.decima_ckpt and cname == "c1":
            from spark_sched_sim_amd.decima import DecimaPolicy
            kw = {k: v for k, v in AGENT.items() if k != "agent_cls"}
            policy = DecimaPolicy(num_executors=cfg["num_executors"], **kw).to(dev)
            policy.load_state_dict(torch.load(a.decima_ckpt, map_location=dev))
            policy.eval()
            gen = torch.Generator(device=dev).manual_seed(7)
            for tag, greedy in (("decima_sampled", False), ("decima_greedy", True)):
                env = fresh()
                res[tag] = episodes_under_decima(env, policy, a.eval_seed, greedy, gen)
                env.close()
        c = compare(res)
        wf = [k for k in c if k.startswith("wfair_")]
        if wf:
            best = min(wf, key=lambda k: c[k]["avg_job_duration_s"])
            c["best_wfair"] = {"label": best, "alpha": int(best.split("_")[1]), "avg_job_duration_s": c[best]["avg_job_duration_s"]}
        c["env"], c["eval_seconds"] = cfg, round(time.perf_counter() - t0, 1)
        rec["configs"][cname] = c
        print(json.dumps({cname: {k: (v["avg_job_duration_s"] if isinstance(v, dict) and "avg_job_duration_s" in v else v)
                                  for k, v in c.items() if k != "env"}}), flush=True)
    for cname in a.configs.split(","):
        env = VecSparkSchedSimEnv(CONFIGS[cname], a.speed_envs, device=dev, pack=pack, _lib=lib, auto_reset=True, seed_stride=a.speed_envs)
        sp = {}
        for label, pol, param in policies(alphas):
            sp[label] = steps_per_second(env, pol, param, a.eval_seed, a.speed_steps, a.speed_launches, timed=dev != "cpu")
        rec["speed"][cname] = {"envs": a.speed_envs, "steps_per_launch": a.speed_steps, "launches": a.speed_launches, "env_steps_per_s": sp}
        print(json.dumps({f"speed_{cname}": {k: round(v) if v == v else None for k, v in sp.items()}}), flush=True)
        env.close()
    with open(a.out, "w") as fp:
        json.dump(rec, fp, indent=1)


if __name__ == "__main__":
    main()
