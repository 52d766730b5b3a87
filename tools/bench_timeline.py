#!/usr/bin/env python3
"""What recording the executor timelines costs, and how fast the Gantt rasteriser writes (profiles/timeline.md):

1. step time at the benchmark's headline sizing (bench.py defaults: 4096 envs, 10 executors, 50 jobs, hash policy, auto-reset) with
   the recording off and on, in both modes - "step" (policy kernel + step kernel per step) and "fused" (rollout launches of 50
   steps) - `--repeats` times each, alternating, from the same pre-rolled steady state; `--config e100` measures the wide
   instantiation of the kernels instead (100 executors, 200 jobs, fair policy);
2. the rasteriser (sss_timeline_render) for `--render-envs` envs at `--width` x `--height`: HIP-event time per launch and the
   achieved bytes per second against the frame bytes it writes.

    python tools/bench_timeline.py --out profiles/timeline_bench.json
    python tools/bench_timeline.py --config e100 --envs 1024 --steps 400 --warmup 50 --preroll 3000 --no-render
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/bench_timeline.py --render-only   # the rasteriser's kernel stats
"""
import argparse
import json
import os.path as osp
import statistics
import sys

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
from spark_sched_sim_amd import VecSparkSchedSimEnv  # noqa: E402

# bench.py's sizings: the headline, and 100 executors (the wide instantiation of the kernels)
CONFIGS = {"c2": dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0),
           "e100": dict(num_executors=100, job_arrival_cap=200, job_arrival_rate=8.0e-5, moving_delay=2000.0, warmup_delay=1000.0)}
POLICY = {"c2": ("hash", 30), "e100": ("fair", 0)}   # (on-device policy, its parameter: the hash policy's permille of "no stage")


def make_env(config: str, envs: int, cap: int | None, preroll: int) -> VecSparkSchedSimEnv:
    env = VecSparkSchedSimEnv(CONFIGS[config], envs, device="cuda:0", auto_reset=True)
    env.bench_policy = POLICY[config]
    if cap:
        env.enable_timeline(cap)
    env.reset(seed=0)
    for _ in range(preroll // 50):
        env.rollout(env.bench_policy[0], 50, env.bench_policy[1])
    torch.cuda.synchronize()
    return env


def time_steps(env: VecSparkSchedSimEnv, mode: str, steps: int, warmup: int) -> float:
    """ms per batched step"""
    def run(n):
        if mode == "fused":
            for _ in range(n // 50):
                env.rollout(env.bench_policy[0], 50, env.bench_policy[1])
        else:
            for _ in range(n):
                env.step_async(**env.policy_actions(*env.bench_policy))
    run(warmup)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    run(steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def time_render(env: VecSparkSchedSimEnv, width: int, height: int, reps: int) -> dict:
    frames = env.render(width=width, height=height)   # warm-up (and the allocation)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frames = env.render(width=width, height=height)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    nbytes = frames.numel()
    best, med = min(times), statistics.median(times)
    return {"envs": env.num_envs, "width": width, "height": height, "frame_bytes": nbytes, "ms_best": best, "ms_median": med,
            "gb_per_s_best": nbytes / best / 1e6, "gb_per_s_median": nbytes / med / 1e6,
            "note": "times include the output tensor's allocation by the caching allocator; the kernel alone: rocprofv3 --kernel-trace --stats"}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c2", choices=list(CONFIGS))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--preroll", type=int, default=1500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--render-envs", type=int, default=4096)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--height", type=int, default=300)
    ap.add_argument("--render-reps", type=int, default=20)
    ap.add_argument("--render-only", action="store_true")
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    report: dict = {"device": torch.cuda.get_device_name(0), "config": CONFIGS[args.config], "envs": args.envs, "steps": args.steps, "cap": args.cap}
    if not args.render_only:
        for mode in ("step", "fused"):
            rows = {"off": [], "on": []}
            for _ in range(args.repeats):
                for which, cap in (("off", None), ("on", args.cap)):
                    env = make_env(args.config, args.envs, cap, args.preroll)
                    rows[which].append(time_steps(env, mode, args.steps, args.warmup))
                    if cap:
                        report.setdefault("max_entries_per_executor", []).append(int(env.timeline_arrays()[2].max()))
                    env.close()
            report[mode] = {k: {"ms_per_step": v, "median": statistics.median(v)} for k, v in rows.items()}
            report[mode]["on_over_off"] = report[mode]["on"]["median"] / report[mode]["off"]["median"]
            print(mode, json.dumps(report[mode]), flush=True)
    if not args.no_render:
        env = make_env(args.config, args.render_envs, args.cap, args.preroll)
        report["render"] = time_render(env, args.width, args.height, args.render_reps)
        env.close()
        print("render", json.dumps(report["render"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
