#!/usr/bin/env python3
"""One job sequence under several on-device schedulers, as the Gantt charts the Decima paper and the reference's examples.py show:
per policy a PNG of the executors' timelines (VecSparkSchedSimEnv.render: one band per executor coloured by the job it belongs
to, black = the common pool, red columns = job completions) and a JSON with the average job duration and the executor-time each
job held, taken from the recorded timeline (the reference's `Executor.history`).

    python tools/gantt.py --policies fair,fifo,sjfcp,wfair --seed 3 --out artifacts/gantt
    python tools/gantt.py --emu --config tiny --out /tmp/gantt       # plumbing check on the CPU wave emulator

The same seed gives every policy the same job sequence (arrival times and templates are drawn at reset). "wfair" takes
`--alpha` (default -1). PNGs are written with zlib / struct alone.
"""
import argparse
import json
import os
import os.path as osp
import struct
import sys
import zlib

import numpy as np

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
from spark_sched_sim_amd import VecSparkSchedSimEnv  # noqa: E402

CONFIGS = {
    "tiny": dict(num_executors=5, job_arrival_cap=8, job_arrival_rate=1.0e-4, moving_delay=1500.0, warmup_delay=500.0),
    "c1": dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0),
    "c3": dict(num_executors=50, job_arrival_cap=200, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0),
}


def write_png(path: str, rgb: np.ndarray) -> None:
    """uint8 [H, W, 3] -> an 8-bit RGB PNG (filter 0 on every row)"""
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b""))


def executor_time_per_job(history: list[list[list]], wall_time: float, num_jobs: int) -> list[float]:
    """ms of executor-time each job held: an entry [t, j] lasts from the previous entry's release (0 for the first) to t, the open
    entry to the end of the episode"""
    out = [0.0] * num_jobs
    for h in history:
        start = 0.0
        for t, j in h:
            end = wall_time if t is None else t
            if j >= 0:
                out[j] += end - start
            start = end
    return out


def run_policy(env: VecSparkSchedSimEnv, policy: str, param: int, seed: int, width: int, height: int):
    env.reset(seed=[seed])
    for _ in range(100000):
        env.rollout(policy, 256, param)
        if int(env.obs_i32[0, 6]) or int(env.obs_i32[0, 7]):
            break
    env.raise_on_error()
    hdr = env.header(0)
    ta, tc, _, _ = env.job_times(0)
    done = np.isfinite(tc)
    history = env.timeline(0)
    frame = env.render([0], width=width, height=height)[0].cpu().numpy()
    stats = {"policy": policy, "param": param, "seed": seed, "steps": hdr["ep_steps"], "wall_time_ms": hdr["wall_time"], "num_jobs": hdr["J"],
             "num_completed": int(done.sum()), "avg_job_duration_s": float(np.mean(tc[done] - ta[done]) * 1e-3) if done.any() else None,
             "executor_time_per_job_ms": executor_time_per_job(history, hdr["wall_time"], hdr["J"]),
             "max_entries_per_executor": max(len(h) for h in history)}
    return frame, stats


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--policies", default="fair,fifo,sjfcp,wfair")
    ap.add_argument("--alpha", type=int, default=-1, help="weighted fair's exponent")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--config", default="c1", choices=sorted(CONFIGS))
    ap.add_argument("--out", required=True)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=300)
    ap.add_argument("--cap", type=int, default=1024, help="timeline entries kept per executor")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--emu", action="store_true", help="run on the CPU wave emulator (tests/emu) instead of a GPU")
    args = ap.parse_args()
    lib, device = None, args.device
    if args.emu:
        sys.path.insert(0, osp.join(ROOT, "tests"))
        from emu_util import load_emu
        lib, device = load_emu(), "cpu"
    os.makedirs(args.out, exist_ok=True)
    env = VecSparkSchedSimEnv(CONFIGS[args.config], 1, device=device, _lib=lib)
    env.enable_timeline(args.cap)
    report = []
    for policy in [p for p in args.policies.split(",") if p]:
        frame, stats = run_policy(env, policy, args.alpha if policy == "wfair" else 0, args.seed, args.width, args.height)
        stats["png"] = f"gantt_{args.config}_seed{args.seed}_{policy}.png"
        write_png(osp.join(args.out, stats["png"]), frame)
        report.append(stats)
        print(f"{policy:6s} {stats['steps']:5d} steps  avg job duration {stats['avg_job_duration_s']:.2f} s  -> {stats['png']}", flush=True)
    env.close()
    with open(osp.join(args.out, f"gantt_{args.config}_seed{args.seed}.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
