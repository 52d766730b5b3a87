#!/usr/bin/env python3
"""The differential-returns step alone on a synthetic [T, B] record of one GPU's share of BASELINE config 5 (no collection):
`training.DeviceDifferentialReturns` (the kernels of csrc/sss_returns.h) against `training.DifferentialReturns` (the host form) on
the same record, alternating, every call between two device synchronises; then the ordered sum alone (an empty record: the
window is only summed). Checks that the two forms agree bit for bit while it is at it. Prints one JSON line.
`--device-only`: the kernels alone (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os.path as osp
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from spark_sched_sim_amd.training import DeviceDifferentialReturns, DifferentialReturns, Rollouts  # noqa: E402


def record(gen, T, B, dev):
    n = torch.randint(T // 2, T + 1, (B,), generator=gen)
    dt = torch.rand((T, B), generator=gen, dtype=torch.float64) * 5e4
    dt[torch.rand((T, B), generator=gen) < 0.25] = 0.0  # (a quarter of the reference's steps take no time: tests/golden/ppo_c1.npz)
    ta = torch.cumsum(dt, 0)
    tb = torch.cat([torch.zeros((1, B), dtype=torch.float64), ta[:-1]])
    rw = -torch.rand((T, B), generator=gen, dtype=torch.float64) * 1e4
    a = torch.arange(T)[:, None] < n[None, :]
    z = torch.zeros((1, 1), dtype=torch.long)
    return Rollouts(graph={}, active=a.to(dev), t_before=(tb * a).to(dev), t_after=(ta * a).to(dev), rewards=(rw * a).to(dev), stage_sel=z, job_idx=z, exec_sel=z,
                    lgprobs=z.float(), resets=z.bool())


def timed(fn, *args):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def spread(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7441, help="T: the longest rollout (BASELINE config 5: 7 441)")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--cap", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3)
    ros = [record(gen, a.steps, a.envs, dev) for _ in range(2)]
    devc, host = DeviceDifferentialReturns(a.cap), DifferentialReturns(a.cap)
    t_dev, t_host, equal = [], [], True
    for i in range(a.warmup + a.repeats):
        ro = ros[i % 2]
        td, out_d = timed(devc, ro)
        if not a.device_only:
            th, out_h = timed(host, ro)
            equal = equal and bool(torch.equal(out_d.view(torch.int64), out_h.view(torch.int64))) and \
                np.float64(devc.avg_num_jobs).view(np.uint64) == np.float64(host.avg_num_jobs).view(np.uint64)
            if i >= a.warmup:
                t_host.append(th)
        if i >= a.warmup:
            t_dev.append(td)
    empty = Rollouts(**{**ros[0].__dict__, **{k: getattr(ros[0], k)[:0] for k in ("active", "t_before", "t_after", "rewards")}})
    t_sum = [timed(devc, empty)[0] for _ in range(a.warmup + 10 * a.repeats)][a.warmup:]  # (the sum kernel and a one-block returns launch that writes avg)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(100):
        devc(empty)
    ev[1].record()
    torch.cuda.synchronize()
    out = {"T": a.steps, "B": a.envs, "cap": a.cap, "samples": int(ros[0].active.sum()), "device": spread(t_dev), "host": spread(t_host) if t_host else None,
           "bit_identical": bool(equal) if t_host else None, "sum_only_call": spread(t_sum), "sum_only_device_events_ms_per_call": ev[0].elapsed_time(ev[1]) / 100,
           "avg_num_jobs": devc.avg_num_jobs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
