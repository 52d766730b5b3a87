#!/usr/bin/env python3
"""Times `VecSparkSchedSimEnv.fork` of B/2 envs into the other B/2, mid-episode, at the C2 and C3 sizings (bench.py CONFIGS), against
the copy a user could write without it: whole arena blocks and whole observation rows by tensor indexing,
    env._env_view[dst] = env._env_view[src]    (+ nodes, edge_links, dag_ptr, exec_supplies, obs_i32, obs_f64 the same way)
which moves the pool overflow area too (and leaves the header's bookkeeping wrong - it is a yardstick for the bytes, not a fork).

    python tools/bench_fork.py [--envs 4096] [--repeats 50] [--json out.json]

Method: the envs play `--preroll` steps of the fair policy from distinct seeds first, so pools have grown and observations are
full-size; both forms are warmed up, then timed `--repeats` times each, ALTERNATING, every call between two device events on the
same stream; the median and the min..max spread are reported (`fork`: the API call with the tensor ops that copy the host-side
mirrors; `copy_launch`: the sss_env_copy launch alone). The bytes of the selective copy are counted from the state itself
(dense part + tables of pools with mask != 7 + live observation prefixes), read + write; TB/s = bytes / median time, next to the
MI355X's measured copy ceiling of about 6.3 TB/s. At C2 the working set of a repeat (2 x 2048 images) fits the 256 MB last-level
cache; at C3 the whole-block copy does not."""
from __future__ import annotations

import argparse
import json
import os.path as osp
import statistics
import sys

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

from spark_sched_sim_amd import VecSparkSchedSimEnv  # noqa: E402

CONFIGS = {
    "c2": dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0),
    "c3": dict(num_executors=50, job_arrival_cap=200, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0),
}
COPY_CEILING_TBS = 6.3


def image_bytes(env, ids: torch.Tensor) -> tuple[float, dict]:
    """bytes one fork of the envs `ids` reads (= writes), counted from their state: csrc/sss_fork.h's image"""
    d = env.dims
    J, SP, E = d.job_cap, d.stage_stride, env.num_executors
    al = lambda x: (x + 63) // 64 * 64  # noqa: E731
    off_pool_hdr = al(al(d.off_t_completed + 8 * J + 8 * J * SP) + 4 * J * SP)
    n_pools = 1 + J + J * SP
    off_pool_tab = al(off_pool_hdr + 16 * n_pools)
    table = 1024 if E >= 128 else (512 if E >= 64 else 256)
    assert off_pool_tab + table * n_pools == d.off_dur_ring
    dense = off_pool_tab + (d.env_stride - d.off_dur_ring)
    rows = env._env_view[ids.long()]
    masks = rows[:, off_pool_hdr: off_pool_hdr + 16 * n_pools].reshape(len(ids), n_pools, 16)[:, :, :2].contiguous().view(torch.int16)
    grown = (masks.reshape(len(ids), n_pools) != 7).sum(1).double()
    o = env.obs_i32[ids.long()].double()
    obs = o[:, 0] * 12 + o[:, 1] * 8 + (o[:, 2] + 1) * 4 + o[:, 2] * 4 + 32 + 16
    per_env = dense + grown * table + obs
    return float(per_env.sum()), {"dense_bytes": dense, "grown_tables_mean": float(grown.mean()), "table_bytes": table, "obs_prefix_bytes_mean": float(obs.mean()),
                                  "image_bytes_mean": float(per_env.mean())}


def whole_copy(env, src: torch.Tensor, dst: torch.Tensor) -> None:
    env._env_view[dst] = env._env_view[src]
    for t in (env.nodes, env.edge_links, env.dag_ptr, env.exec_supplies, env.obs_i32, env.obs_f64):
        t[dst] = t[src]


def timed(fn, stream) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def bench(config: str, B: int, repeats: int, preroll: int, dev: str) -> dict:
    env = VecSparkSchedSimEnv(CONFIGS[config], B, device=dev, auto_reset=True)
    env.reset(seed=12345)
    env.rollout("fair", preroll)
    half = B // 2
    src = torch.arange(half, dtype=torch.int32, device=dev)
    dst = src + half
    src_l, dst_l = src.long(), dst.long()
    moved, parts = image_bytes(env, src)
    d = env.dims
    whole = half * (d.env_stride + 12 * d.node_cap + 8 * d.edge_cap + 4 * (d.job_cap + 1) + 4 * d.job_cap + 32 + 16)
    stream = torch.cuda.current_stream(env.device)
    for _ in range(5):
        env.fork(src, dst)
        whole_copy(env, src_l, dst_l)
    torch.cuda.synchronize(env.device)
    t_fork, t_whole, t_launch = [], [], []
    for _ in range(repeats):
        t_fork.append(timed(lambda: env.fork(src, dst), stream))
        t_launch.append(timed(lambda: env._env_copy(None, None, src, dst, None), stream))  # the copy launch alone, without the host mirrors' tensor ops
        t_whole.append(timed(lambda: whole_copy(env, src_l, dst_l), stream))
    env.fork(src, dst)  # (the yardstick leaves the destinations' headers inconsistent: end on a real fork)
    torch.cuda.synchronize(env.device)
    err = int((env.obs_i32[:, 7] != 0).sum())
    env.close()
    mf, mw, ml = statistics.median(t_fork), statistics.median(t_whole), statistics.median(t_launch)
    return {"config": config, "envs": B, "pairs": half, "preroll_steps": preroll, "repeats": repeats, **parts,
            "block_bytes": int(d.env_stride), "whole_copy_bytes_per_env": whole // half,
            "fork_s": {"median": mf, "min": min(t_fork), "max": max(t_fork)}, "whole_copy_s": {"median": mw, "min": min(t_whole), "max": max(t_whole)},
            "copy_launch_s": {"median": ml, "min": min(t_launch), "max": max(t_launch)}, "copy_launch_read_plus_write_TBs": 2 * moved / ml * 1e-12,
            "fork_read_plus_write_TBs": 2 * moved / mf * 1e-12, "whole_copy_read_plus_write_TBs": 2 * whole / mw * 1e-12, "copy_ceiling_TBs": COPY_CEILING_TBS,
            "bytes_ratio_whole_over_fork": whole / moved, "time_ratio_whole_over_fork": mw / mf, "envs_with_error": err}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fork.py measures on the GPU: no device found")
    out = [bench(c, args.envs, args.repeats, args.preroll, "cuda:0") for c in args.configs.split(",")]
    for r in out:
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
