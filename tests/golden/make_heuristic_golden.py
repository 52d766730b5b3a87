#!/usr/bin/env python3
"""Regenerates the weighted-fair and SJF-CP fixtures (tests/golden/{c1,c3,e100,deep_c1,tiny}_{wfair,sjfcp}*.npz) by driving the
REFERENCE env (imported, unmodified, as make_golden.py does) with this repo's host plugins WeightedFairScheduler /
SJFCPScheduler (spark_sched_sim_amd/schedulers.py). The plugins only read the reference's observation dict, so the recorded
action streams pin the definitions; the on-device policies ("wfair" / "sjfcp") are tested against them.

Runs only in the build container (where the reference is importable); the GPU box sees the .npz outputs alone.

    python tests/golden/make_heuristic_golden.py                # every set below
    python tests/golden/make_heuristic_golden.py c1_sjfcp       # one set
    python tests/golden/make_heuristic_golden.py --out DIR c1_sjfcp   # written to DIR instead (regeneration checks)

The file layout is make_golden.py's (make_golden.run_episode records every episode), plus `param` (the policy's integer
parameter: alpha for "wfair", 0 for "sjfcp"); `policy` names the on-device policy.
"""
from __future__ import annotations

import os
import os.path as osp
import sys
import tempfile

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (puts the repository, the gymnasium stand-in and the reference on sys.path)
from make_golden import C1, C3, DEEP, E100, TINY  # noqa: E402

from spark_sched_sim_amd import workload  # noqa: E402
from spark_sched_sim_amd.schedulers import SJFCPScheduler, WeightedFairScheduler  # noqa: E402

# name -> (env_cfg, policy, param, seeds, reset options[, (query sizes, number of queries, generator seed[, profile])]);
# seeds are chosen to keep every file well under 1 MB
SETS = {
    "c1_wfair_m1": (C1, "wfair", -1, [0, 1, 2, 3], None),
    "c1_wfair_p1": (C1, "wfair", 1, [4, 5, 6], None),
    "c1_sjfcp": (C1, "sjfcp", 0, [0, 1, 2, 3], None),
    "c3_wfair_m1": (C3, "wfair", -1, [0], None),
    "c3_sjfcp": (C3, "sjfcp", 0, [1], None),
    "e100_wfair_m1": (E100, "wfair", -1, [0, 1], None),
    "e100_sjfcp": (E100, "sjfcp", 0, [2, 3], None),
    "deep_c1_sjfcp": (C1, "sjfcp", 0, [0], None, DEEP),
    # bounded by a time limit instead of a job cap, alpha = 2
    "tiny_wfair_p2_tlimit": (dict(TINY, job_arrival_cap=None), "wfair", 2, list(range(6)), {"time_limit": 400000.0}),
}


def plugin_factory(policy: str, param: int):
    """make_golden.run_episode builds its scheduler as sched_cls(num_executors, dynamic_partition=True) for policy "fair";
    this stands in for that class"""
    def make(num_executors, dynamic_partition=True):
        if policy == "wfair":
            return WeightedFairScheduler(num_executors, alpha=param)
        return SJFCPScheduler(num_executors)
    return make


def main(argv):
    out_dir = HERE
    if argv and argv[0] == "--out":
        out_dir, argv = argv[1], argv[2:]
    names = argv or list(SETS)
    cwd0 = os.getcwd()
    gym = metrics = None
    for name in names:
        env_cfg, policy, param, seeds, options = SETS[name][:5]
        shape = SETS[name][5] if len(SETS[name]) > 5 else None
        sizes, n_queries, raw_seed = shape[:3] if shape else (list(workload.QUERY_SIZES), workload.NUM_QUERIES, workload.DEFAULT_SEED)
        profile = shape[3] if shape and len(shape) > 3 else "default"
        raw = workload.make_raw_workload(raw_seed, sizes, n_queries, profile=profile)
        pack = workload.build_pack(raw)
        with tempfile.TemporaryDirectory() as tmp:
            workload.write_reference_layout(raw, tmp)
            os.chdir(tmp)  # the reference reads data/tpch relative to cwd (tpch.py:48,119)
            if gym is None:
                gym, _, metrics = make_golden.import_reference()
            from spark_sched_sim.data_samplers import tpch
            keep = (tpch.QUERY_SIZES, tpch.NUM_QUERIES)
            tpch.QUERY_SIZES, tpch.NUM_QUERIES = list(sizes), n_queries
            try:
                blob = {}
                for seed in seeds:
                    ep = make_golden.run_episode(gym, metrics, env_cfg, "fair", seed, options, plugin_factory(policy, param), sizes)
                    for k, v in ep.items():
                        blob[f"s{seed}_{k}"] = v
                    print(f"{name} seed={seed}: {len(ep['stage_idx']) - 1} steps, "
                          f"{int(ep['num_completed'])}/{int(ep['num_jobs'])} jobs"
                          + (f"  ERROR at step {int(ep['error_step'])}: {ep['error_msg']}" if ep["error_step"] >= 0 else ""),
                          flush=True)
            finally:
                tpch.QUERY_SIZES, tpch.NUM_QUERIES = keep
                os.chdir(cwd0)
        blob["seeds"] = np.asarray(seeds, dtype=np.int64)
        blob["policy"] = np.asarray(policy)
        blob["param"] = np.int64(param)
        blob["pack_sha256"] = np.asarray(workload.pack_digest(pack))
        if shape:  # what tests/golden_util.py needs to rebuild the set's pack
            blob["trace_sizes"], blob["trace_queries"], blob["trace_seed"] = np.asarray(sizes), np.int64(n_queries), np.int64(raw_seed)
            if profile != "default":
                blob["trace_profile"] = np.asarray(profile)
        blob["cfg_keys"] = np.asarray(sorted(k for k in env_cfg if k != "data_sampler_cls"))
        blob["cfg_vals"] = np.asarray(
            [np.nan if env_cfg[k] is None else float(env_cfg[k]) for k in sorted(env_cfg) if k != "data_sampler_cls"],
            dtype=np.float64)
        blob["time_limit"] = np.float64((options or {}).get("time_limit", np.inf))
        np.savez_compressed(osp.join(out_dir, f"{name}.npz"), **blob)


if __name__ == "__main__":
    main(sys.argv[1:])
