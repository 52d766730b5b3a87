"""helpers of the executor-timeline tests (tests/test_emu_timeline.py, tests/test_gpu_timeline.py): the fixtures of
tests/golden/make_timeline_golden.py, their replay through the batched env, and the numpy rasteriser the frames are checked
against - written from the rules of include/sss.h (sss_timeline_render), not from the kernel."""
from __future__ import annotations

import json
import math
import os.path as osp

import numpy as np
import torch

from golden_util import GOLDEN_DIR, Golden
from spark_sched_sim_amd import VecSparkSchedSimEnv

HASH_NONE_PERMILLE = 30  # make_golden.hash_policy
# set -> seeds (all the fixture holds)
SETS = {"c1_fair": [0, 1, 2], "c1_hash": [100, 101], "c1_fifo": [5, 6], "c3_fair": [0], "e100_hash": [2], "e120_hash": [0, 1],
        "deep_c1_fair_beta": [4], "tiny_fair_tlimit": [0, 1, 2, 3], "stall": [2002]}


class TimelineGolden:
    def __init__(self, name: str):
        self.name = name
        self.z = np.load(osp.join(GOLDEN_DIR, f"timeline_{name}.npz"))
        self.seeds = [int(s) for s in self.z["seeds"]]
        if name == "stall":
            c = json.load(open(osp.join(GOLDEN_DIR, "stall_case.json")))
            self.cfg = {k: v for k, v in c["env_cfg"].items() if k != "mean_time_limit"}
            self.time_limit = float(c["time_limit"])
            self.policy, self.base = None, None
            self._actions = {int(c["seed"]): (np.asarray(c["stage_idx"]), np.asarray(c["num_exec"]))}
        else:
            self.base = Golden(name)
            self.cfg = dict(self.base.cfg)
            self.time_limit = self.base.time_limit
            self.policy = self.base.policy
            self._actions = {s: (self.base.ep(s, "stage_idx")[1:], self.base.ep(s, "num_exec")[1:]) for s in self.seeds}
        if self.cfg.get("job_arrival_cap") is None:
            self.cfg["max_jobs"] = 64

    def pack(self, default: bytes) -> bytes:
        return self.base.pack(default) if self.base is not None else default

    def ep(self, seed: int, key: str):
        return self.z[f"s{seed}_{key}"]

    def steps(self, seed: int) -> int:
        return int(self.ep(seed, "steps"))

    def actions(self, seed: int):
        return self._actions[seed]

    def history(self, seed: int) -> list[list[list]]:
        """the reference's `[e.history for e in env.executors]`"""
        ptr, t, job = self.ep(seed, "hist_ptr"), self.ep(seed, "hist_t"), self.ep(seed, "hist_job")
        return [[[None if math.isnan(t[k]) else float(t[k]), int(job[k])] for k in range(ptr[e], ptr[e + 1])] for e in range(len(ptr) - 1)]

    def make_env(self, seeds, pack, device, lib=None, cap=256, timeline=True, **kw) -> VecSparkSchedSimEnv:
        env = VecSparkSchedSimEnv(self.cfg, len(seeds), device=device, pack=self.pack(pack), _lib=lib, **kw)
        if timeline:
            env.enable_timeline(cap)
        env.reset(seed=list(seeds), options={"time_limit": self.time_limit})
        return env


def step_actions(tg: TimelineGolden, seeds, i: int, device):
    """the recorded actions of step i (0-based) for every seed; envs whose episode is over are skipped (SSS_SKIP_ENV)"""
    si = torch.full((len(seeds),), -2147483648, dtype=torch.int32)
    ne = torch.ones(len(seeds), dtype=torch.int32)
    for k, s in enumerate(seeds):
        if i < tg.steps(s):
            st, n = tg.actions(s)
            si[k], ne[k] = int(st[i]), int(n[i])
    return si.to(device), ne.to(device)


def check_final(tg: TimelineGolden, env, k: int, seed: int, cap: int | None = None) -> list[str]:
    """env k's recorded rows against seed's final histories, bit for bit (the stored prefix when cap is smaller)"""
    t, job, count = (x[k].cpu().numpy() for x in env.timeline_arrays())
    ptr, ht, hj = tg.ep(seed, "hist_ptr"), tg.ep(seed, "hist_t"), tg.ep(seed, "hist_job")
    cap = t.shape[1] if cap is None else cap
    bad = []
    for e in range(len(ptr) - 1):
        n = int(ptr[e + 1] - ptr[e])
        if int(count[e]) != n:
            bad.append(f"{tg.name} seed {seed} executor {e}: count {int(count[e])}, expected {n}")
            continue
        m = min(n, cap)
        et, ej = ht[ptr[e]: ptr[e] + m].copy(), hj[ptr[e]: ptr[e] + m]
        # (the fixture's NaN and the kernel's are both "None": compared as such, everything else by bits)
        gt = t[e, :m]
        if not (np.array_equal(np.isnan(gt), np.isnan(et)) and np.array_equal(np.where(np.isnan(gt), 0.0, gt).view(np.uint64), np.where(np.isnan(et), 0.0, et).view(np.uint64))
                and np.array_equal(job[e, :m], ej)):
            bad.append(f"{tg.name} seed {seed} executor {e}: entries differ: {list(zip(gt.tolist(), job[e, :m].tolist()))[:6]} expected {list(zip(et.tolist(), ej.tolist()))[:6]}")
    return bad


def replay(tg: TimelineGolden, seeds, pack, device, lib=None, cap=256, bounded=None, check_counts=True, env=None):
    """steps every seed's recorded actions; after every step the entry counts equal the fixture's (min(count, anything) is not
    taken: count is the true count whatever cap is). Returns (env, mismatches)."""
    from replay_util import step_in_bounded_launches
    env = tg.make_env(seeds, pack, device, lib, cap) if env is None else env
    bad: list[str] = []
    launch_no = [0]

    def counts_ok(i):
        cnt = env.timeline_arrays()[2].cpu().numpy()
        for k, s in enumerate(seeds):
            row = tg.ep(s, "counts")[min(i, tg.steps(s))].astype(np.int32)
            if not np.array_equal(cnt[k], row):
                bad.append(f"{tg.name} seed {s} after step {i}: counts {cnt[k].tolist()} expected {row.tolist()}")
                return False
        return True

    if check_counts and not counts_ok(0):
        return env, bad
    for i in range(max(tg.steps(s) for s in seeds)):
        si, ne = step_actions(tg, seeds, i, env.device)
        if bounded is None:
            env.step_async(si, ne)
        else:
            step_in_bounded_launches_skip(env, si, ne, bounded, launch_no, step_in_bounded_launches)
        if check_counts and not counts_ok(i + 1):
            return env, bad
    err = env.obs_i32[:, 7].cpu().numpy()
    if err.any():
        bad.append(f"{tg.name}: env error codes {err.tolist()}")
    for k, s in enumerate(seeds):
        bad += check_final(tg, env, k, s, cap)
    return env, bad


def step_in_bounded_launches_skip(env, si, ne, bounded, launch_no, inner):
    """replay_util.step_in_bounded_launches for a batch in which some envs sit the step out: those count as done from the start"""
    if bool((si == -2147483648).any()):
        done = si == -2147483648
        while not bool(done.all()):
            budget = int(bounded)
            launch_no[0] += 1
            s2 = torch.where(done, torch.full_like(si, -2147483648), si).contiguous()
            ready = env.step_bounded_async(s2, ne, budget).bool()
            done = done | (ready & (s2 != -2147483648))
            assert launch_no[0] < 10 ** 7
    else:
        inner(env, si, ne, bounded, launch_no)


# ---- the frame, from the rules of include/sss.h ----

C1 = np.array([0.0, 100.0, 255.0])
C2 = np.array([2.0, 247.0, 112.0])


def job_colour(j: int, J: int):
    if j < 0:
        return (0, 0, 0)
    p = np.float64(j + 1) / np.float64(J)
    return tuple(int(v) for v in np.trunc(C1 + p * (C2 - C1)))


def numpy_frame(t, job, count, T: float, J: int, t_completed, W: int, H: int) -> np.ndarray:
    """t f64[E, cap], job i32[E, cap], count i32[E] of one env -> uint8 [H, W, 3]"""
    E, cap = t.shape
    img = np.zeros((H, W, 3), dtype=np.uint8)
    rh = -(-H // E)
    T = np.float64(T)
    for i in range(E):
        y0, y1 = i * rh, min((i + 1) * rh, H)
        if y0 >= y1:
            continue
        n = int(count[i])
        overflow = n > cap
        release = list(t[i, :cap]) if overflow else list(t[i, : n - 1]) + [np.inf]   # the open entry's release is +inf
        jobs = list(job[i, :cap]) if overflow else list(job[i, :n])
        for x in range(W):
            if T <= 0:
                col = (128, 128, 128) if overflow else job_colour(int(jobs[-1]), J)
            else:
                tx = (np.float64(x) + 0.5) * (T / np.float64(W))
                k = next((k for k, r in enumerate(release) if tx < r), None)
                col = (128, 128, 128) if k is None else job_colour(int(jobs[k]), J)
            img[y0:y1, x] = col
    if T > 0:
        for tc in t_completed:
            if tc < T:
                x = min(W - 1, int(np.floor(np.float64(W) * np.float64(tc) / T)))
                img[:, x] = (255, 0, 0)
    return img


def expected_frames(env, env_ids, W: int, H: int) -> np.ndarray:
    t, job, count = (x.cpu().numpy() for x in env.timeline_arrays())
    out = []
    for i in env_ids:
        h = env.header(i)
        _, tc, _, _ = env.job_times(i)
        out.append(numpy_frame(t[i], job[i], count[i], h["wall_time"], h["J"], tc, W, H))
    return np.stack(out) if out else np.zeros((0, H, W, 3), np.uint8)
