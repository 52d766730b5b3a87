"""The checks of env copies (VecSparkSchedSimEnv.fork / snapshot / restore, SparkSchedSimEnv.__deepcopy__, evaluation.continuations;
include/sss.h sss_env_copy, csrc/sss_fork.h), shared by tests/test_emu_fork.py (the CPU wave emulator: the plain-loop form of the
copy) and tests/test_gpu_fork.py (the kernel). Every check takes (device, lib): ("cpu", the emulator's library) or ("cuda:0", None).
A copy is held to the recorded trajectories of tests/golden: a fork of an env that replays a fixture must show the fixture's
observation before it takes a step and then finish on the fixture, step for step, with the comparisons of replay_util.replay_golden."""
from __future__ import annotations

import copy
import ctypes as C
import os.path as osp
import re
import subprocess

import numpy as np
import torch

from golden_util import Golden, bits
from spark_sched_sim_amd import SparkSchedSimEnv, VecSparkSchedSimEnv
from spark_sched_sim_amd.digest import digest_words
from spark_sched_sim_amd.vec_env import HDR_OFF, HDR_PROF

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
SKIP = -2147483648
TINY = dict(num_executors=5, job_arrival_cap=8, job_arrival_rate=1.0e-4, moving_delay=1500.0, warmup_delay=500.0)
C1 = dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
# SssHdr words (8 bytes each) that belong to an env's lifetime and stay the destination's: n_steps, n_events, model_bytes, prof[5],
# n_fast, n_batched, n_rounds
LIFETIME_BYTES = [(HDR_OFF["n_steps"], HDR_OFF["model_bytes"] + 8), (HDR_PROF, HDR_OFF["n_rounds"] + 8)]
RNG_BYTES = (0, 40)  # rng_state_hi/lo, rng_inc_hi/lo, rng_has32, rng_u32


def golden_cfg(g: Golden) -> dict:
    cfg = dict(g.cfg)
    if cfg.get("job_arrival_cap") is None:
        cfg["max_jobs"] = 64
    return cfg


def pool_layout(env) -> dict:
    """where the pool records and the overflow area lie in an env's block: csrc/sss_layout.h sss_compute_layout, restated (the dims
    the library reports hold the offsets on either side)"""
    d = env.dims
    J, SP, E = d.job_cap, d.stage_stride, env.num_executors
    al = lambda x: (x + 63) // 64 * 64  # noqa: E731
    off_stages = d.off_t_completed + 8 * J
    off_durations = al(off_stages + 8 * J * SP)
    off_pool_hdr = al(off_durations + 4 * J * SP)
    n_pools = 1 + J + J * SP
    off_pool_tab = al(off_pool_hdr + 16 * n_pools)
    table = 1024 if E >= 128 else (512 if E >= 64 else 256)
    assert off_pool_tab + table * n_pools == d.off_dur_ring, "the layout restated here has drifted from csrc/sss_layout.h"
    return dict(off_pool_hdr=off_pool_hdr, off_pool_tab=off_pool_tab, n_pools=n_pools, table=table)


def env_bytes(env, i: int) -> dict[str, np.ndarray]:
    """everything env i owns: its arena block, its observation rows, its timeline rows"""
    out = {"state": env._env_view[i], "nodes": env.nodes[i], "edge_links": env.edge_links[i], "dag_ptr": env.dag_ptr[i],
           "exec_supplies": env.exec_supplies[i], "obs_i32": env.obs_i32[i], "obs_f64": env.obs_f64[i]}
    if getattr(env, "_timeline", None) is not None:
        out.update({"tl_t": env._timeline[0][i], "tl_job": env._timeline[1][i], "tl_count": env._timeline[2][i]})
    return {k: v.cpu().numpy().copy().view(np.uint8) for k, v in out.items()}


def same_bytes(a: dict, b: dict) -> list[str]:
    return [k for k in a if not np.array_equal(a[k], b[k])]


def obs_mismatch(env, k: int, g: Golden, s: int, i: int) -> str | None:
    """env k's outputs against step i of seed s's recording: the comparisons of replay_util.replay_golden"""
    o = env.obs_i32[k].cpu().numpy()
    of = env.obs_f64[k].cpu().numpy()
    got = (int(o[0]), int(o[1]), int(o[2]), int(o[4]), int(o[5]))
    exp = tuple(int(g.ep(s, kk)[i]) for kk in ("n_nodes", "n_edges", "n_jobs", "ncommit", "src_idx"))
    ok = got == exp and bits(of[1]) == int(g.ep(s, "wall_time")[i]) and int(o[7]) == 0
    if i > 0:
        ok = ok and bits(of[0]) == bits(g.ep(s, "reward")[i: i + 1].view(np.float64)[0]) and bool(o[6]) == bool(g.ep(s, "terminated")[i])
    if ok:
        n, ne, a = got[0], got[1], got[2]
        d = (digest_words(env.nodes[k, :n].cpu().numpy()), digest_words(env.edge_links[k, :ne].cpu().numpy()),
             digest_words(env.dag_ptr[k, : a + 1].cpu().numpy()), digest_words(env.exec_supplies[k, :a].cpu().numpy()))
        ok = d == tuple(int(g.ep(s, kk)[i]) for kk in ("d_nodes", "d_edges", "d_ptr", "d_sup"))
        if not ok:
            return f"{g.name} seed {s} step {i} (env {k}): observation digests differ"
    return None if ok else f"{g.name} seed {s} step {i} (env {k}): got {got} err={int(o[7])} reward={of[0]!r} wall={of[1]!r}; expected {exp}"


def totals_mismatch(env, k: int, g: Golden, s: int) -> str | None:
    ta, tc, _, tmpl = env.job_times(k)
    if not np.array_equal(ta.view(np.uint64), g.ep(s, "t_arrival").view(np.uint64)) or not np.array_equal(tmpl.astype(np.int32), g.ep(s, "template")):
        return f"{g.name} seed {s} (env {k}): arrival times / templates differ"
    wall, arrived = env.obs_f64[k, 1].item(), env.header(k)["next_arrival"]
    dur = np.sort(np.minimum(tc[:arrived], wall) - ta[:arrived])
    return None if np.array_equal(dur, np.sort(g.ep(s, "job_durations"))) else f"{g.name} seed {s} (env {k}): job durations differ"


def n_steps(g: Golden, s: int) -> int:
    return len(g.ep(s, "reward"))


def step_envs(env, acts: dict[int, tuple[int, int]], policy_envs=()) -> None:
    """one launch: env k takes acts[k]; the envs of `policy_envs` the fair policy's action; every other env sits it out"""
    B = env.num_envs
    si = torch.full((B,), SKIP, dtype=torch.int32)
    ne = torch.ones(B, dtype=torch.int32)
    for k, (st, n) in acts.items():
        si[k], ne[k] = st, n
    si, ne = si.to(env.device), ne.to(env.device)
    if policy_envs:
        a = env.policy_actions("fair")
        sel = torch.zeros(B, dtype=torch.bool)
        sel[list(policy_envs)] = True
        sel = sel.to(env.device)
        live = sel & (env.obs_i32[:, 6] == 0) & (env.obs_i32[:, 7] == 0)
        si, ne = torch.where(live, a["stage_idx"], si).contiguous(), torch.where(live, a["num_exec"], ne).contiguous()
    env.step_async(si, ne)


def recorded(g: Golden, s: int, i: int) -> tuple[int, int]:
    """the action that leads from step i to step i + 1"""
    return int(g.ep(s, "stage_idx")[i + 1]), int(g.ep(s, "num_exec")[i + 1])


def replay_rest(env, ks, g: Golden, s: int, i0: int, others=()) -> list[str]:
    """the envs `ks` are at step i0 of seed s's recording: they take the remaining recorded actions (the envs of `others` play the
    fair policy alongside) and must match every remaining step and the final job times"""
    bad: list[str] = []
    n = n_steps(g, s)
    for i in range(i0, n - 1):
        step_envs(env, {k: recorded(g, s, i) for k in ks}, others)
        for k in ks:
            m = obs_mismatch(env, k, g, s, i + 1)
            if m:
                return bad + [m]
    if int(g.ep(s, "error_step")) < 0:
        bad += [m for m in (totals_mismatch(env, k, g, s) for k in ks) if m]
    return bad


def make_env(g: Golden, seeds, pack, device, lib, timeline=False, **kw):
    env = VecSparkSchedSimEnv(golden_cfg(g), len(seeds), device=device, pack=g.pack(pack), _lib=lib, **kw)
    if timeline:
        env.enable_timeline(256)
    env.reset(seed=list(seeds), options={"time_limit": g.time_limit})
    return env


# ---- 1. a fork continues the recorded trajectory -------------------------------------------------

def fork_points(g: Golden, s: int) -> list[int]:
    n = n_steps(g, s)
    return sorted({0, n // 3, n - 2})


def check_fork_continues(name: str, seed: int, k: int, pack, device, lib) -> None:
    """three envs. 0 replays the fixture to step k; 1 and 2 have played ~50 steps of other seeds (every buffer of theirs is dirty);
    fork 0 -> 1. Env 1 shows the fixture's step k before it takes a step and finishes on the fixture while env 0, reset to another
    seed, plays something else beside it; env 2, never named, is byte for byte what it was"""
    g = Golden(name)
    env = make_env(g, [seed, seed + 1001, seed + 2002], pack, device, lib)
    for _ in range(50):
        step_envs(env, {}, policy_envs=(1, 2))
    for i in range(k):
        step_envs(env, {0: recorded(g, seed, i)})
    assert obs_mismatch(env, 0, g, seed, k) is None
    before = env_bytes(env, 2)
    env.fork(0, 1)
    assert same_bytes(before, env_bytes(env, 2)) == [], "a fork wrote to an env it was not given"
    m = obs_mismatch(env, 1, g, seed, k)
    assert m is None, m
    env.reset(seed=[seed + 3003] * 3, options={"time_limit": g.time_limit}, mask=torch.tensor([1, 0, 0], dtype=torch.uint8).to(env.device))
    bad = replay_rest(env, [1], g, seed, k, others=(0,))
    assert not bad, "\n".join(bad)
    assert same_bytes(before, env_bytes(env, 2)) == []
    env.close()


# ---- 2. a fork diverges as the reference's deepcopy does -----------------------------------------

class ForkGolden:
    """tests/golden/fork_<set>.npz (make_fork_golden.py): the children of the reference's `copy.deepcopy(env)` at step k of a base
    fixture; `ep(child, key)` reads like Golden.ep with the child's name in the seed's place"""

    def __init__(self, name: str):
        from golden_util import GOLDEN_DIR
        self.name = f"fork_{name}"
        self.z = np.load(osp.join(GOLDEN_DIR, f"fork_{name}.npz"))
        self.base, self.seed, self.k, self.reseed = Golden(str(self.z["base"])), int(self.z["seed"]), int(self.z["k"]), int(self.z["reseed"])
        self.children = [str(c) for c in self.z["children"]]

    def ep(self, child: str, key: str):
        return self.z[f"{child}_{key}"]

    def history(self, child: str) -> list[list[list]]:
        ptr, t, job = self.ep(child, "hist_ptr"), self.ep(child, "hist_t"), self.ep(child, "hist_job")
        return [[[None if np.isnan(t[k]) else float(t[k]), int(job[k])] for k in range(ptr[e], ptr[e + 1])] for e in range(len(ptr) - 1)]


def check_fork_diverges(name: str, pack, device, lib) -> None:
    """env 0 replays the base fixture to step k with the timeline on; env 1 becomes a plain fork, env 2 one reseeded with 777. Each
    child replays the actions the reference's copy took under its FIFO scheduler and must give the reference's bits at every step -
    rewards, clocks, observation digests - its completion times and its `Executor.history`, the part before the fork included;
    the parent goes on beside them and still ends on the base fixture"""
    fg = ForkGolden(name)
    g, seed, k = fg.base, fg.seed, fg.k
    assert fg.children == ["plain", f"r{fg.reseed}"]
    env = make_env(g, [seed, seed + 1001, seed + 2002], pack, device, lib, timeline=True)
    for _ in range(20):
        step_envs(env, {}, policy_envs=(1, 2))
    for i in range(k):
        step_envs(env, {0: recorded(g, seed, i)})
    env.fork(0, 1)
    env.fork([0], [2], reseed=[fg.reseed])
    who = {1: fg.children[0], 2: fg.children[1]}
    bad = [m for m in (obs_mismatch(env, e, fg, c, 0) for e, c in who.items()) if m]
    assert not bad, "\n".join(bad)
    n_parent = n_steps(g, seed) - 1 - k
    for i in range(max(max(n_steps(fg, c) for c in who.values()) - 1, n_parent)):
        acts = {e: recorded(fg, c, i) for e, c in who.items() if i < n_steps(fg, c) - 1}
        if i < n_parent:
            acts[0] = recorded(g, seed, k + i)
        step_envs(env, acts)
        bad = [m for m in (obs_mismatch(env, e, fg, c, i + 1) for e, c in who.items() if e in acts) if m]
        assert not bad, "\n".join(bad)
    m = obs_mismatch(env, 0, g, seed, n_steps(g, seed) - 1) or totals_mismatch(env, 0, g, seed)
    assert m is None, m
    assert bits(env.header(0)["wall_time"]) == bits(fg.z["parent_final_wall"])
    for e, c in who.items():
        ta, tc, _, _ = env.job_times(e)
        assert np.array_equal(ta.view(np.uint64), fg.ep(c, "t_arrival").view(np.uint64)), c
        assert np.array_equal(tc.view(np.uint64), fg.ep(c, "t_completed").view(np.uint64)), c
        assert env.timeline(e) == fg.history(c), c
        assert env.header(e)["terminated"] == 1 and env.header(e)["err"] == 0
    assert not np.array_equal(fg.ep("plain", "wall_time"), fg.ep(f"r{fg.reseed}", "wall_time"))
    env.close()


# ---- 3. reseed is numpy's fresh generator --------------------------------------------------------

def dense_ranges(env) -> list[tuple[int, int]]:
    lay = pool_layout(env)
    return [(0, lay["off_pool_tab"]), (env.dims.off_dur_ring, env.dims.env_stride)]


def check_reseed(seed_value: int, pack, device, lib) -> None:
    env = VecSparkSchedSimEnv(TINY, 2, device=device, pack=pack, _lib=lib)
    env.reset(seed=[11, 12])
    for _ in range(9):
        step_envs(env, {}, policy_envs=(0, 1))
    own = env._env_view[1].cpu().numpy().copy()
    env.fork(0, 1, reseed=[seed_value])
    src, dst = env._env_view[0].cpu().numpy(), env._env_view[1].cpu().numpy()
    st = np.random.PCG64(np.random.SeedSequence(seed_value)).state
    assert (st["has_uint32"], st["uinteger"]) == (0, 0)
    words = dst[:32].view(np.uint64)
    state, inc = st["state"]["state"], st["state"]["inc"]
    assert [int(w) for w in words] == [state >> 64, state & (2 ** 64 - 1), inc >> 64, inc & (2 ** 64 - 1)]
    assert not dst[32:40].any()  # rng_has32 == rng_u32 == 0
    keep = np.ones(env.dims.env_stride, dtype=bool)
    keep[RNG_BYTES[0]: RNG_BYTES[1]] = False
    for a, b in LIFETIME_BYTES:
        keep[a:b] = False
        assert np.array_equal(dst[a:b], own[a:b])
    dense = np.zeros_like(keep)
    for a, b in dense_ranges(env):
        dense[a:b] = True
    assert np.array_equal(dst[dense & keep], src[dense & keep]), "a reseeded fork differs from its source outside the generator"
    env.close()


# ---- 4. what an image is ---------------------------------------------------------------------------

def check_image_definition(pack, device, lib) -> None:
    env = VecSparkSchedSimEnv(C1, 3, device=device, pack=pack, _lib=lib)
    env.enable_timeline(64)
    env.reset(seed=[5, 6, 7])
    for _ in range(60):
        step_envs(env, {}, policy_envs=(0, 1))
    for _ in range(25):
        step_envs(env, {}, policy_envs=(1, 2))
    lay = pool_layout(env)
    own, bystander, totals = env._env_view[1].cpu().numpy().copy(), env_bytes(env, 2), env.counters()
    whole = env.state.cpu().numpy().copy()
    # n = 0 and refused ids write nothing
    env.fork([], [])
    for s, d in (([0], [3]), ([-1], [1]), ([0, 0], [1, 1]), ([0, 1], [2, 0]), ([0], [0])):
        try:
            env.fork(s, d)
        except ValueError:
            pass
        else:
            raise AssertionError(f"fork({s}, {d}) was not refused")
    try:
        env.fork([0, 1], [2])
    except ValueError:
        pass
    else:
        raise AssertionError("fork with 2 sources and 1 destination was not refused")
    assert np.array_equal(env.state.cpu().numpy(), whole)
    env.fork([0], [1])
    src, dst = env._env_view[0].cpu().numpy(), env._env_view[1].cpu().numpy()
    keep = np.zeros(env.dims.env_stride, dtype=bool)
    for a, b in dense_ranges(env):
        keep[a:b] = True
    for a, b in LIFETIME_BYTES:
        keep[a:b] = False
        assert np.array_equal(dst[a:b], own[a:b]), "a lifetime field of the destination changed"
        assert not np.array_equal(own[a:b], src[a:b]), "(the two envs' lifetime fields should differ for this to show anything)"
    assert np.array_equal(dst[keep], src[keep])
    masks = src[lay["off_pool_hdr"]: lay["off_pool_hdr"] + 16 * lay["n_pools"]].view(np.uint16)[::8]
    grown = np.nonzero(masks != 7)[0]
    assert 0 in grown  # ten executors: the common pool's table has 32 slots from the reset on
    for p in grown:
        a = lay["off_pool_tab"] + int(p) * lay["table"]
        assert np.array_equal(dst[a: a + lay["table"]], src[a: a + lay["table"]]), f"table of pool {p}"
    assert env.counters() == totals
    o = env.obs_i32[0].cpu().numpy()
    n, ne, a = int(o[0]), int(o[1]), int(o[2])
    assert torch.equal(env.nodes[1, :n], env.nodes[0, :n]) and torch.equal(env.edge_links[1, :ne], env.edge_links[0, :ne])
    assert torch.equal(env.dag_ptr[1, : a + 1], env.dag_ptr[0, : a + 1]) and torch.equal(env.exec_supplies[1, :a], env.exec_supplies[0, :a])
    assert torch.equal(env.obs_i32[1], env.obs_i32[0]) and torch.equal(env.obs_f64[1], env.obs_f64[0])
    assert env.timeline(1) == env.timeline(0)
    assert same_bytes(bystander, env_bytes(env, 2)) == []
    # ids on the device go through unchecked; one outside the store is skipped by the kernel
    whole = env.state.cpu().numpy().copy()
    env.fork(torch.tensor([0, 0, 5], dtype=torch.int32).to(env.device), torch.tensor([7, -3, 1], dtype=torch.int32).to(env.device))
    assert np.array_equal(env.state.cpu().numpy(), whole)
    env.close()


# ---- 5. a fork in the middle of a step ----------------------------------------------------------

def check_mid_step_fork(pack, device, lib) -> None:
    g, seed = Golden("c1_hash"), 100
    env = make_env(g, [seed, seed + 1001], pack, device, lib)
    dev = env.device

    def bounded(acts):
        si = torch.full((2,), SKIP, dtype=torch.int32)
        ne = torch.ones(2, dtype=torch.int32)
        for k, (st, n) in acts.items():
            si[k], ne[k] = st, n
        return env.step_bounded_async(si.to(dev), ne.to(dev), 3).cpu().numpy().copy()

    i = 0
    while True:  # env 0 replays until a step is cut at its budget
        ready = bounded({0: recorded(g, seed, i)})
        if not ready[0]:
            break
        i += 1
        assert obs_mismatch(env, 0, g, seed, i) is None
        assert i < n_steps(g, seed) - 45, "no step of the recording needs more than 3 events"
    assert env.header(0)["n_steps"] >= 0 and int(env._env_view[0, 280:284].cpu().numpy().view(np.int32)[0]) == 1  # SssHdr::mid_step
    env.fork(0, 1)
    assert int(env._ready[1]) == 0
    pending = {0, 1}
    for _ in range(10 ** 5):  # both finish the step in further launches (a continuing env's action entries are ignored)
        ready = bounded({k: (-1, 1) for k in pending})
        pending = {k for k in pending if not ready[k]}
        if not pending:
            break
    assert not pending
    i += 1
    bad = [m for m in (obs_mismatch(env, k, g, seed, i) for k in (0, 1)) if m]
    for j in range(i, i + 40):
        if bad:
            break
        step_envs(env, {0: recorded(g, seed, j), 1: recorded(g, seed, j)})
        bad = [m for m in (obs_mismatch(env, k, g, seed, j + 1) for k in (0, 1)) if m]
    assert not bad, "\n".join(bad)
    env.close()


# ---- 6. snapshot and restore -----------------------------------------------------------------------

def check_snapshot_restore(pack, device, lib) -> None:
    from timeline_util import TimelineGolden, check_final
    g, seed = Golden("c1_fair"), 0
    tg = TimelineGolden("c1_fair")
    k = n_steps(g, seed) // 3
    env = make_env(g, [seed, seed + 1001], pack, device, lib, timeline=True)
    for _ in range(30):
        step_envs(env, {}, policy_envs=(1,))
    for i in range(k):
        step_envs(env, {0: recorded(g, seed, i)})
    snap = env.snapshot([0])
    assert snap.num_slots == 1 and snap.layout_id == env.layout_id and snap.nbytes > env.dims.env_stride
    assert int(snap.seeds[0]) == seed and float(snap.time_limits[0]) == g.time_limit
    bad = replay_rest(env, [0], g, seed, k)
    assert not bad, "\n".join(bad)
    final = env._env_view[0].cpu().numpy().copy()
    # back to step k - in the env it came from and in another index - and to the end again: the same bits
    env.restore(snap)
    env.restore(snap, env_ids=[1])
    for e in (0, 1):
        m = obs_mismatch(env, e, g, seed, k)
        assert m is None, m
    bad = replay_rest(env, [0, 1], g, seed, k)
    assert not bad, "\n".join(bad)
    again = env._env_view[0].cpu().numpy()
    life = np.ones(env.dims.env_stride, dtype=bool)
    for a, b in LIFETIME_BYTES:
        life[a:b] = False
    assert np.array_equal(again[life], final[life]), "the second run from the snapshot left other bytes than the first"
    bad = [m for e in (0, 1) for m in check_final(tg, env, e, seed)]
    assert not bad, "\n".join(bad)  # the histories, the part before the snapshot included
    # another VecSparkSchedSimEnv of the same configuration and another num_envs
    other = make_env(g, [7, 8, 9], pack, device, lib, timeline=True)
    other.restore(snap, env_ids=[2])
    m = obs_mismatch(other, 2, g, seed, k)
    assert m is None, m
    bad = replay_rest(other, [2], g, seed, k) + check_final(tg, other, 2, seed)
    assert not bad, "\n".join(bad)
    other.close()
    # other layouts are refused
    for change in (dict(num_executors=C1["num_executors"] + 1), dict(max_jobs=60)):
        wrong = VecSparkSchedSimEnv({**golden_cfg(g), **change}, 2, device=device, pack=g.pack(pack), _lib=lib)
        wrong.reset(seed=[1, 2])
        held = wrong.state.cpu().numpy().copy()
        try:
            wrong.restore(snap, env_ids=[0])
        except ValueError as e:
            assert "layout" in str(e)
        else:
            raise AssertionError(f"a snapshot was restored into an env with {change}")
        try:  # ... by the library as well, whatever the Python side checks
            wrong._env_copy(snap._store(), None, torch.zeros(1, dtype=torch.int32).to(wrong.device), torch.zeros(1, dtype=torch.int32).to(wrong.device), None)
        except ValueError as e:
            assert "-51" in str(e) and "layout" in str(e)
        else:
            raise AssertionError("sss_env_copy took a store of another layout")
        assert np.array_equal(wrong.state.cpu().numpy(), held)
        wrong.close()
    env.close()


def check_abi(lib, tmp_path) -> None:
    """the two argument structures of sss_env_copy: registered with sss_abi_sizeof, mirrored field for field"""
    from spark_sched_sim_amd import binding as B
    for sym in ("sss_env_copy", "sss_env_layout_id"):
        assert sym in B.EXPORTS and hasattr(lib, sym)
    assert set(B.ABI_STORE_STRUCTS) == {"sss_env_store", "sss_env_copy_args"}
    header = open(osp.join(ROOT, "include", "sss.h")).read()
    assert set(re.findall(r"^struct (sss_[a-z_]+)\n\{", header, re.M)) == set(B.ABI_STORE_STRUCTS)
    lib.sss_abi_sizeof.argtypes = [C.c_char_p]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{osp.join(ROOT, "include", "sss.h")}"', "int main(void) {"]
    for cname, cls in B.ABI_STORE_STRUCTS.items():
        assert lib.sss_abi_sizeof(cname.encode()) == C.sizeof(cls), cname
        lines.append(f'  printf("{cname} %zu\\n", sizeof(struct {cname}));')
        for fname, *_ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof(struct {cname}, {fname}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")], check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in B.ABI_STORE_STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, *_ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


# ---- 7. the facade -----------------------------------------------------------------------------------

def check_facade_deepcopy(device, lib) -> None:
    from timeline_util import TimelineGolden
    g, seed = Golden("c1_fair"), 0
    tg = TimelineGolden("c1_fair")
    n = n_steps(g, seed)
    k = n // 3
    env = SparkSchedSimEnv(golden_cfg(g), device=device, _lib=lib)
    env.reset(seed=seed)
    for i in range(k):
        st, ne = recorded(g, seed, i)
        env.step({"stage_idx": st, "num_exec": ne})
    twin = copy.deepcopy(env)
    assert twin is not env and twin._vec is not env._vec
    assert obs_mismatch(twin._vec, 0, g, seed, k) is None
    assert twin.job_arrival_cap == env.job_arrival_cap and twin.action_space["stage_idx"].n == env.action_space["stage_idx"].n
    assert twin.observation_space["source_job_idx"].n == env.observation_space["source_job_idx"].n
    held_obs, held_hist = env_bytes(env._vec, 0), [e.history for e in env.executors]
    assert [e.history for e in twin.executors] == held_hist
    st, ne = recorded(g, seed, k)
    twin.step({"stage_idx": st, "num_exec": ne})
    assert same_bytes(held_obs, env_bytes(env._vec, 0)) == [] and [e.history for e in env.executors] == held_hist
    for who, i0 in ((env, k), (twin, k + 1)):
        for i in range(i0, n - 1):
            st, ne = recorded(g, seed, i)
            _, reward, term, _, info = who.step({"stage_idx": st, "num_exec": ne})
            assert bits(reward) == int(g.ep(seed, "reward")[i + 1]) and bits(info["wall_time"]) == int(g.ep(seed, "wall_time")[i + 1]), (i, who is twin)
            assert term == bool(g.ep(seed, "terminated")[i + 1])
        assert totals_mismatch(who._vec, 0, g, seed) is None
        assert [e.history for e in who.executors] == tg.history(seed)
    env.close(), twin.close()


# ---- 8. evaluation.continuations ------------------------------------------------------------------

def check_continuations(pack, device, lib) -> None:
    from spark_sched_sim_amd import evaluation
    env = VecSparkSchedSimEnv(TINY, 6, device=device, pack=pack, _lib=lib)
    env.reset(seed=[21, 22, 23, 24, 25, 26])
    for _ in range(12):
        step_envs(env, {}, policy_envs=(0, 5))
    for _ in range(5):
        step_envs(env, {}, policy_envs=(1, 2, 3, 4))
    ta_parent = env.job_times(0)[0]
    for policy, dst, seeds in (("fair", [1, 2], [101, 102]), ("fifo", [3, 4], [101, 102])):
        others = [e for e in range(6) if e not in dst]
        held = {e: env_bytes(env, e) for e in others}
        r = evaluation.continuations(env, [0, 0], dst, policy, reseed=seeds, max_steps=2000)
        assert bool(r["ok"].all()) and r["avg_job_duration_s"].shape == (2,) and int(r["num_completed_jobs"][0]) == TINY["job_arrival_cap"]
        for e in dst:
            assert env.header(e)["err"] == 0 and env.header(e)["terminated"] == 1
            assert np.array_equal(env.job_times(e)[0].view(np.uint64), ta_parent.view(np.uint64))
        for e in others:
            assert same_bytes(held[e], env_bytes(env, e)) == [], f"env {e} took no part and changed"
    env.close()
