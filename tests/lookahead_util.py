"""The checks of the lookahead scheduler and the two entry points under it (include/sss.h sss_rollout_each, sss_lookahead_pick;
VecSparkSchedSimEnv.rollout_each / lookahead_pick, lookahead.LookaheadScheduler, evaluation.run_lookahead, evaluation.continuations
with fused=True), shared by tests/test_emu_lookahead.py (the CPU wave emulator) and tests/test_gpu_lookahead.py (the kernels). Every
check takes (device, lib): ("cpu", the emulator's library) or ("cuda:0", None). What the new paths are held to is the existing ones:
`env.rollout`, `policy_actions` + `step_async`, `evaluation.continuations`, `job_stats` - bit for bit."""
from __future__ import annotations

import numpy as np
import torch

from fork_util import SKIP, TINY, env_bytes, same_bytes, step_envs
from spark_sched_sim_amd import VecSparkSchedSimEnv, evaluation
from spark_sched_sim_amd.binding import POLICY_IDS
from spark_sched_sim_amd.lookahead import LookaheadScheduler
from spark_sched_sim_amd.vec_env import HDR_PROF

CANDIDATES = [("fair", 0), ("fifo", 0), ("sjfcp", 0), ("wfair", 1)]
EACH_POLICIES = [("fair", 0), ("fifo", 0), ("sjfcp", 0), ("wfair", 1), ("wfair", -1), ("hash", 100)]


def cfg_of(num_executors: int) -> dict:
    return {**TINY, "num_executors": num_executors}


def i32(env, v) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.int32).to(env.device)


def no_ticks(b: dict) -> dict:
    """env_bytes without the header's five shader-clock counters (prof[5]: two runs of the same steps differ there on a GPU)"""
    b = dict(b)
    s = b["state"].copy()
    s[HDR_PROF: HDR_PROF + 40] = 0
    b["state"] = s
    return b


def live_image(env, e: int) -> dict:
    """no_ticks(env_bytes) without the commitment entries behind the live ones (SssHot c_src / c_dst / c_seq / c_n from index n_commits
    on): a launch's end writes the live entries only and nothing ever reads the others (csrc/sss_sim_env.h env_end), so they show
    where the launch boundaries were - which is exactly what differs between one fused launch and a step launch followed by one"""
    b = no_ticks(env_bytes(env, e))
    M = 64 if env.num_executors <= 64 else 128
    n = env.header(e)["n_commits"]
    at = 320 + M * (16 + 4 + 2 + 1 + 1)  # csrc/sss_layout.h SssHot: header, ev, ex_loc, ex_job, ex_task_stage, ex_executing
    for width in (4, 4, 4, 2):
        b["state"][at + n * width: at + M * width] = 0
        at += M * width
    # ... and likewise the ordered active-job list behind its n_active entries (u16 each; behind the list: the old-active copy of
    # a step cut at its event budget, which no env here is in)
    b["state"][env.dims.off_active + 2 * env.header(e)["n_active"]: env.dims.off_jobs] = 0
    return b


def per_env(env, entries: dict[int, tuple[str, int]]) -> tuple[torch.Tensor, torch.Tensor]:
    pol, par = [-1] * env.num_envs, [-1] * env.num_envs
    for e, (name, p) in entries.items():
        pol[e], par[e] = POLICY_IDS[name], p
    return i32(env, pol), i32(env, par)


def lock_step(env, ids, policy: str, param: int, n: int) -> None:
    """n x (policy_actions -> step) for the envs `ids` that are not over; every other env sits the launches out"""
    sel = torch.zeros(env.num_envs, dtype=torch.bool)
    sel[list(ids)] = True
    sel = sel.to(env.device)
    skip = torch.full((env.num_envs,), SKIP, dtype=torch.int32, device=env.device)
    for _ in range(n):
        a = env.policy_actions(policy, param)
        live = sel & (env.obs_i32[:, 6] == 0) & (env.obs_i32[:, 7] == 0)
        env.step_async(torch.where(live, a["stage_idx"], skip).contiguous(), a["num_exec"])


# ---- 1. rollout_each equals the existing fused rollout, env by env ---------------------------------

def check_each_equals_rollout(num_executors: int, pack, device, lib) -> None:
    cfg, seeds, n = cfg_of(num_executors), list(range(21, 29)), 40
    env = VecSparkSchedSimEnv(cfg, 8, device=device, pack=pack, _lib=lib)
    env.reset(seed=seeds)
    env.rollout("fair", 5)
    held = {e: env_bytes(env, e) for e in (6, 7)}
    before = env.header_field("ep_steps").clone()
    pol, par = per_env(env, dict(enumerate(EACH_POLICIES)))
    out = env.rollout_each(pol, par, n)
    for e in (6, 7):
        assert same_bytes(held[e], env_bytes(env, e)) == [], f"env {e} has policy -1 and changed"
    steps = out["steps"].cpu().numpy()
    assert np.array_equal(steps, (env.header_field("ep_steps") - before).cpu().numpy()) and (steps[:6] > 0).all() and (steps[6:] == 0).all()
    assert (out["first_stage_idx"][6:] == -1).all() and (out["first_num_exec"][:6] >= 1).all()
    for k, (name, p) in enumerate(EACH_POLICIES):
        ref = VecSparkSchedSimEnv(cfg, 1, device=device, pack=pack, _lib=lib)
        ref.reset(seed=[seeds[k]])
        ref.rollout("fair", 5)
        ref.rollout(name, n, p)
        bad = same_bytes(no_ticks(env_bytes(ref, 0)), no_ticks(env_bytes(env, k)))
        assert bad == [], f"env {k} under {name}:{p} differs from env.rollout in {bad}"
        ref.close()
    env.close()


# ---- 2. the first step's policy ----------------------------------------------------------------------

def check_first_step_policy(pack, device, lib) -> None:
    seeds, n = [31, 32, 33, 34], 25
    env = VecSparkSchedSimEnv(TINY, 4, device=device, pack=pack, _lib=lib)
    ref = VecSparkSchedSimEnv(TINY, 4, device=device, pack=pack, _lib=lib)
    for e in (env, ref):
        e.reset(seed=seeds)
        e.rollout("sjfcp", 12)
    pol, par = per_env(env, {e: ("fair", 0) for e in range(4)})
    fpol, fpar = per_env(env, {e: ("fifo", 0) for e in (0, 1, 2)})  # (env 3: a negative entry - the first step is fair's as well)
    out = env.rollout_each(pol, par, n, fpol, fpar)
    a = ref.policy_actions("fifo")
    act = (a["stage_idx"].clone(), a["num_exec"].clone())
    fair = ref.policy_actions("fair")
    act[0][3], act[1][3] = fair["stage_idx"][3], fair["num_exec"][3]
    ref.step_async(act[0], act[1])
    ref.rollout("fair", n - 1)
    assert torch.equal(out["first_stage_idx"], act[0]) and torch.equal(out["first_num_exec"], act[1])
    for e in range(4):
        bad = same_bytes(live_image(ref, e), live_image(env, e))
        assert bad == [], f"env {e}: {bad}"
    env.close(), ref.close()


# ---- 3. an env stops at the end of its episode -------------------------------------------------------

def check_stops_at_the_end(num_executors: int, pack, device, lib) -> None:
    env = VecSparkSchedSimEnv(cfg_of(num_executors), 4, device=device, pack=pack, _lib=lib)
    env.reset(seed=[41, 42, 43, 44])
    pol, par = per_env(env, dict(enumerate(CANDIDATES)))
    out = env.rollout_each(pol, par, 100000)
    assert (env.header_field("terminated") == 1).all() and (env.header_field("err") == 0).all() and (env.obs_i32[:, 6] == 1).all()
    assert torch.equal(out["steps"], env.header_field("ep_steps")) and (out["steps"] > 10).all()
    held = [env_bytes(env, e) for e in range(4)]
    again = env.rollout_each(pol, par, 100000)
    assert (again["steps"] == 0).all() and (again["first_stage_idx"] == -1).all()
    assert all(same_bytes(held[e], env_bytes(env, e)) == [] for e in range(4)), "an env that was over took part in a launch"
    # one env starts over, the others are over at entry
    env.reset(seed=[45, 0, 0, 0], mask=torch.tensor([1, 0, 0, 0], dtype=torch.uint8).to(env.device))
    mixed = env.rollout_each(pol, par, 7)
    assert mixed["steps"].tolist() == [7, 0, 0, 0] and env.header(0)["ep_steps"] == 7
    assert all(same_bytes(held[e], env_bytes(env, e)) == [] for e in (1, 2, 3))
    env.close()


# ---- 4. the pick kernel against the host's definition ------------------------------------------------

def host_pick(cost: np.ndarray, ok: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """cost f64[P, K, S], ok bool[P, K, S] -> (score f64[P, K], best i64[P]): Python's sum over the samples in order, one division, the
    first of the lowest scores, NaN (an unfinished sample) never"""
    P, K, S = cost.shape
    score = np.full((P, K), np.nan)
    best = np.full(P, -1, dtype=np.int64)
    for p in range(P):
        for k in range(K):
            if ok[p, k].all():
                score[p, k] = sum(float(x) for x in cost[p, k]) / S
        for k in range(K):
            if not np.isnan(score[p, k]) and (best[p] < 0 or score[p, k] < score[p, best[p]]):
                best[p] = k
    return score, best


def check_pick(samples: int, pack, device, lib) -> None:
    cands = [("fair", 0), ("fair", 0), ("fifo", 0)]  # a duplicate: the tie goes to the lower index
    P, K, S = 2, len(cands), samples
    B = P * (1 + K * S)
    env = VecSparkSchedSimEnv(TINY, B, device=device, pack=pack, _lib=lib)
    env.reset(seed=[0, 1] + [7] * (B - 2))
    lock_step(env, [0, 1], "fair", 0, 20)
    kids = np.arange(P, B).reshape(P, K, S)
    reseed = None if S == 1 else [500 + s for _ in range(P) for s in range(S)]  # (sample s: the same noise for every candidate)

    def play(p_list, k, max_steps):
        src = [p for p in p_list for _ in range(S)]
        dst = [int(kids[p, k, s]) for p in p_list for s in range(S)]
        rs = None if S == 1 else [500 + s for _ in p_list for s in range(S)]
        evaluation.continuations(env, src, dst, cands[k][0], cands[k][1], reseed=rs, max_steps=max_steps, check_every=16)

    for k in range(K):
        play([0, 1], k, 2000)
    cand = {"first_policy": i32(env, [10, 11, 12]), "first_param": i32(env, [20, 21, 22]), "policy": i32(env, [30, 31, 32]), "param": i32(env, [40, 41, 42])}

    def run_and_compare(what):
        stats = env.job_stats()["stats"].cpu().numpy()
        ok = ((env.header_field("terminated") != 0) & (env.header_field("err") == 0)).cpu().numpy()
        score, best = host_pick(stats[kids, 1], ok[kids])
        got_best = torch.full((P,), -9, dtype=torch.int32, device=env.device)
        got_score = torch.zeros((P, K), dtype=torch.float64, device=env.device)
        slots = {k: torch.full((B,), -7, dtype=torch.int32, device=env.device) for k in cand}
        held = [env_bytes(env, e) for e in range(B)]
        env.lookahead_pick(i32(env, [0, 1]), i32(env, kids.tolist()), cand, got_best, got_score, slots)
        assert all(same_bytes(held[e], env_bytes(env, e)) == [] for e in range(B)), "the pick kernel wrote to the arena"
        gs = got_score.cpu().numpy()
        nan = np.isnan(score)
        assert np.array_equal(np.isnan(gs), nan), (what, gs, score)
        assert np.array_equal(gs[~nan].view(np.uint64), score[~nan].view(np.uint64)), (what, gs, score)
        assert got_best.tolist() == best.tolist(), (what, got_best.tolist(), best.tolist())
        for name, t in slots.items():
            want = [-7] * B
            for p in range(P):
                want[p] = int(cand[name][max(int(best[p]), 0)])
            assert t.tolist() == want, (what, name)
        return score, best

    score, best = run_and_compare("all finished")
    assert not np.isnan(score).any() and (best != 1).all()  # (candidates 0 and 1 are the same policy on the same noise: never 1)
    assert np.array_equal(score[:, 0].view(np.uint64), score[:, 1].view(np.uint64))
    # parent 0: the winner's first sample starts over and is left unfinished after 3 steps - it is cheap (few jobs have arrived) and must not win
    w = int(best[0])
    dup = [k for k in range(K) if cands[k] == cands[w]]
    for k in dup:
        play([0], k, 3)
    score2, best2 = run_and_compare("one candidate unfinished")
    assert np.isnan(score2[0, dup]).all() and best2[0] not in dup and best2[0] >= 0 and best2[1] == best[1]
    for k in range(K):
        play([0], k, 3)
    score3, best3 = run_and_compare("every candidate unfinished")
    assert np.isnan(score3[0]).all() and best3[0] == -1 and best3[1] == best[1]
    env.close()


# ---- 5. the whole scheduler against a composition of the existing calls -----------------------------

def compose_lookahead(env, parents: list[int], kids: np.ndarray, candidates, seeds, max_decisions: int = 1000):
    """policy switching written with the API as it was before the scheduler: fork + lock-step continuations per candidate, job_stats,
    numpy's arg-min, policy_actions + step_async. Returns the winners per decision (list of lists, -2 for a parent that is over)"""
    B, P, K = env.num_envs, len(parents), len(candidates)
    per_env = [0] * B
    for i, p in enumerate(parents):
        per_env[p] = seeds[i]
    env.reset(seed=per_env)
    winners = []
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=env.device)
    for _ in range(max_decisions):
        live = [(env.obs_i32[p, 6] == 0).item() and (env.obs_i32[p, 7] == 0).item() for p in parents]
        if not any(live):
            break
        cost = np.full((P, K), np.nan)
        for k, (name, param) in enumerate(candidates):
            r = evaluation.continuations(env, parents, [int(c) for c in kids[:, k, 0]], name, param, max_steps=5000, check_every=16)
            c = r["total_job_time"].cpu().numpy()
            cost[:, k] = np.where(r["ok"].cpu().numpy(), c, np.nan)
        best = [int(np.nanargmin(cost[i])) for i in range(P)]
        si, ne = skip.clone(), torch.ones(B, dtype=torch.int32, device=env.device)
        for k, (name, param) in enumerate(candidates):
            a = env.policy_actions(name, param)
            for i, p in enumerate(parents):
                if live[i] and best[i] == k:
                    si[p], ne[p] = a["stage_idx"][p], a["num_exec"][p]
        env.step_async(si, ne)
        winners.append([best[i] if live[i] else -2 for i in range(P)])
    return winners


def check_scheduler_against_composition(seeds: list[int], pack, device, lib) -> None:
    P, K = len(seeds), len(CANDIDATES)
    B = P * (1 + K)
    parents = list(range(P))
    kids = np.arange(P, B).reshape(P, K, 1)
    env = VecSparkSchedSimEnv(TINY, B, device=device, pack=pack, _lib=lib)
    sched = LookaheadScheduler(env, parents, CANDIDATES)
    assert sched.children == kids.reshape(-1).tolist()
    r = evaluation.run_lookahead(env, sched, seeds, check_every=16)
    assert bool(r["ok"].all()) and r["fallbacks"] == 0 and sched.fallbacks == 0
    ref = VecSparkSchedSimEnv(TINY, B, device=device, pack=pack, _lib=lib)
    want = compose_lookahead(ref, parents, kids, CANDIDATES, seeds)
    got = r["winners"].cpu().numpy()
    for i in range(P):
        mine = [int(x) for x in got[: int(r["decisions"][i]), i]]
        theirs = [w[i] for w in want if w[i] != -2]
        assert mine == theirs, f"parent {i} (seed {seeds[i]}): the winners differ from decision {next((d for d, (a, b) in enumerate(zip(mine, theirs)) if a != b), min(len(mine), len(theirs)))} on"
        for a, b in zip(env.job_times(i)[:2], ref.job_times(i)[:2]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"parent {i}: job times differ"
        assert int(r["steps"][i]) == ref.header(i)["ep_steps"]
    env.close(), ref.close()


# ---- 6. the lookahead never ends above a candidate (deterministic children) --------------------------

def check_exact_improvement(pack, device, lib) -> None:
    seeds = [0, 1, 2]
    P, K = len(seeds), len(CANDIDATES)
    solo = VecSparkSchedSimEnv(TINY, P, device=device, pack=pack, _lib=lib)
    own = {}
    for name, param in CANDIDATES:
        r = evaluation.run_episodes(solo, name, seeds, param=param)
        assert bool(r["ok"].all()), f"{name}:{param} ended in an env error"
        own[(name, param)] = r["total_job_time"].cpu().numpy()
    solo.close()
    best_own = np.min(np.stack(list(own.values())), axis=0)
    env = VecSparkSchedSimEnv(TINY, P * (1 + K), device=device, pack=pack, _lib=lib)

    def run(**kw):
        r = evaluation.run_lookahead(env, LookaheadScheduler(env, list(range(P)), CANDIDATES, **kw), seeds, check_every=16)
        assert bool(r["ok"].all()) and r["fallbacks"] == 0, "a parent was left out"
        return r["total_job_time"].cpu().numpy(), r

    switching, r = run()
    print("own episodes:", {f"{n}:{p}": v.tolist() for (n, p), v in own.items()}, "switching:", switching.tolist())
    for c, v in own.items():
        assert (switching <= v).all(), (c, switching, v)
    assert (switching < best_own).any(), "policy switching never beat the best candidate: the check above shows nothing"
    w = r["winners"].cpu().numpy()
    for i in range(P):
        seq = w[: int(r["decisions"][i]), i]
        assert (np.diff(seq) != 0).sum() >= 1, f"parent {i} never changed its winner"
    over_fair, _ = run(base=("fair", 0))
    print("rollout algorithm over fair:", over_fair.tolist())
    assert (over_fair <= own[("fair", 0)]).all(), (over_fair, own[("fair", 0)])
    every4, _ = run(replan_every=4)
    print("replan_every=4:", every4.tolist())
    assert (every4 <= best_own).all(), (every4, best_own)
    env.close()


# ---- 7. continuations(fused=True) ---------------------------------------------------------------------

def check_fused_continuations(pack, device, lib) -> None:
    def prepared():
        env = VecSparkSchedSimEnv(TINY, 6, device=device, pack=pack, _lib=lib)
        env.reset(seed=[21, 22, 23, 24, 25, 26])
        for _ in range(12):
            step_envs(env, {}, policy_envs=(0, 5))
        for _ in range(5):
            step_envs(env, {}, policy_envs=(1, 2, 3, 4))
        return env

    a, b = prepared(), prepared()
    for policy, dst, seeds in (("fair", [1, 2], [101, 102]), ("fifo", [3, 4], [101, 102]), ("sjfcp", [1, 3], None)):
        others = [e for e in range(6) if e not in dst]
        held = {e: env_bytes(b, e) for e in others}
        ra = evaluation.continuations(a, [0, 0], dst, policy, reseed=seeds, max_steps=2000)
        rb = evaluation.continuations(b, [0, 0], dst, policy, reseed=seeds, max_steps=2000, fused=True)
        assert bool(rb["ok"].all()) and set(ra) == set(rb)
        for k in ra:
            x, y = ra[k].cpu().numpy(), rb[k].cpu().numpy()
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (policy, k)
        for e in others:
            assert same_bytes(held[e], env_bytes(b, e)) == [], f"env {e} took no part and changed"
        for e in dst:
            assert same_bytes(live_image(a, e), live_image(b, e)) == []
    a.close(), b.close()


# ---- 8. refusals, the caller's duties, the scheduler's arguments -------------------------------------

def check_refusals(pack, device, lib) -> None:
    import ctypes as C

    import pytest
    from spark_sched_sim_amd import binding as B

    env = VecSparkSchedSimEnv(TINY, 4, device=device, pack=pack, _lib=lib)
    env.reset(seed=[51, 52, 53, 54])
    L = env._b.lib
    for sym in ("sss_rollout_each", "sss_lookahead_pick"):
        assert sym in B.EXPORTS and hasattr(L, sym)
    pol, par = per_env(env, {0: ("fair", 0)})
    whole = env.state.cpu().numpy().copy()

    def refused(rc, message):
        assert rc != 0 and message in L.sss_last_error().decode(), (rc, L.sss_last_error().decode())

    refused(L.sss_rollout_each(env._h, None, par.data_ptr(), None, None, 5, None, None, None, None), "policy_dev is NULL")
    refused(L.sss_rollout_each(env._h, pol.data_ptr(), par.data_ptr(), None, None, -1, None, None, None, None), "n_steps must be >= 0")
    with pytest.raises(ValueError, match="n_steps must be >= 0"):
        env.rollout_each(pol, par, -1)
    env.enable_timeline(8)
    with pytest.raises(ValueError, match="not available while a timeline is recorded"):
        env.rollout_each(pol, par, 5)
    env.disable_timeline()
    with pytest.raises(ValueError, match="int32"):
        env.rollout_each(pol.long(), par, 5)
    with pytest.raises(ValueError, match="together"):
        env.rollout_each(pol, par, 5, first_policy=pol)
    refused(L.sss_lookahead_pick(env._h, 1, 0, 1, *([None] * 13)), "candidates and samples")
    refused(L.sss_lookahead_pick(env._h, 1, 64, 17, *([None] * 13)), "at most 1024")
    assert np.array_equal(env.state.cpu().numpy(), whole)
    # the arrays' contents are the caller's duty: the kernel skips such an env and says so
    bad_pol, bad_par = i32(env, [9, 3, 0, -5]), i32(env, [0, 7, 0, 0])
    out = env.rollout_each(bad_pol, bad_par, 5, i32(env, [-1, -1, 3, -1]), i32(env, [0, 0, -9, 0]))
    assert out["steps"].tolist() == [-1, -1, -1, -1] and np.array_equal(env.state.cpu().numpy(), whole)
    out = env.rollout_each(pol, par, 0)  # n_steps = 0
    assert out["steps"].tolist() == [0, 0, 0, 0] and np.array_equal(env.state.cpu().numpy(), whole)
    env.close()
    # the scheduler's arguments
    env = VecSparkSchedSimEnv(TINY, 10, device=device, pack=pack, _lib=lib)
    two = [("fair", 0), ("fifo", 0)]
    for kw, what in ((dict(parents=[0, 1, 2], candidates=CANDIDATES), "need 15 envs"), (dict(parents=[0], candidates=two, base=("sjfcp", 0)), "must be one of the candidates"),
                     (dict(parents=[0], candidates=two, children=[0, 1]), "disjoint"), (dict(parents=[0], candidates=two, children=[1, 1]), "distinct"),
                     (dict(parents=[0], candidates=two, children=[1]), "need 2 children"), (dict(parents=[8], candidates=two), "not enough env slots"),
                     (dict(parents=[0], candidates=[("wfair", 9)]), "alpha")):
        with pytest.raises(ValueError, match=what):
            LookaheadScheduler(env, **kw)
    sched = LookaheadScheduler(env, [0, 1], two, samples=2, reseed=12345, base=("fifo", 0))
    assert sched.children == list(range(2, 10))  # the ids behind the parents, [parent][candidate][sample]
    assert sched._cand["first_policy"].tolist() == [0, 1] and sched._cand["policy"].tolist() == [1, 1]
    env.close()


def check_reseeded_samples(pack, device, lib) -> None:
    """sample s of decision d is seeded by seed_for(s, d) for every candidate and parent: duplicate candidates get equal scores"""
    cands = [("sjfcp", 0), ("sjfcp", 0), ("fifo", 0)]
    P, K, S = 2, 3, 2
    env = VecSparkSchedSimEnv(TINY, P * (1 + K * S), device=device, pack=pack, _lib=lib)
    env.reset(seed=[3, 4] + [9] * (P * K * S))
    sched = LookaheadScheduler(env, [0, 1], cands, samples=S, reseed=2 ** 63 + 11)
    for d in range(3):
        sched.decide_and_step()
        want = [sched.seed_for(s, d) for _ in range(P * K) for s in range(S)]
        assert [int(x) % 2 ** 64 for x in sched._seeds.tolist()] == want
        sc = sched.last_scores.cpu().numpy()
        assert not np.isnan(sc).any() and np.array_equal(sc[:, 0].view(np.uint64), sc[:, 1].view(np.uint64))
        assert (sched.last_best != 1).all() and (sched.parent_out["steps"][:2] == 1).all()
    assert len({sched.seed_for(s, d) for s in range(S) for d in range(50)}) == 50 * S and sched.fallbacks == 0
    env.close()
