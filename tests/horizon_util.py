"""The checks of the lookahead with a time horizon and the two entry points under it (include/sss.h sss_rollout_until,
sss_lookahead_pick_horizon; VecSparkSchedSimEnv.rollout_until / lookahead_pick_horizon, lookahead.LookaheadScheduler with `horizon`,
evaluation.horizon_cost, evaluation.continuations with `horizon`), shared by tests/test_emu_horizon.py (the CPU wave emulator) and
tests/test_gpu_horizon.py (the kernels). Every check takes (device, lib): ("cpu", the emulator's library) or ("cuda:0", None). What
the new paths are held to is what was there before them - `rollout_each`, `policy_actions` + `step_async` with the wall time read on
the host, `schedulers.job_work`, `lookahead_pick` - and a restatement of the cost in Python floats, bit for bit. The seeds and horizons
were picked on the emulator so that the coverage guards hold; the guards are asserted, so no check passes without its branch."""
from __future__ import annotations

import math

import numpy as np
import torch

from fork_util import SKIP, TINY, env_bytes, same_bytes
from lookahead_util import CANDIDATES, EACH_POLICIES, cfg_of, host_pick, i32, live_image, lock_step, per_env
from spark_sched_sim_amd import VecSparkSchedSimEnv, evaluation, schedulers
from spark_sched_sim_amd.lookahead import LookaheadScheduler
from spark_sched_sim_amd.vec_env import HDR_OFF

INF = float("inf")
SEEDS = list(range(21, 29))
# (num_executors -> a horizon at which, from 5 fair steps into SEEDS, some envs stop on it and at least one ends its episode first)
MIXED_HORIZON = {5: 600000.0, 65: 170000.0}


def step_image(env, e: int) -> dict:
    """live_image for a comparison between one fused launch and lock step: without the header's n_batched and n_rounds. The two
    count which path of the event loop handled an event (sss_layout.h SssHdr), not what the event did, and with 65 executors they
    depend on where a launch begins - `rollout_each` against lock step shows the same two words, seed 26 of SEEDS for one"""
    b = live_image(env, e)
    b["state"][HDR_OFF["n_batched"]: HDR_OFF["n_rounds"] + 8] = 0
    return b


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def walls(env) -> np.ndarray:
    return env.header_field("wall_time").cpu().numpy().copy()


def over(env) -> np.ndarray:
    return ((env.header_field("terminated") != 0) | (env.header_field("need_reset") != 0)).cpu().numpy()


def lock_step_until(env, policy_of: dict[int, tuple[str, int]], T: dict[int, float], first: dict[int, tuple[str, int]] | None = None,
                    max_steps: int = 100000) -> tuple[dict[int, int], dict[int, float]]:
    """the stop time written with the calls that were there before it: env e takes policy_actions + step_async steps under
    policy_of[e] (its first under first[e]) for as long as its wall time, READ ON THE HOST, is < T[e] and its episode is not over;
    every other env sits the launches out. Returns (steps taken, the wall time before the last step) per env"""
    B, dev = env.num_envs, env.device
    taken = {e: 0 for e in policy_of}
    before = {e: math.nan for e in policy_of}
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=dev)
    while True:
        w, done = walls(env), over(env)
        live = [e for e in policy_of if not done[e] and w[e] < T[e] and taken[e] < max_steps]
        if not live:
            return taken, before
        now = {e: (first[e] if first and e in first and taken[e] == 0 else policy_of[e]) for e in live}
        si, ne = skip.clone(), torch.ones(B, dtype=torch.int32, device=dev)
        for name, param in sorted(set(now.values())):
            a = env.policy_actions(name, param)
            sel = torch.tensor([e for e in live if now[e] == (name, param)], dtype=torch.long).to(dev)
            si[sel], ne[sel] = a["stage_idx"][sel], a["num_exec"][sel]
        env.step_async(si, ne)
        for e in live:
            taken[e] += 1
            before[e] = float(w[e])


def prepared(num_executors: int, pack, device, lib):
    env = VecSparkSchedSimEnv(cfg_of(num_executors), 8, device=device, pack=pack, _lib=lib)
    env.reset(seed=SEEDS)
    env.rollout("fair", 5)
    return env


# ---- 1. horizon = inf is rollout_each ---------------------------------------------------------------------

def check_inf_equals_each(num_executors: int, pack, device, lib) -> None:
    a, b = prepared(num_executors, pack, device, lib), prepared(num_executors, pack, device, lib)
    pol, par = per_env(a, dict(enumerate(EACH_POLICIES)))  # (envs 6, 7: -1)
    fpol, fpar = per_env(a, {0: ("fifo", 0), 2: ("fair", 0)})
    for n in (7, 100000):  # a bound on the steps that binds, then the rest of the episodes
        ra = a.rollout_each(pol, par, n, fpol, fpar)
        rb = b.rollout_until(pol, par, INF, n, fpol, fpar)
        for k in ("steps", "first_stage_idx", "first_num_exec"):
            assert torch.equal(ra[k], rb[k]), (n, k, ra[k].tolist(), rb[k].tolist())
        for e in range(8):
            bad = same_bytes(live_image(a, e), live_image(b, e))  # (the arena block and every observation tensor of the env)
            assert bad == [], f"max_steps {n}, env {e}: {bad}"
        t = rb["t_stop"].cpu().numpy()
        assert np.isinf(t[:6]).all() and (t[:6] > 0).all() and (t[6:] == 0).all(), t
        if n == 7:
            assert (rb["steps"][:6] == 7).all() and (rb["rem_work"][:6] != 0).any()
    term = b.header_field("terminated").cpu().numpy() != 0
    assert over(b)[:6].all() and term[:5].all() and (rb["steps"][:6] > 10).all()  # (the hash policy may end in the reference's own stall: an env error)
    assert (rb["rem_work"][torch.from_numpy(term).to(b.device)] == 0).all(), "an env that terminated holds no work"
    # over at entry: no byte of the env moves, t_stop is written all the same, the row is zeroed
    held = [env_bytes(b, e) for e in range(8)]
    out = {k: torch.full_like(v, 5) for k, v in rb.items()}
    b.rollout_until(pol, par, 1000.0, 50, out=out)
    assert all(same_bytes(held[e], env_bytes(b, e)) == [] for e in range(8))
    assert out["steps"].tolist() == [0] * 6 + [5, 5] and (out["rem_work"][:6] == 0).all() and (out["rem_work"][6:] == 5).all()
    assert np.array_equal(bits(out["t_stop"].cpu().numpy()[:6]), bits(walls(b)[:6] + 1000.0)) and (out["t_stop"][6:] == 5).all()
    a.close(), b.close()


# ---- 2. a finite horizon is lock step with the wall time read on the host; 3. rem_work is schedulers.job_work ----------------

def active_ids(env, e: int) -> list[int]:
    """the arena's ordered active-job list of env e (u16 each at dims.off_active)"""
    n = env.header(e)["n_active"]
    raw = env._env_view[e, env.dims.off_active: env.dims.off_active + 2 * n].cpu().numpy()
    return raw.view(np.uint16).astype(int).tolist()


def check_finite_equals_lock_step(num_executors: int, pack, device, lib) -> None:
    H = MIXED_HORIZON[num_executors]
    a, b = prepared(num_executors, pack, device, lib), prepared(num_executors, pack, device, lib)
    policy_of = dict(enumerate(EACH_POLICIES))
    first = {0: ("fifo", 0), 2: ("fair", 0), 5: ("wfair", 2)}
    T = {e: float(np.float64(walls(a)[e]) + np.float64(H)) for e in policy_of}
    want_steps, before = lock_step_until(a, policy_of, T, first)
    pol, par = per_env(b, policy_of)
    fpol, fpar = per_env(b, first)
    held = {e: env_bytes(b, e) for e in (6, 7)}
    out = b.rollout_until(pol, par, H, 100000, fpol, fpar)
    for e in (6, 7):
        assert same_bytes(held[e], env_bytes(b, e)) == [], f"env {e} has policy -1 and changed"
    assert out["steps"].tolist() == [want_steps[e] for e in range(6)] + [0, 0]
    assert np.array_equal(bits(out["t_stop"].cpu().numpy()[:6]), bits([T[e] for e in range(6)])) and (out["t_stop"][6:] == 0).all()
    w, term = walls(b), over(b)  # (an env error ends an env as well: the hash policy may run into the reference's own stall)
    on_horizon = [e for e in range(6) if not term[e]]
    for e in range(6):
        bad = same_bytes(step_image(a, e), step_image(b, e))
        assert bad == [], f"env {e}: {bad}"
        assert before[e] < T[e] and (term[e] or w[e] >= T[e]), (e, before[e], w[e], T[e])
    assert on_horizon and any(b.header(e)["terminated"] and w[e] < T[e] for e in range(6)), "need an env that stops on the horizon and one that ends before it"
    assert all(w[e] >= T[e] for e in on_horizon)
    # 3. the remaining work of the state each env stopped in
    rem = out["rem_work"].cpu().numpy()
    assert rem.shape == (8, b.dims.job_cap) and (rem[6:] == 0).all()
    out_of_order = False
    for e in range(6):
        W = schedulers.job_work(b.obs_view(e))
        ids = active_ids(b, e)
        assert len(W) == len(ids) == b.header(e)["n_active"]
        want = np.zeros(b.dims.job_cap)
        want[ids] = W
        assert np.array_equal(bits(rem[e]), bits(want)), (e, rem[e].tolist(), want.tolist())
        by_id = [x for _, x in sorted(zip(ids, W))]
        out_of_order |= len(W) >= 2 and any(x > y for x, y in zip(by_id, by_id[1:]))
    assert out_of_order, "no env has two active jobs whose work is not ascending in id order: the pick's sort would show nothing"
    # max_steps = 0: nothing moves, the row is that of the state as it is
    whole = b.state.cpu().numpy().copy()
    again = b.rollout_until(pol, par, H, 0)
    assert again["steps"].tolist() == [0] * 8 and np.array_equal(b.state.cpu().numpy(), whole)
    assert np.array_equal(bits(again["rem_work"].cpu().numpy()), bits(rem))
    a.close(), b.close()


# ---- 4. the pick kernel against the host's definition ------------------------------------------------------------

def host_cost(env, c: int, T: float, rem: np.ndarray, tail: str) -> tuple[float, dict]:
    """(cost of child c, what the guards ask about it): include/sss.h sss_lookahead_pick_horizon restated with numpy reads and
    Python floats; NaN for an invalid child"""
    h = env.header(c)
    ta, tc = env.job_times(c)[:2]
    n, w, term = min(max(h["next_arrival"], 0), env.dims.job_cap), float(h["wall_time"]), h["terminated"] != 0
    info = {"excluded": sum(1 for j in range(n) if not float(ta[j]) < T), "open_work": False, "valid": h["err"] == 0 and (term or w >= T)}
    if not info["valid"]:
        return math.nan, info
    counted = [j for j in range(n) if float(ta[j]) < T]
    upto = w if tail == "srpt" else min(T, w)
    cost = 0.0
    for j in counted:
        cost = cost + (min(float(tc[j]), upto) - float(ta[j]))
    if tail == "srpt" and not term:
        left = sorted(float(rem[j]) for j in counted if float(tc[j]) > w)
        info["open_work"] = any(x > 0 for x in left)
        p, rest = 0.0, 0.0
        for x in left:
            p = p + x
            rest = rest + p / float(env.num_executors)
        cost = cost + rest
    assert bits(cost) == bits(evaluation.horizon_cost(ta[:n], tc[:n], w, T, rem, env.num_executors, term, tail)) or math.isnan(cost)
    return cost, info


def check_pick(samples: int, H: float, pack, device, lib) -> None:
    cands = [("fair", 0), ("fair", 0), ("fifo", 0)]  # a duplicate: the tie goes to the lower index
    P, K, S = 2, len(cands), samples
    B = P * (1 + K * S)
    env = VecSparkSchedSimEnv(TINY, B, device=device, pack=pack, _lib=lib)
    env.reset(seed=[0, 1] + [7] * (B - 2))
    lock_step(env, [0, 1], "fair", 0, 6)  # (early in the episodes: jobs still arrive, and a child's last step can carry it past an arrival)
    kids = np.arange(P, B).reshape(P, K, S)
    out = None

    def play(p_list, k_list, max_steps):
        nonlocal out
        pairs = [(p, k, s) for p in p_list for k in k_list for s in range(S)]
        env.fork([p for p, _, _ in pairs], [int(kids[p, k, s]) for p, k, s in pairs], reseed=None if S == 1 else [500 + s for _, _, s in pairs])
        pol, par = per_env(env, {int(kids[p, k, s]): cands[k] for p, k, s in pairs})
        out = env.rollout_until(pol, par, H, max_steps, out=out)

    play([0, 1], range(K), 100000)
    cand = {"first_policy": i32(env, [10, 11, 12]), "first_param": i32(env, [20, 21, 22]), "policy": i32(env, [30, 31, 32]), "param": i32(env, [40, 41, 42])}
    seen = {"excluded": False, "open_work": False}

    def run_and_compare(what, tail):
        t_stop, rem = out["t_stop"].cpu().numpy(), out["rem_work"].cpu().numpy()
        cost, ok = np.zeros((P, K, S)), np.zeros((P, K, S), dtype=bool)
        for p, k, s in np.ndindex(P, K, S):
            c = int(kids[p, k, s])
            cost[p, k, s], info = host_cost(env, c, float(t_stop[c]), rem[c], tail)
            ok[p, k, s] = info["valid"]
            seen["excluded"] |= info["valid"] and info["excluded"] > 0
            seen["open_work"] |= info["open_work"]
        score, best = host_pick(cost, ok)
        got_best = torch.full((P,), -9, dtype=torch.int32, device=env.device)
        got_score = torch.zeros((P, K), dtype=torch.float64, device=env.device)
        slots = {k: torch.full((B,), -7, dtype=torch.int32, device=env.device) for k in cand}
        held = [env_bytes(env, e) for e in range(B)]
        env.lookahead_pick_horizon(i32(env, [0, 1]), i32(env, kids.tolist()), cand, out["t_stop"], out["rem_work"], tail, got_best, got_score, slots)
        assert all(same_bytes(held[e], env_bytes(env, e)) == [] for e in range(B)), "the pick kernel wrote to the arena"
        gs = got_score.cpu().numpy()
        nan = np.isnan(score)
        assert np.array_equal(np.isnan(gs), nan), (what, tail, gs, score)
        assert np.array_equal(bits(gs[~nan]), bits(score[~nan])), (what, tail, gs, score)
        assert got_best.tolist() == best.tolist(), (what, tail, got_best.tolist(), best.tolist())
        for name, t in slots.items():
            want = [-7] * B
            for p in range(P):
                want[p] = int(cand[name][max(int(best[p]), 0)])
            assert t.tolist() == want, (what, tail, name)
        return score, best

    first = {}
    for tail in ("none", "srpt"):
        score, best = first[tail] = run_and_compare("all at their horizon", tail)
        assert not np.isnan(score).any() and (best != 1).all()  # (candidates 0 and 1 are the same policy on the same noise: never 1)
        assert np.array_equal(bits(score[:, 0]), bits(score[:, 1]))
    t_stop = out["t_stop"].cpu().numpy()
    assert len({t_stop[int(c)] for c in kids[0].reshape(-1)}) == 1, "the children of a parent share their stop time"
    assert not env.header_field("terminated")[P:].bool().all(), "every child ended its episode: the horizon shows nothing"
    assert seen["excluded"], "no child overshot its horizon past an arrival: `t_arrival < T` excluded nothing"
    assert seen["open_work"], "no child holds an unfinished counted job with work left: the srpt tail added nothing"
    # parent 0: the winner's children start over and are cut by max_steps before their horizon - cheap (little time has passed), must not win
    for tail in ("none", "srpt"):
        score, best = first[tail]
        dup = [k for k in range(K) if cands[k] == cands[int(best[0])]]
        play([0], dup, 3)
        c = int(kids[0, dup[0], 0])
        assert env.header(c)["terminated"] == 0 and env.header(c)["wall_time"] < float(out["t_stop"][c])
        score2, best2 = run_and_compare("one candidate cut short", tail)
        assert np.isnan(score2[0, dup]).all() and best2[0] not in dup and best2[0] >= 0 and best2[1] == best[1]
        play([0], range(K), 3)
        score3, best3 = run_and_compare("every candidate cut short", tail)
        assert np.isnan(score3[0]).all() and best3[0] == -1 and best3[1] == best[1]
        play([0], range(K), 100000)
    env.close()


# ---- 5. the scheduler: horizon = inf is horizon = None; 7. a finite horizon takes fewer child steps --------------------------

def run_scheduler(env, sched, seeds, warm: int = 0, max_decisions: int = 2000) -> dict:
    """the parents of `sched` play one episode (reset as evaluation.run_lookahead resets), its first `warm` steps under the fair
    policy and the rest under the scheduler (a decision costs its children's steps: the emulator starts late in the episode); per
    decision: the winners of the parents that were not over, the scores' bits, and the steps its children took"""
    P = len(sched.parents)
    per, mask = [0] * env.num_envs, [0] * env.num_envs
    for i, p in enumerate(sched.parents):
        for e in [p] + sched.children[i * (len(sched.children) // P): (i + 1) * (len(sched.children) // P)]:
            per[e], mask[e] = seeds[i], 1
    env.reset(seed=per, mask=torch.tensor(mask, dtype=torch.uint8).to(env.device))
    sched.reset()
    if warm:
        env.rollout_each(*per_env(env, {p: ("fair", 0) for p in sched.parents}), warm)
    log = {"winners": [], "scores": [], "child_steps": [], "longest": 0}
    kids = torch.tensor(sched.children, dtype=torch.long).to(env.device)
    for _ in range(max_decisions):
        live = ~over(env)[sched.parents]
        if not live.any():
            break
        sched.decide_and_step()
        best = sched.last_best.cpu().numpy()
        log["winners"].append([int(best[i]) if live[i] else -2 for i in range(P)])
        log["scores"].append(bits(sched.last_scores.cpu().numpy())[live].copy())
        steps = sched.child_out["steps"][kids].cpu().numpy().reshape(P, -1)[live]
        assert (steps >= 0).all()
        log["child_steps"].append(int(steps.sum()))
        log["longest"] = max(log["longest"], int(steps.max()))
    assert over(env)[sched.parents].all() and (env.header_field("err")[sched.parents] == 0).all()
    return log


def check_scheduler_inf_equals_none(seeds: list[int], warm: int, pack, device, lib) -> None:
    P, K = len(seeds), len(CANDIDATES)
    envs = [VecSparkSchedSimEnv(TINY, P * (1 + K), device=device, pack=pack, _lib=lib) for _ in range(3)]
    parents = list(range(P))
    ref = run_scheduler(envs[0], LookaheadScheduler(envs[0], parents, CANDIDATES), seeds, warm)
    assert len(ref["winners"]) > 10 and len({w[i] for w in ref["winners"] for i in range(P)} - {-2}) > 1
    for env, tail in zip(envs[1:], ("srpt", "none")):
        got = run_scheduler(env, LookaheadScheduler(env, parents, CANDIDATES, horizon=INF, tail=tail), seeds, warm)
        assert got["winners"] == ref["winners"], tail
        assert all(np.array_equal(x, y) for x, y in zip(got["scores"], ref["scores"])), tail
        assert got["child_steps"] == ref["child_steps"]
        for p in range(P):
            assert same_bytes(live_image(envs[0], p), live_image(env, p)) == [], (tail, p)
    for env in envs:
        env.close()


# ---- 6. the scheduler with a finite horizon against a composition of the calls that were there before ---------------------

def compose_horizon(env, parents: list[int], kids: np.ndarray, candidates, seeds, H: float, tail: str, max_decisions: int = 2000) -> list[list[int]]:
    """policy switching with a horizon written without the new entry points: fork, lock-step children that the host stops by their
    wall time, the host's cost, numpy's arg-min, policy_actions + step_async for the parent. Winners per decision (-2: parent over)"""
    B, P, K = env.num_envs, len(parents), len(candidates)
    per = [0] * B
    for i, p in enumerate(parents):
        per[p] = seeds[i]
    env.reset(seed=per)
    winners = []
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=env.device)
    for _ in range(max_decisions):
        live = ~over(env)[parents]
        if not live.any():
            break
        w = walls(env)
        pairs = [(i, k) for i in range(P) for k in range(K)]
        env.fork([parents[i] for i, _ in pairs], [int(kids[i, k, 0]) for i, k in pairs])
        T = {int(kids[i, k, 0]): float(np.float64(w[parents[i]]) + np.float64(H)) for i, k in pairs}
        lock_step_until(env, {int(kids[i, k, 0]): candidates[k] for i, k in pairs}, T)
        cost = np.full((P, K), np.nan)
        for i, k in pairs:
            c = int(kids[i, k, 0])
            W = schedulers.job_work(env.obs_view(c))
            rem = np.zeros(env.dims.job_cap)
            rem[active_ids(env, c)] = W
            cost[i, k], info = host_cost(env, c, T[c], rem, tail)
            assert info["valid"]
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


def check_scheduler_against_composition(seeds: list[int], H: float, tail: str, pack, device, lib) -> None:
    P, K = len(seeds), len(CANDIDATES)
    B = P * (1 + K)
    parents, kids = list(range(P)), np.arange(P, B).reshape(P, K, 1)
    env = VecSparkSchedSimEnv(TINY, B, device=device, pack=pack, _lib=lib)
    got = run_scheduler(env, LookaheadScheduler(env, parents, CANDIDATES, horizon=H, tail=tail), seeds)
    ref = VecSparkSchedSimEnv(TINY, B, device=device, pack=pack, _lib=lib)
    want = compose_horizon(ref, parents, kids, CANDIDATES, seeds, H, tail)
    for i in range(P):
        mine, theirs = [w[i] for w in got["winners"] if w[i] != -2], [w[i] for w in want if w[i] != -2]
        assert mine == theirs, f"parent {i} (seed {seeds[i]}): the winners differ from decision {next((d for d, (a, b) in enumerate(zip(mine, theirs)) if a != b), min(len(mine), len(theirs)))} on"
        assert len(set(mine)) > 1, f"parent {i} never changed its winner"
        assert same_bytes(step_image(env, i), step_image(ref, i)) == [], f"parent {i}: final bytes differ"
    env.close(), ref.close()


# ---- 7. the point of it: fewer child steps ------------------------------------------------------------------------

def check_fewer_child_steps(seeds: list[int], H: float, warm: int, pack, device, lib) -> None:
    K, parents = len(CANDIDATES), list(range(len(seeds)))
    env = VecSparkSchedSimEnv(TINY, len(seeds) * (1 + K), device=device, pack=pack, _lib=lib)
    full = run_scheduler(env, LookaheadScheduler(env, parents, CANDIDATES), seeds, warm)
    for tail in ("srpt", "none"):
        cut = run_scheduler(env, LookaheadScheduler(env, parents, CANDIDATES, horizon=H, tail=tail), seeds, warm)
        print(f"child steps per episode: horizon None {sum(full['child_steps'])} (longest {full['longest']}), {H:g} / {tail} {sum(cut['child_steps'])} (longest {cut['longest']})")
        assert sum(cut["child_steps"]) < sum(full["child_steps"]) and cut["longest"] < full["longest"]
    env.close()


# ---- 8. reseeded samples with a horizon ----------------------------------------------------------------------------

def check_reseeded_samples(H: float, pack, device, lib) -> None:
    cands = [("sjfcp", 0), ("sjfcp", 0), ("fifo", 0)]
    P, K, S = 2, 3, 2
    env = VecSparkSchedSimEnv(TINY, P * (1 + K * S), device=device, pack=pack, _lib=lib)
    for tail in ("srpt", "none"):
        env.reset(seed=[3, 4] + [9] * (P * K * S))
        sched = LookaheadScheduler(env, [0, 1], cands, samples=S, reseed=2 ** 63 + 11, horizon=H, tail=tail)
        for d in range(3):
            sched.decide_and_step()
            assert [int(x) % 2 ** 64 for x in sched._seeds.tolist()] == [sched.seed_for(s, d) for _ in range(P * K) for s in range(S)]
            sc = sched.last_scores.cpu().numpy()
            assert not np.isnan(sc).any() and np.array_equal(bits(sc[:, 0]), bits(sc[:, 1]))
            assert (sched.last_best != 1).all() and (sched.parent_out["steps"][:2] == 1).all()
            kids = sched.child_out["t_stop"][2:].cpu().numpy().reshape(P, K * S)
            assert (kids == kids[:, :1]).all() and not (env.header_field("terminated")[2:] != 0).all()
        assert sched.fallbacks == 0
    env.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------

def check_refusals(pack, device, lib) -> None:
    import os.path as osp

    import pytest
    from spark_sched_sim_amd import binding as Bd

    env = VecSparkSchedSimEnv(TINY, 4, device=device, pack=pack, _lib=lib)
    env.reset(seed=[51, 52, 53, 54])
    L = env._b.lib
    header = open(osp.join(osp.dirname(osp.dirname(osp.abspath(__file__))), "include", "sss.h")).read()
    for sym in ("sss_rollout_until", "sss_lookahead_pick_horizon"):
        assert sym in Bd.EXPORTS and hasattr(L, sym) and f"int {sym}(sss_handle* h" in header
    pol, par = per_env(env, {0: ("fair", 0)})
    t_stop = torch.zeros(4, dtype=torch.float64, device=env.device)
    whole = env.state.cpu().numpy().copy()

    def refused(rc, message):
        assert rc != 0 and message in L.sss_last_error().decode(), (rc, L.sss_last_error().decode())

    P, N, T = pol.data_ptr(), None, t_stop.data_ptr()
    refused(L.sss_rollout_until(env._h, N, par.data_ptr(), N, N, 5.0, 5, N, N, N, T, N, N), "policy_dev is NULL")
    refused(L.sss_rollout_until(env._h, P, N, N, N, 5.0, 5, N, N, N, T, N, N), "param_dev is NULL")
    refused(L.sss_rollout_until(env._h, P, par.data_ptr(), N, N, 5.0, 5, N, N, N, N, N, N), "t_stop_dev is NULL")
    refused(L.sss_rollout_until(env._h, P, par.data_ptr(), P, N, 5.0, 5, N, N, N, T, N, N), "together")
    for h in (0.0, -1.0, float("nan"), -INF):
        refused(L.sss_rollout_until(env._h, P, par.data_ptr(), N, N, h, 5, N, N, N, T, N, N), "horizon must be > 0")
        with pytest.raises(ValueError, match="horizon must be > 0"):
            env.rollout_until(pol, par, h, 5)
        with pytest.raises(ValueError, match="horizon must be > 0"):
            LookaheadScheduler(env, [0], [("fair", 0), ("fifo", 0)], horizon=h)
    refused(L.sss_rollout_until(env._h, P, par.data_ptr(), N, N, 5.0, -1, N, N, N, T, N, N), "max_steps must be >= 0")
    with pytest.raises(ValueError, match="max_steps must be >= 0"):
        env.rollout_until(pol, par, 5.0, -1)
    with pytest.raises(ValueError, match="int32"):
        env.rollout_until(pol.long(), par, 5.0, 5)
    with pytest.raises(ValueError, match="together"):
        env.rollout_until(pol, par, 5.0, 5, first_policy=pol)
    with pytest.raises(ValueError, match="float64"):
        env.rollout_until(pol, par, 5.0, 5, out={"steps": pol.clone(), "first_stage_idx": pol.clone(), "first_num_exec": pol.clone(),
                                                "t_stop": t_stop.float(), "rem_work": torch.zeros((4, env.dims.job_cap), dtype=torch.float64, device=env.device)})
    env.enable_timeline(8)
    with pytest.raises(ValueError, match="not available while a timeline is recorded"):
        env.rollout_until(pol, par, 5.0, 5)
    env.disable_timeline()
    refused(L.sss_lookahead_pick_horizon(env._h, 1, 0, 1, *([None] * 8), 1, *([None] * 7)), "candidates and samples")
    refused(L.sss_lookahead_pick_horizon(env._h, 1, 64, 17, *([None] * 8), 0, *([None] * 7)), "at most 1024")
    refused(L.sss_lookahead_pick_horizon(env._h, 1, 1, 1, *([None] * 8), 2, *([None] * 7)), "tail must be 0 (none) or 1 (srpt)")
    one = {k: torch.zeros(1, dtype=torch.int32, device=env.device) for k in ("first_policy", "first_param", "policy", "param")}
    slots = {k: torch.zeros(4, dtype=torch.int32, device=env.device) for k in one}
    ids, best, score = i32(env, [0]), i32(env, [0]), torch.zeros((1, 1), dtype=torch.float64, device=env.device)
    rem = torch.zeros((4, env.dims.job_cap), dtype=torch.float64, device=env.device)
    refused(L.sss_lookahead_pick_horizon(env._h, 1, 1, 1, ids.data_ptr(), ids.data_ptr(), *(one[k].data_ptr() for k in one), None, rem.data_ptr(), 1,
                                         best.data_ptr(), score.data_ptr(), *(slots[k].data_ptr() for k in slots), None), "t_stop_dev is NULL")
    refused(L.sss_lookahead_pick_horizon(env._h, 1, 1, 1, ids.data_ptr(), ids.data_ptr(), *(one[k].data_ptr() for k in one), T, None, 1,
                                         best.data_ptr(), score.data_ptr(), *(slots[k].data_ptr() for k in slots), None), "rem_work_dev is NULL")
    with pytest.raises(ValueError, match="tail must be one of"):
        env.lookahead_pick_horizon(ids, ids.reshape(1, 1, 1), one, t_stop, rem, "fifo", best, score, slots)
    with pytest.raises(ValueError, match="rem_work must be a contiguous"):
        env.lookahead_pick_horizon(ids, ids.reshape(1, 1, 1), one, t_stop, rem[:2], "srpt", best, score, slots)
    with pytest.raises(ValueError, match="tail must be one of"):
        LookaheadScheduler(env, [0], [("fair", 0), ("fifo", 0)], horizon=5.0, tail="fifo")
    with pytest.raises(ValueError, match="needs fused=True"):
        evaluation.continuations(env, [0], [1], "fair", horizon=5.0)
    assert np.array_equal(env.state.cpu().numpy(), whole)
    # the arrays' contents are the caller's duty: the kernel skips such an env and says so; nothing else of it is written
    out = env.rollout_until(i32(env, [9, 3, 0, -5]), i32(env, [0, 7, 0, 0]), 5.0, 5, i32(env, [-1, -1, 3, -1]), i32(env, [0, 0, -9, 0]))
    assert out["steps"].tolist() == [-1, -1, -1, -1] and (out["t_stop"] == 0).all() and np.array_equal(env.state.cpu().numpy(), whole)
    # the scheduler's arguments reach the launches; continuations hands the children's costs on
    sched = LookaheadScheduler(env, [0], [("fair", 0), ("fifo", 0)], horizon=INF, tail="none")
    assert sched.horizon == INF and sched.tail == "none" and sched.child_out["rem_work"].shape == (4, env.dims.job_cap)
    assert LookaheadScheduler(env, [0], [("fair", 0), ("fifo", 0)]).horizon is None
    r = evaluation.continuations(env, [0, 0], [2, 3], "sjfcp", fused=True, horizon=40000.0, tail="srpt")
    for n, c in enumerate((2, 3)):
        want, info = host_cost(env, c, float(r["t_stop"][n]), r["rem_work"][n].cpu().numpy(), "srpt")
        assert info["valid"] and bits(want) == bits(float(r["horizon_cost"][n])) and r["t_stop"][n] == env.header(0)["wall_time"] + 40000.0
    env.close()
