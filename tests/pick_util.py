"""The two pick kernels of the lookahead (csrc/sss_lookahead.h: sss_lookahead_pick_kernel, sss_lookahead_pick_horizon_kernel) and the
rem_work rows they sort (csrc/sss_sim_until.h until_rem_work) at the sizes where their lanes stride: K x S up to the 1024 entries of
the LDS cost table, job counts up to the 1024 sort keys, more than two strides of active jobs. Shared by tests/test_emu_pick.py (the
emulator's library: the plain-loop form of the picks, until_rem_work lane by lane) and tests/test_gpu_pick.py (the gfx950 kernels).
Every check takes (device, lib): ("cpu", the emulator's library) or ("cuda:0", None). Everything is compared bit for bit, NaN
matching NaN - the order of every sum is the definition (include/sss.h): `evaluation.horizon_cost` in Python floats,
`lookahead_util.host_pick`, and for the plain pick Python's sum of min(t_completed, wall) - t_arrival in job-id order, which is also
column 1 of `env.job_stats()`. The crafted blocks follow jobstats_util.check_crafted; the coverage guards are asserted, so no check
passes without its branch. Each check returns what it saw (shapes, guard values) for the caller to print."""
from __future__ import annotations

import math

import numpy as np
import torch

import horizon_util as HU
from jobstats_util import pattern, same_bits, write_block
from lookahead_util import EACH_POLICIES, host_pick, i32, per_env
from spark_sched_sim_amd import VecSparkSchedSimEnv, evaluation, schedulers
from spark_sched_sim_amd.vec_env import HDR_OFF

INF = float("inf")
CAP = 1024
CRAFTED_N = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 512, 513, 1023, 1024)  # the lanes' strides and the sort's powers of two
REM_PATTERNS = ("wide", "duplicates", "equal", "descending")
SHAPES = ((1, 1), (3, 1), (63, 1), (64, 1), (65, 1), (1024, 1), (1, 1024), (128, 8), (65, 15), (7, 146))  # (K, S)
N_PARENTS = (1, 3)
K_MAX = max(K for K, _ in SHAPES)
TIED = (3, 67, 131)  # candidates in three different 64-strides
KEYS = ("first_policy", "first_param", "policy", "param")
GUARD_I32, GUARD_F64, N_GUARD = -9, -1.2345e300, 4
DENSE = dict(job_arrival_cap=200, job_arrival_rate=1.0e-3, moving_delay=1500.0, warmup_delay=500.0)
DENSE_SEEDS = list(range(31, 37))
DENSE_HORIZON = 400000.0
CHILD_HORIZON = 50000.0  # the children of the dense parents: a few steps each, no job completes them all


# ---- 1. crafted arena blocks ---------------------------------------------------------------------------------------------------

def general_times(n: int, rng) -> tuple[np.ndarray, np.ndarray, float]:
    """arrival times, completed and running jobs, a wall time inside the run (jobstats_util's "general" block, 40 % unfinished)"""
    ta = np.sort(rng.uniform(0.0, 4e6, n))
    tc = ta + 10.0 ** rng.uniform(2.0, 6.5, n)
    tc[rng.random(n) < 0.4] = np.inf
    return ta, tc, (float(ta[-1] + 1e5) if n else 1e5)


def crafted_blocks(rng) -> list[dict]:
    """one dict per env: n, ta, tc, wall, T (its t_stop), rem (its rem_work row, full width), terminated, err, what"""
    blocks = []
    for i, n in enumerate(CRAFTED_N):
        ta, tc, wall = general_times(n, rng)
        # T on the wall time, or on the arrival of a job in the last tenth: that job and those behind it have t_arrival >= T
        T = wall if i % 2 == 0 or n < 2 else float(ta[n - max(1, n // 10)])
        blocks.append(dict(n=n, ta=ta, tc=tc, wall=wall, T=T, rem=pattern(REM_PATTERNS[i % 4], CAP, rng), terminated=0, err=0, what=f"n={n}"))

    def special(n, what, rem="wide", **kw):
        ta, tc, wall = general_times(n, rng)
        b = dict(n=n, ta=ta, tc=tc, wall=wall, T=wall, rem=pattern(rem, CAP, rng), terminated=0, err=0, what=what)
        b.update(kw)
        blocks.append(b)
        return b

    special(300, "err")["err"] = 3
    b = special(129, "terminated before T", terminated=1)
    b["T"] = b["wall"] + 5e4
    b = special(65, "cut short of T")
    b["T"] = b["wall"] + 5e4
    b = special(65, "every counted job completed", rem="duplicates")
    b["tc"] = np.minimum(b["ta"] + 10.0 ** rng.uniform(2.0, 4.0, 65), b["wall"])
    special(1024, "every job unfinished, no padding key")["tc"] = np.full(1024, np.inf)
    special(513, "every job unfinished, mostly padding keys")["tc"] = np.full(513, np.inf)
    return blocks


def put_header(env, i: int, name: str, value: int) -> None:
    b = torch.from_numpy(np.array([value], np.int32).view(np.uint8).copy()).to(env.device)
    env._env_view[i, HDR_OFF[name]: HDR_OFF[name] + 4] = b


def write_blocks(env, blocks: list[dict]) -> None:
    for i, b in enumerate(blocks):
        write_block(env, i, b["ta"], b["tc"], b["wall"])
        put_header(env, i, "terminated", b["terminated"])
        put_header(env, i, "err", b["err"])


def plain_cost(b: dict) -> float:
    """Python's sum of the job durations in id order (metrics.job_durations): column 1 of sss_job_stats and the plain pick's cost"""
    total = 0.0
    for j in range(b["n"]):
        total = total + (min(float(b["tc"][j]), b["wall"]) - float(b["ta"][j]))
    return total


def block_costs(blocks: list[dict], mode: str, T_of, num_executors: int) -> tuple[np.ndarray, np.ndarray]:
    """(cost f64[B], valid bool[B]) of every block under `mode`: "plain", "none" or "srpt" (the horizon pick's tails, T_of(b) its T)"""
    cost, valid = np.full(len(blocks), np.nan), np.zeros(len(blocks), dtype=bool)
    for e, b in enumerate(blocks):
        if mode == "plain":
            valid[e] = b["terminated"] != 0 and b["err"] == 0
            cost[e] = plain_cost(b) if valid[e] else math.nan
        else:
            T = T_of(b)
            valid[e] = b["err"] == 0 and (b["terminated"] != 0 or b["wall"] >= T)
            cost[e] = evaluation.horizon_cost(b["ta"], b["tc"], b["wall"], T, b["rem"], num_executors, b["terminated"] != 0, mode) if valid[e] else math.nan
        assert valid[e] == (not math.isnan(cost[e])), (mode, b["what"])
    return cost, valid


def sorted_works(b: dict) -> list[float]:
    """the works the srpt tail of block b sorts (none if it is terminated)"""
    if b["terminated"]:
        return []
    return [float(b["rem"][j]) for j in range(b["n"]) if float(b["ta"][j]) < b["T"] and float(b["tc"][j]) > b["wall"]]


def child_tables(rng, K: int, S: int, roles: list[str], cost: np.ndarray, valid: np.ndarray, blocks: list[dict], outside: list[int]) -> np.ndarray:
    """i32[P, K, S] env ids, parent i by roles[i]:
    "tie"     the candidates of TIED below K all play the cheapest valid block with a job, every other candidate dearer blocks
              only: the lowest score is shared across the strides; a few other candidates hold an invalid child
    "mixed"   children from the valid blocks, a few percent of the candidates with an invalid block or an id outside the arena
    "none"    every candidate holds an invalid child, some nothing else"""
    B = len(blocks)
    ok = [e for e in range(B) if valid[e]]
    bad = [e for e in range(B) if not valid[e]] + outside
    tab = np.zeros((len(roles), K, S), dtype=np.int64)
    for i, role in enumerate(roles):
        tied = [k for k in TIED if k < K] if role == "tie" else []
        tied = tied if len(tied) >= 2 else []
        pool = ok
        if tied:
            cheapest = min((e for e in ok if blocks[e]["n"] >= 1), key=lambda e: cost[e])
            pool = [e for e in ok if cost[e] > cost[cheapest]]
        tab[i] = rng.choice(pool, size=(K, S))
        for k in tied:
            tab[i, k] = cheapest
        if role == "none":
            spoiled = list(range(K))
        else:
            free = [k for k in range(K) if k not in tied]
            spoiled = list(rng.choice(free, size=0 if K == 1 else max(1, round(0.03 * K)), replace=False))
        for n, k in enumerate(spoiled):
            hit = range(S) if role == "none" and n % 5 == 0 else rng.choice(S, size=min(S, 1 + int(rng.integers(0, 3))), replace=False)
            for s in hit:
                tab[i, k, s] = bad[int(rng.integers(0, len(bad)))]
    return tab


def check_crafted(which: str, pack, device, lib) -> dict:
    """which = "horizon": the horizon pick under both tails on blocks that stopped at or behind their T (or did not);
    which = "plain": the plain pick on the same blocks marked terminated, and the horizon pick with T = +inf against it"""
    rng = np.random.default_rng(29)
    blocks = crafted_blocks(rng)
    B = len(blocks)
    env = VecSparkSchedSimEnv({**DENSE, "num_executors": 10, "job_arrival_cap": CAP}, B, device=device, pack=pack, _lib=lib)
    assert env.dims.job_cap == CAP and B <= 20
    if which == "plain":
        for b in blocks:
            b["terminated"] = 0 if b["what"] == "cut short of T" else 1
    write_blocks(env, blocks)
    dev, N = env.device, env.num_executors
    rem = torch.from_numpy(np.stack([b["rem"] for b in blocks])).to(dev)
    assert rem.shape == (B, CAP)
    outside = [-1, B, B + 7, 2 ** 31 - 1, -2 ** 31]
    cand_host = {name: np.arange(K_MAX) + 1000 * (2 * n + 1) for n, name in enumerate(KEYS)}  # distinct values over the four tables
    seen = dict(launches=0, scores=0, nan=0, valid=0, nan_and_valid=0, ties=0, all_invalid=0, outside_parents=0, outside_ids=set(), excluded=0,
                m_max=0, m_distinct=0, m_duplicates=0, shapes=[])
    works_of = [sorted_works(b) for b in blocks]
    m_of = [len(w) for w in works_of]
    excluded_of = [sum(1 for j in range(b["n"]) if not float(b["ta"][j]) < b["T"]) for b in blocks]

    if which == "horizon":
        t_stop = torch.tensor([b["T"] for b in blocks], dtype=torch.float64).to(dev)
        modes = [(tail, t_stop, block_costs(blocks, tail, lambda b: b["T"], N)) for tail in ("none", "srpt")]
        assert [b["what"] for e, b in enumerate(blocks) if not modes[0][2][1][e]] == ["err", "cut short of T"]
        named = {b["what"]: e for e, b in enumerate(blocks)}
        assert m_of[named["every counted job completed"]] == 0 and blocks[named["every counted job completed"]]["n"] == 65
        assert m_of[named["every job unfinished, no padding key"]] == 1024 and m_of[named["every job unfinished, mostly padding keys"]] == 513
        assert m_of[named["terminated before T"]] == 0 and any(float(x) > blocks[named["terminated before T"]]["wall"] for x in blocks[named["terminated before T"]]["tc"])
    else:
        t_inf = torch.full((B,), INF, dtype=torch.float64, device=dev)
        plain = block_costs(blocks, "plain", None, N)
        stats = env.job_stats()["stats"].cpu().numpy()
        for e, b in enumerate(blocks):  # the header's promise: the plain pick's cost carries the bits of sss_job_stats' column 1
            assert same_bits(stats[e, 1], plain_cost(b)), (b["what"], stats[e, 1], plain_cost(b))
        for tail in ("none", "srpt"):  # ... and with T = +inf the definition of the horizon cost is that of the plain one
            assert same_bits(block_costs(blocks, tail, lambda b: INF, N)[0], plain[0]), tail
        assert [b["what"] for e, b in enumerate(blocks) if not plain[1][e]] == ["err", "cut short of T"]
        modes = [("plain", None, plain), ("none", t_inf, plain), ("srpt", t_inf, plain)]
    whole = env.state.clone()

    for K, S in SHAPES:
        cand = {name: i32(env, cand_host[name][:K].tolist()) for name in KEYS}
        for P in N_PARENTS:
            roles = ["tie"] if P == 1 else ["tie", "none", "mixed"]
            parents = [5] if P == 1 else [B - 2, 3, outside[seen["launches"] % len(outside)]]
            reference = None
            for mode, T_dev, (cost, valid) in modes:
                # (one table per tail on the horizon pass: the cheapest block differs; on the plain pass the three launches share it)
                if reference is None or which == "horizon":
                    kids = child_tables(rng, K, S, roles, cost, valid, blocks, outside)
                inside = (kids >= 0) & (kids < B)
                c = np.where(inside, cost[np.clip(kids, 0, B - 1)], np.nan)
                ok = np.where(inside, valid[np.clip(kids, 0, B - 1)], False)
                score, best = host_pick(c, ok)
                best_buf = torch.full((P + N_GUARD,), GUARD_I32, dtype=torch.int32, device=dev)
                score_buf = torch.full((P * K + N_GUARD,), GUARD_F64, dtype=torch.float64, device=dev)
                slots = {name: torch.full((B,), -7, dtype=torch.int32, device=dev) for name in KEYS}
                args = (i32(env, parents), i32(env, kids.tolist()), cand)
                outs = (best_buf[:P], score_buf[: P * K].view(P, K), slots)
                if mode == "plain":
                    env.lookahead_pick(*args, *outs)
                else:
                    env.lookahead_pick_horizon(*args, T_dev, rem, mode, *outs)
                what = (which, mode, K, S, P)
                got_best, got_score = best_buf.cpu().numpy(), score_buf.cpu().numpy()
                assert (got_best[P:] == GUARD_I32).all() and (got_score[P * K:] == GUARD_F64).all(), (what, "guard words")
                gs = got_score[: P * K].reshape(P, K)
                wrong = np.argwhere(~((gs.view(np.uint64) == score.view(np.uint64)) | (np.isnan(gs) & np.isnan(score))))
                assert len(wrong) == 0, (what, "scores", [(int(p), int(k), gs[p, k], score[p, k]) for p, k in wrong[:5]])
                assert got_best[:P].tolist() == best.tolist(), (what, got_best[:P].tolist(), best.tolist())
                for name, t in slots.items():
                    want = np.full(B, -7)
                    for p in range(P):
                        if 0 <= parents[p] < B:
                            want[parents[p]] = cand_host[name][max(int(best[p]), 0)]
                    assert t.cpu().numpy().tolist() == want.tolist(), (what, name)
                assert torch.equal(env.state, whole), (what, "the pick kernel wrote to the arena")
                if mode == "plain":
                    reference = (gs.copy(), got_best[:P].copy())
                elif reference is not None:  # T = +inf on terminated children: the plain pick's bits
                    assert same_bits(gs, reference[0]) and got_best[:P].tolist() == reference[1].tolist(), (what, "differs from lookahead_pick")
                # what this launch reached
                seen["launches"] += 1
                seen["scores"] += P * K
                nan = np.isnan(score)
                seen["nan"] += int(nan.sum())
                seen["valid"] += int((~nan).sum())
                seen["nan_and_valid"] += int((nan.any(axis=1) & (~nan).any(axis=1)).sum())
                seen["outside_ids"] |= set(int(x) for x in kids[~inside])
                tied = [k for k in TIED if k < K]
                if len(tied) >= 2:
                    low = np.nanmin(score[0])
                    assert best[0] == 3 and all(same_bits(score[0, k], low) for k in tied) and not (score[0, :3] <= low).any(), (what, "the tie is not the lowest score")
                    assert all(k // 64 != tied[0] // 64 for k in tied[1:])
                    seen["ties"] += 1
                if P == 3:
                    assert best[1] == -1 and np.isnan(score[1]).all() and not (0 <= parents[2] < B)
                    seen["all_invalid"] += 1
                    seen["outside_parents"] += 1
                if which == "horizon":
                    for e in set(int(x) for x in kids[inside]):
                        if not valid[e]:
                            continue
                        seen["excluded"] = max(seen["excluded"], excluded_of[e])
                        if mode == "srpt":
                            w = works_of[e]
                            seen["m_max"] = max(seen["m_max"], len(w))
                            if len(w) > 64:
                                seen["m_distinct"] += len(set(w)) == len(w)
                                seen["m_duplicates"] += len(set(w)) < len(w)
            seen["shapes"].append((K, S, P))
    env.close()
    assert seen["nan"] > 0 and seen["valid"] > 0 and seen["nan_and_valid"] > 0, "no parent holds a NaN score beside a valid one"
    assert seen["ties"] > 0 and seen["all_invalid"] > 0 and seen["outside_parents"] > 0
    assert seen["outside_ids"] == set(outside), f"ids outside the arena that no child table held: {set(outside) - seen['outside_ids']}"
    if which == "horizon":
        assert seen["excluded"] > 0, "no valid child excludes a job by t_arrival >= T"
        assert seen["m_max"] == 1024 and seen["m_distinct"] > 0 and seen["m_duplicates"] > 0, "the srpt tail sorted no more than 64 works, distinct and with duplicates"
    seen["outside_ids"] = sorted(seen["outside_ids"])
    return seen


# ---- 2. rem_work with more than two strides of active jobs ------------------------------------------------------------------

def dense_env(num_executors: int, B: int, seeds: list[int], pack, device, lib):
    env = VecSparkSchedSimEnv({**DENSE, "num_executors": num_executors}, B, device=device, pack=pack, _lib=lib)
    env.reset(seed=seeds)
    return env


def check_dense_rem_work(num_executors: int, pack, device, lib) -> dict:
    """six envs play 400000 time units of a queue that arrives twenty times faster than it drains: well over 128 active jobs each"""
    env = dense_env(num_executors, 6, DENSE_SEEDS, pack, device, lib)
    pol, par = per_env(env, dict(enumerate(EACH_POLICIES)))
    out = env.rollout_until(pol, par, DENSE_HORIZON, 100000)
    n_active = [env.header(e)["n_active"] for e in range(6)]
    assert not HU.over(env).any() and (env.header_field("err") == 0).all() and (out["steps"] > 0).all(), "an env ended or is in error"
    assert max(n_active) > 128 and min(n_active) > 64, n_active
    assert (HU.walls(env) >= out["t_stop"].cpu().numpy()).all()
    rem = out["rem_work"].cpu().numpy()
    assert rem.shape == (6, 200) and env.dims.job_cap == 200
    for e in range(6):
        W = schedulers.job_work(env.obs_view(e))
        ids = HU.active_ids(env, e)
        assert len(W) == len(ids) == n_active[e] and len(set(ids)) == len(ids)
        want = np.zeros(200)
        want[ids] = W
        assert np.array_equal(HU.bits(rem[e]), HU.bits(want)), (e, np.nonzero(HU.bits(rem[e]) != HU.bits(want))[0].tolist())
        assert (rem[e] != 0).sum() > 64, "no more than one stride of the row holds work: a stride that is skipped would not show"
    whole = env.state.clone()
    again = env.rollout_until(pol, par, DENSE_HORIZON, 0)
    assert again["steps"].tolist() == [0] * 6 and torch.equal(env.state, whole), "max_steps = 0 moved the state"
    assert np.array_equal(HU.bits(again["rem_work"].cpu().numpy()), HU.bits(rem))
    env.close()
    return dict(num_executors=num_executors, n_active=n_active)


# ---- 3. the horizon pick on those children ------------------------------------------------------------------------------

def check_dense_pick(pack, device, lib) -> dict:
    """two dense parents, three candidates (a duplicate pair), two reseeded samples: real rem_work rows under the sort at P = 256"""
    cands = [("fair", 0), ("fair", 0), ("fifo", 0)]
    P, K, S = 2, len(cands), 2
    B = P * (1 + K * S)
    env = dense_env(5, B, DENSE_SEEDS[:P] + [7] * (B - P), pack, device, lib)
    env.rollout_until(*per_env(env, {p: EACH_POLICIES[p] for p in range(P)}), DENSE_HORIZON, 100000)
    assert not HU.over(env)[:P].any() and all(env.header(p)["n_active"] > 128 for p in range(P))
    kids = np.arange(P, B).reshape(P, K, S)
    trio = list(np.ndindex(P, K, S))
    env.fork([p for p, _, _ in trio], [int(kids[t]) for t in trio], reseed=[500 + s for _, _, s in trio])
    out = env.rollout_until(*per_env(env, {int(kids[p, k, s]): cands[k] for p, k, s in trio}), CHILD_HORIZON, 100000)
    t_stop, rem = out["t_stop"].cpu().numpy(), out["rem_work"].cpu().numpy()
    assert (out["steps"][P:] > 0).all() and all(len({t_stop[int(c)] for c in kids[p].reshape(-1)}) == 1 for p in range(P))
    cand = {name: i32(env, [10 * (n + 1) + k for k in range(K)]) for n, name in enumerate(KEYS)}
    m = []
    for c in kids.reshape(-1):
        h = env.header(int(c))
        ta, tc = env.job_times(int(c))[:2]
        assert h["err"] == 0 and h["terminated"] == 0 and h["wall_time"] >= t_stop[c] and h["next_arrival"] == 200
        m.append(sum(1 for j in range(200) if ta[j] < t_stop[c] and tc[j] > h["wall_time"]))
    assert max(m) > 64, m  # (200 arrived jobs: the network sorts P = 256 keys)
    whole = env.state.clone()
    result = dict(m=m)
    for tail in ("none", "srpt"):
        cost, ok = np.zeros((P, K, S)), np.zeros((P, K, S), dtype=bool)
        for t in trio:
            c = int(kids[t])
            cost[t], info = HU.host_cost(env, c, float(t_stop[c]), rem[c], tail)
            ok[t] = info["valid"]
            assert info["valid"] and (tail == "none" or info["open_work"])
        score, best = host_pick(cost, ok)
        got_best = torch.full((P,), GUARD_I32, dtype=torch.int32, device=env.device)
        got_score = torch.zeros((P, K), dtype=torch.float64, device=env.device)
        slots = {name: torch.full((B,), -7, dtype=torch.int32, device=env.device) for name in KEYS}
        env.lookahead_pick_horizon(i32(env, list(range(P))), i32(env, kids.tolist()), cand, out["t_stop"], out["rem_work"], tail, got_best, got_score, slots)
        assert torch.equal(env.state, whole), "the pick kernel wrote to the arena"
        gs = got_score.cpu().numpy()
        assert not np.isnan(score).any() and np.array_equal(HU.bits(gs), HU.bits(score)), (tail, gs, score)
        assert got_best.tolist() == best.tolist() and (best != 1).all(), (tail, got_best.tolist(), best.tolist())
        assert np.array_equal(HU.bits(score[:, 0]), HU.bits(score[:, 1])), "the duplicate candidates differ"
        for name, t in slots.items():
            assert t.tolist() == [int(cand[name][int(best[p])]) for p in range(P)] + [-7] * (B - P), (tail, name)
        result[tail] = best.tolist()
    env.close()
    return result
