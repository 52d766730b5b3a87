"""The checks of the lookahead over ACTIONS (include/sss.h sss_decima_topk and sss_rollout_action; DecimaPolicy.topk_env and
rollout_action_env, VecSparkSchedSimEnv.rollout_action, lookahead.ActionLookaheadScheduler), shared by
tests/test_emu_action_lookahead.py (the CPU wave emulator) and tests/test_gpu_action_lookahead.py (the kernels). Every check takes
(device, lib): ("cpu", the emulator's library) or ("cuda:0", None). What the new calls are held to is the existing ones - `act_env`,
`step_async`, `rollout_each`, `rollout_env`, `fork`, `job_stats` - bit for bit; the one tolerance is the log-probabilities' stage term
against fp64, with the bound tests/inference_fp64_util.py holds the one-launch route's scores to (its CEILING). Envs and weights are
those of tests/fused_decima_util.py: the TINY config at 5 and at 100 executors, 8 envs that played a prefix under `fair`, the
reference's published model."""
from __future__ import annotations

import numpy as np
import torch

from fork_util import SKIP, TINY, env_bytes, same_bytes
from fused_decima_util import CONFIGS, COUNTER0, SEED, batch_bytes, differing, image, live_mask, make_env, make_policy, prepared
from inference_fp64_util import CEILING
from lookahead_util import i32, no_ticks, per_env
from spark_sched_sim_amd import evaluation
from spark_sched_sim_amd.binding import POLICY_DECIMA, POLICY_IDS
from spark_sched_sim_amd.decima import DecimaPolicy
from spark_sched_sim_amd.lookahead import ActionLookaheadScheduler, LookaheadScheduler

KS = (1, 4, 64)
POINTS = (0, 12, 12)  # the stretch's points: steps under `fair` before each (the envs move on between the looks)


def bits(t) -> np.ndarray:
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def rows(env) -> list[dict]:
    """per env, from the observation rows: the node ids of the schedulable stages in ascending order, every node's job, the jobs' caps"""
    oi = env.obs_i32.cpu().numpy()
    nodes, dag_ptr, sup = env.nodes.cpu().numpy(), env.dag_ptr.cpu().numpy(), env.exec_supplies.cpu().numpy()
    E, out = env.num_executors, []
    for e in range(env.num_envs):
        n, A, ncommit, src = int(oi[e, 0]), int(oi[e, 2]), int(oi[e, 4]), int(oi[e, 5])
        sched = np.flatnonzero(nodes[e, :n, 2] != 0.0)
        job = np.searchsorted(dag_ptr[e, 1: A + 1], np.arange(n), side="right") if A else np.zeros(0, dtype=np.int64)
        cap = [ncommit if a == src else min(max(E - int(sup[e, a]), 0), ncommit) for a in range(A)]
        out.append(dict(n=n, A=A, sched=sched, job=job, cap=cap, ncommit=ncommit))
    return out


def advance(env, n: int) -> None:
    if n:
        env.rollout("fair", n)


def zero_last_layers(policy: DecimaPolicy) -> DecimaPolicy:
    """every stage score equals the stage network's last bias and every count score the exec network's: all scores tie"""
    with torch.no_grad():
        policy.stage_policy_network.mlp_score[4].weight.zero_()
        policy.exec_policy_network.mlp_score[4].weight.zero_()
    policy.invalidate_kernel_weights()
    return policy


# ---- 1. slot 0 is the policy -------------------------------------------------------------------------

def check_slot0_is_the_policy(which: str, pack, device, lib) -> None:
    policy = make_policy(CONFIGS[which], device)
    env = prepared(which, pack, device, lib)
    seen = dict(nodes=0, commit=0, few=0)
    for gap in POINTS:
        advance(env, gap)
        act, aux = policy.act_env(env, 0, greedy=True)
        want = {"stage_idx": act["stage_idx"].clone(), "num_exec": act["num_exec"].clone(), "lgprob": aux["lgprob"].clone()}
        r = rows(env)
        seen["nodes"] = max(seen["nodes"], max(x["n"] for x in r))
        seen["commit"] = max(seen["commit"], max(x["ncommit"] for x in r))
        seen["few"] += sum(0 < len(x["sched"]) < 4 for x in r)
        for k in KS:
            top = policy.topk_env(env, k)
            for name in want:
                assert np.array_equal(bits(top[name][:, 0]), bits(want[name])), (which, k, name, top[name][:, 0].tolist(), want[name].tolist())
            assert top["stage_idx"].shape == (env.num_envs, k) and top["count"].dtype == torch.int32
    print(which, seen)
    assert seen["nodes"] > 64 and seen["few"] >= 1, seen  # the lane stride, and an env with fewer schedulable stages than k = 4
    if CONFIGS[which]["num_executors"] > 64:
        assert seen["commit"] > 64, seen
    env.close()


# ---- 2. order and padding --------------------------------------------------------------------------------

def _log_softmax64(row: np.ndarray, at: int) -> float:
    fin = np.isfinite(row)
    if not fin.any():
        return 0.0
    v = row[fin].astype(np.float64)
    return float(row[at]) - (v.max() + np.log(np.exp(v - v.max()).sum()))


def check_order_and_padding(which: str, pack, device, lib) -> None:
    policy = make_policy(CONFIGS[which], device)
    env = prepared(which, pack, device, lib)
    B = env.num_envs
    active = torch.ones(B, dtype=torch.bool, device=env.device)
    active[2] = False
    worst, slots = 0.0, 0
    for gap in POINTS:
        advance(env, gap)
        _, aux = policy.act_env(env, 0, greedy=True, want_scores=True)
        ss, r = aux["stage_scores"].cpu().numpy(), rows(env)
        for k in (4, 64):
            top = {n: t.cpu().numpy() for n, t in policy.topk_env(env, k, active=active, want_scores=True).items()}
            for e in range(B):
                si, ne, lg, es = top["stage_idx"][e], top["num_exec"][e], top["lgprob"][e], top["exec_scores"][e]
                if e == 2:
                    assert top["count"][e] == 0 and (si == -1).all() and (ne == -1).all() and np.isneginf(lg).all(), (which, k, e)
                    continue
                sc = ss[e][r[e]["sched"]]
                assert np.isfinite(sc).all()
                count = max(1, min(k, len(sc)))
                assert top["count"][e] == count, (which, k, e, top["count"][e], count)
                assert (si[count:] == -1).all() and (ne[count:] == -1).all() and np.isneginf(lg[count:]).all() and np.isneginf(es[count:]).all(), (which, k, e)
                if len(sc) == 0:
                    assert (si[0], ne[0], lg[0]) == (-1, 1, 0.0), (which, k, e)
                    continue
                order = np.argsort(-(sc + np.float32(0.0)), kind="stable")[:count]  # descending, equal keys to the lower index
                assert si[:count].tolist() == order.tolist(), (which, k, e, si[:count].tolist(), order.tolist())
                lse = float(sc.astype(np.float64).max() + np.log(np.exp(sc.astype(np.float64) - sc.astype(np.float64).max()).sum()))
                for q in range(count):
                    stage_term = float(lg[q]) - _log_softmax64(es[q], int(ne[q]) - 1)
                    err = abs(stage_term - (float(sc[order[q]]) - lse))
                    worst, slots = max(worst, err), slots + 1
                    assert err <= CEILING, (which, k, e, q, err)
    print(which, "slots", slots, "worst stage-term error", worst, "bound", CEILING)
    env.close()


# ---- 3. ties, exactly ------------------------------------------------------------------------------------

def check_ties(which: str, pack, device, lib) -> None:
    policy = zero_last_layers(make_policy(CONFIGS[which], device))
    env = prepared(which, pack, device, lib)
    r = rows(env)
    for k in KS:
        top = {n: t.cpu().numpy() for n, t in policy.topk_env(env, k).items()}
        for e in range(env.num_envs):
            ns = len(r[e]["sched"])
            count = max(1, min(k, ns))
            want = list(range(count)) if ns else [-1]
            assert top["count"][e] == count and top["stage_idx"][e, :count].tolist() == want, (which, k, e, top["stage_idx"][e].tolist())
            assert (top["num_exec"][e, :count] == 1).all() and (top["num_exec"][e, count:] == -1).all(), (which, k, e)
    assert any(len(x["sched"]) > 4 for x in r)
    env.close()


# ---- 4. the executor counts of the other slots -------------------------------------------------------------

EXEC_K = 4
EXEC_COUNTERS = {"narrow": range(2000, 2040), "wide": range(2000, 2040)}  # of the sampled `act_env` calls that reach the other jobs' rows


def check_exec_counts(which: str, pack, device, lib) -> None:
    policy = make_policy(CONFIGS[which], device)
    env = prepared(which, pack, device, lib)
    B, E, k = env.num_envs, env.num_executors, EXEC_K
    r = rows(env)
    top = {n: t.cpu().numpy() for n, t in policy.topk_env(env, k, want_scores=True).items()}
    _, aux = policy.act_env(env, 0, greedy=True, want_scores=True)
    own = aux["exec_scores"].cpu().numpy()
    slot_job = {}
    for e in range(B):
        for q in range(int(top["count"][e])):
            if top["stage_idx"][e, q] < 0:
                continue
            a = int(r[e]["job"][r[e]["sched"][top["stage_idx"][e, q]]])
            slot_job[e, q] = a
            row = top["exec_scores"][e, q]
            cap = r[e]["cap"][a]
            assert np.isfinite(row[:cap]).all() and np.isneginf(row[cap:]).all(), (which, e, q, cap, row)
            assert int(top["num_exec"][e, q]) - 1 == (int(np.argmax(row)) if cap > 0 else 0), (which, e, q)
            if a == slot_job[e, 0]:
                assert np.array_equal(bits(row), bits(own[e])), (which, e, q, "the policy's own exec_scores row")
    others = {(e, q) for (e, q), a in slot_job.items() if q >= 1 and a != slot_job[e, 0]}
    covered = set()
    for c in EXEC_COUNTERS[which]:
        _, s = policy.act_env(env, c, seed=SEED, greedy=False, want_scores=True)
        job, es = s["job_idx"].cpu().numpy(), s["exec_scores"].cpu().numpy()
        for (e, q) in others:
            if int(job[e]) == slot_job[e, q] and bool(s["any_stage"][e]):
                assert np.array_equal(bits(top["exec_scores"][e, q]), bits(es[e])), (which, e, q, c)
                covered.add((e, q))
    print(which, "slots of other jobs:", len(others), "covered by a sampled draw:", len(covered))
    assert len(others) >= 4 and 2 * len(covered) >= len(others), (which, len(others), len(covered))
    env.close()


# ---- 5. a forced action is a step ----------------------------------------------------------------------------

def _second_choices(policy, env):
    """a legal action per env that is not the policy's own where there is a choice: top-2's last filled slot"""
    top = policy.topk_env(env, 2)
    at = (top["count"].long() - 1).clamp(min=0)[:, None]
    return top["stage_idx"].gather(1, at)[:, 0].contiguous(), top["num_exec"].gather(1, at)[:, 0].contiguous()


def check_forced_action(which: str, follower: str, pack, device, lib) -> None:
    """follower: "fair" / "sjfcp" (the heuristic kernel, policy arguments NULL), "decima_greedy", "decima_sampled" """
    cfg, n = CONFIGS[which], 12
    policy = make_policy(cfg, device)
    a, b = prepared(which, pack, device, lib), prepared(which, pack, device, lib)
    B = a.num_envs
    assert B == 8
    decima, greedy = follower.startswith("decima"), follower != "decima_sampled"
    fid = POLICY_DECIMA if decima else POLICY_IDS[follower]
    si, ne = _second_choices(policy, a)
    assert bool((ne >= 1).all()) and bool((si >= 0).all())
    #                  0    1  2  3  4  5  6  7
    pol = i32(a, [-1, fid, fid, fid, fid, fid, fid, fid])
    par = i32(a, [0] * 8)
    mode = [1, -1, 0, 1, 1, 1, 1, 1]  # first_exec: forced (the action's count), < 0 sits out, 0 = the policy's own first step
    fe = torch.where(i32(a, mode) == 1, ne, i32(a, mode)).contiguous()
    forced = [e for e in range(B) if mode[e] == 1 and e != 0]
    held = {e: env_bytes(a, e) for e in (0, 1)}
    before = a.header_field("ep_steps").tolist()

    def run(env, steps, counter, ids, first=None):
        """the EXISTING fused kernels for the envs `ids`"""
        p = [-1] * B
        for e in ids:
            p[e] = fid
        if decima:
            return policy.rollout_env(env, steps, greedy=greedy, seed=SEED, counter=counter, policy=i32(env, p), param=par)
        return env.rollout_each(i32(env, p), par, steps)

    if decima:
        out = policy.rollout_action_env(a, n, si, fe, greedy=greedy, seed=SEED, counter=COUNTER0, policy=pol, param=par)
    else:
        out = a.rollout_action(pol, par, n, si, fe)
    for e in (0, 1):
        assert same_bytes(held[e], env_bytes(a, e)) == [], f"env {e} sits out and changed"
    assert out["steps"].tolist()[:2] == [0, 0] and out["first_stage_idx"].tolist()[:2] == [-1, -1]
    # the twin: the action by sss_step, then the follower by the existing kernels (a sampled one draws with counter + it, it from 1)
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=b.device)
    sel = torch.zeros(B, dtype=torch.bool)
    sel[forced] = True
    b.step_async(torch.where(sel.to(b.device), si, skip).contiguous(), ne)
    rest = run(b, n - 1, COUNTER0 + 1, forced)
    own = run(b, n, COUNTER0, [2])
    for e in forced:
        bad = same_bytes(image(b, e), image(a, e))
        assert bad == [], f"{which} {follower} env {e}: {bad}"
        assert int(out["steps"][e]) == 1 + int(rest["steps"][e]) == a.header(e)["ep_steps"] - before[e]
        assert int(out["first_stage_idx"][e]) == int(si[e]) and int(out["first_num_exec"][e]) == int(ne[e])
    assert same_bytes(no_ticks(env_bytes(b, 2)), no_ticks(env_bytes(a, 2))) == [], "entry 0 is the existing kernel's call"
    for k_ in ("steps", "first_stage_idx", "first_num_exec"):
        assert int(out[k_][2]) == int(own[k_][2]), k_
    assert any(int(out["steps"][e]) == n for e in forced)
    print(which, follower, "steps", out["steps"].tolist())
    a.close(), b.close()


def check_refused_action(which: str, pack, device, lib) -> None:
    """an action the env refuses: sss_step's error state, no other env is touched; id 5 without policy arguments gives steps = -1"""
    policy = make_policy(CONFIGS[which], device)
    a, b = prepared(which, pack, device, lib), prepared(which, pack, device, lib)
    B = a.num_envs
    bad_si = i32(a, [0, 10_000, 0, 0, 0, 0, 0, 0])
    bad_ne = i32(a, [-1, 1, -1, 10_000, -1, -1, -1, -1])  # env 1: no such stage; env 3: more executors than there are; the others sit out
    fair = i32(a, [POLICY_IDS["fair"]] * B)
    zero = i32(a, [0] * B)
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=b.device)
    sel = torch.tensor([e in (1, 3) for e in range(B)]).to(b.device)
    b.step_async(torch.where(sel, bad_si, skip).contiguous(), bad_ne)
    for decima in (False, True):
        if decima:
            a.close()
            a = prepared(which, pack, device, lib)
        held = {e: env_bytes(a, e) for e in range(B) if e not in (1, 3)}  # (of THIS preparation: the header's shader-clock counters differ between two)
        if decima:
            out = policy.rollout_action_env(a, 5, bad_si, bad_ne)
        else:
            out = a.rollout_action(fair, zero, 5, bad_si, bad_ne)
        for e in (1, 3):
            assert same_bytes(no_ticks(env_bytes(b, e)), no_ticks(env_bytes(a, e))) == [], (decima, e)
            assert a.header(e)["err"] != 0 and int(out["steps"][e]) == 0, (decima, e, a.header(e)["err"])
        for e in held:
            assert same_bytes(held[e], env_bytes(a, e)) == [], (decima, e)
    five = i32(a, [POLICY_DECIMA] * B)
    whole = batch_bytes(a)
    assert a.rollout_action(five, zero, 5, zero, zero)["steps"].tolist() == [-1] * B
    assert differing(whole, batch_bytes(a)) == []
    a.close(), b.close()


# ---- 6. the scheduler is its composition -----------------------------------------------------------------------

def compose_action_decision(env, policy, sched, parents, kids, k, S, decision, max_steps=5000):
    """one decision written with the calls that existed before: fork; top-k; every slot's action by step_async in lock step; the
    base policy (Decima, arg-max) to the end by rollout_env; job_stats column 1; the mean over a slot's samples and the arg-min in
    numpy, ties to the lowest slot; the parents take the winner's action by step_async"""
    B, P = env.num_envs, len(parents)
    src = [p for p in parents for _ in range(k * S)]
    dst = [int(c) for c in kids.reshape(-1)]
    seeds = None
    if sched.reseed is not None:
        seeds = [sched.seed_for(s, decision) for _ in range(P * k) for s in range(S)]
    env.fork(src, dst, reseed=seeds)
    active = torch.zeros(B, dtype=torch.bool)
    active[parents] = True
    top = {n: t.clone() for n, t in policy.topk_env(env, k, active=active.to(env.device)).items()}
    si, ne = torch.full((B,), SKIP, dtype=torch.int32), torch.ones(B, dtype=torch.int32)
    t_si, t_ne = top["stage_idx"].cpu(), top["num_exec"].cpu()
    pol = [-1] * B
    for i, p in enumerate(parents):
        for q in range(k):
            if int(t_ne[p, q]) >= 1:
                for c in kids[i, q]:
                    si[c], ne[c], pol[c] = t_si[p, q], t_ne[p, q], POLICY_DECIMA
    env.step_async(si.to(env.device), ne.to(env.device))
    policy.rollout_env(env, max_steps, greedy=True, policy=i32(env, pol), param=i32(env, [0] * B))
    stats = env.job_stats()["stats"].cpu().numpy()
    ok = ((env.header_field("terminated") != 0) & (env.header_field("err") == 0)).cpu().numpy()
    score = np.full((P, k), np.nan)
    for i in range(P):
        for q in range(k):
            ids = [int(c) for c in kids[i, q]]
            if all(ok[c] and pol[c] != -1 for c in ids):
                acc = 0.0
                for c in ids:
                    acc = acc + stats[c, 1]
                score[i, q] = acc / S
    best = [int(np.nanargmin(score[i])) if not np.isnan(score[i]).all() else -1 for i in range(P)]
    si, ne = torch.full((B,), SKIP, dtype=torch.int32), torch.ones(B, dtype=torch.int32)
    for i, p in enumerate(parents):
        si[p], ne[p] = t_si[p, max(best[i], 0)], t_ne[p, max(best[i], 0)]
    env.step_async(si.to(env.device), ne.to(env.device))
    return best, score, top


LA_PREFIX = {"seeds": [3, 4], "fair": 30}


def check_scheduler_against_composition(samples: int, reseed, decisions: int, pack, device, lib, k: int = 3) -> None:
    P, S = 2, samples
    B = P * (1 + k * S)
    parents, kids = list(range(P)), np.arange(P, B).reshape(P, k, S)
    policy = make_policy(TINY, device)
    env, ref = make_env(TINY, B, pack, device, lib), make_env(TINY, B, pack, device, lib)
    for e in (env, ref):  # parent 0 stays where the reset left it (two schedulable stages: an empty slot), parent 1 plays on to a state with several jobs
        e.reset(seed=LA_PREFIX["seeds"] + [0] * (B - P))
        e.rollout_each(*per_env(e, {1: ("fair", 0)}), LA_PREFIX["fair"])
    sched = ActionLookaheadScheduler(env, parents, policy, k, samples=S, reseed=reseed)
    empties, winners = 0, []
    for d in range(decisions):
        before = [env.header(p)["ep_steps"] for p in parents]
        sched.decide_and_step()
        best, score, top = compose_action_decision(ref, policy, sched, parents, kids, k, S, d)
        got = sched.last_scores.cpu().numpy()
        assert np.array_equal(bits(got), bits(score)), (d, got, score)
        assert sched.last_best.tolist() == best, (d, sched.last_best.tolist(), best)
        for name in ("stage_idx", "num_exec", "lgprob", "count"):
            assert np.array_equal(bits(sched.last_actions[name]), bits(top[name][parents])), (d, name)
        assert (sched.parent_out["steps"][:P] == 1).all()
        for p in parents:
            bad = same_bytes(image(ref, p), image(env, p))
            assert bad == [], f"decision {d}, parent {p}: {bad}"
        cnt = sched.last_actions["count"].tolist()
        for i in range(P):
            for q in range(cnt[i], k):  # the children of an empty slot sat out: still the parent's copy, invalid in the pick
                empties += 1
                assert np.isnan(got[i, q])
                for c in kids[i, q]:
                    assert same_bytes(no_ticks(env_bytes(env, int(c))), no_ticks(env_bytes(ref, int(c)))) == [], (d, i, q)
                    assert env.header(int(c))["terminated"] == 0 and env.header(int(c))["ep_steps"] == before[i]
        winners.append(best)
        if reseed is not None:
            want = [sched.seed_for(s, d) for _ in range(P * k) for s in range(S)]
            assert [int(x) % 2 ** 64 for x in sched._seeds.tolist()] == want
    print("samples", S, "reseed", reseed, "winners", winners, "empty slots seen", empties)
    assert empties >= 1, "want a parent with fewer schedulable stages than k"
    env.close(), ref.close()
    return empties


# ---- 7. the guarantee ------------------------------------------------------------------------------------------

GUARANTEE_SEEDS = [0, 1, 2]
EMU_PREFIX = 80  # steps of greedy Decima before the emulator's lookahead takes over


def check_guarantee(prefix: int | None, pack, device, lib, seeds=GUARANTEE_SEEDS, k: int = 3, max_decisions: int = 5000) -> dict:
    """reseed=None, base Decima, k = 3: the best score never increases from one decision to the next, and the parents end at or below
    the greedy Decima episode from the same state - strictly below on at least one seed. `prefix`: None = whole episodes (the GPU's
    share); a number = the parents first play that many steps under greedy Decima (an existing path) and the lookahead takes the
    remaining decisions, which keeps the emulator's run affordable."""
    P = len(seeds)
    B = P * (1 + k)
    policy = make_policy(TINY, device)
    env, solo = make_env(TINY, B, pack, device, lib), make_env(TINY, P, pack, device, lib)
    env.reset(seed=list(seeds) + [0] * (B - P))
    solo.reset(seed=list(seeds))
    policy.rollout_env(solo, 5000, greedy=True)
    assert bool((solo.header_field("terminated") != 0).all())
    own = solo.job_stats()["stats"][:, 1].cpu().numpy()
    if prefix:
        pol = i32(env, [POLICY_DECIMA] * P + [-1] * (B - P))
        policy.rollout_env(env, prefix, greedy=True, policy=pol, param=i32(env, [0] * B))
    sched = ActionLookaheadScheduler(env, list(range(P)), policy, k, base=("decima", 0), reseed=None)
    last = np.full(P, np.inf)
    for d in range(max_decisions):
        if not bool(live_mask(env)[:P].any()):
            break
        live = live_mask(env)[:P].cpu().numpy()
        sched.decide_and_step()
        sc = sched.last_scores.cpu().numpy()
        best = np.array([np.nanmin(row) if not np.isnan(row).all() else np.nan for row in sc])
        assert not np.isnan(best[live]).any() and (best[live] <= last[live]).all(), (d, best, last)
        last = np.where(live, best, last)
    assert sched.fallbacks == 0 and bool((env.header_field("terminated")[:P] != 0).all()) and bool((env.obs_i32[:P, 7] == 0).all())
    total = env.job_stats()["stats"][:P, 1].cpu().numpy()
    print("seeds", list(seeds), "prefix", prefix, "greedy Decima:", own.tolist(), "action lookahead k=3:", total.tolist(), "decisions", sched.decisions)
    assert (total <= own).all(), (total, own)
    assert (total < own).any(), (total, own)
    env.close(), solo.close()
    return {"own": own, "lookahead": total}


# ---- 8. refusals -------------------------------------------------------------------------------------------------

def check_refusals(pack, device, lib) -> None:
    import ctypes as C

    import pytest
    from spark_sched_sim_amd import binding as Bn
    from spark_sched_sim_amd.binding import SssDecimaPolicyArgs

    policy = make_policy(TINY, device)
    env = make_env(TINY, 4, pack, device, lib)
    env.reset(seed=[51, 52, 53, 54])
    L = env._b.lib
    assert {"sss_decima_topk", "sss_rollout_action"} <= set(Bn.EXPORTS) and hasattr(L, "sss_decima_topk") and hasattr(L, "sss_rollout_action")
    policy.rollout_env(env, 0)  # (binds the kernels, makes the work space and the packed weights; takes no step)
    whole = batch_bytes(env)
    w, ws = policy._packed_weights(), policy._ws
    fields = [f[0] for f in SssDecimaPolicyArgs._fields_]

    def args(**change):
        a = SssDecimaPolicyArgs(None, 200.0, 1e5, policy._packed[2], w["prep"].data_ptr(), w["msg"].data_ptr(), w["update"].data_ptr(), w["dag"].data_ptr(),
                                w["glob"].data_ptr(), w["stage"].data_ptr(), w["exec"].data_ptr(), ws["node"].data_ptr(), ws["job"].data_ptr(), 0, 0,
                                ws["stage_idx"].data_ptr(), ws["num_exec"].data_ptr(), ws["stage_sel"].data_ptr(), ws["job_idx"].data_ptr(), ws["exec_sel"].data_ptr(),
                                ws["lgprob"].data_ptr(), None, None, None)
        for k, v in change.items():
            assert k in fields, k
            setattr(a, k, v)
        return a

    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    k = 4
    o = {"si": torch.zeros((4, k), dtype=torch.int32, device=env.device), "ne": torch.zeros((4, k), dtype=torch.int32, device=env.device),
         "lg": torch.zeros((4, k), dtype=torch.float32, device=env.device), "cnt": torch.zeros(4, dtype=torch.int32, device=env.device)}

    def topk(a, k=k, **none):
        p = {n: (None if n in none else t.data_ptr()) for n, t in o.items()}
        return L.sss_decima_topk(env._h, C.byref(a) if a is not None else None, k, p["si"], p["ne"], p["lg"], p["cnt"], None, None)

    def refused(rc, code, message):
        assert rc == code and message in L.sss_last_error().decode(), (rc, L.sss_last_error().decode())

    refused(topk(None), -56, "policy arguments are NULL")
    for f in ("w_prep_dev", "w_msg_dev", "w_upd_dev", "w_dag_dev", "w_glob_dev", "w_stage_dev", "w_exec_dev"):
        refused(topk(args(**{f: None})), -56, "weight pointer")
    for f in ("node_scratch_dev", "job_scratch_dev"):
        refused(topk(args(**{f: None})), -56, "scratch")
    for n in o:
        refused(topk(args(), **{n: True}), -56, "output pointer")
    for bad in (0, -1, 65):
        refused(topk(args(), k=bad), -56, "k must be in [1, 64]")
    # `num_executors > 128` (-56 here, -57 in sss_rollout_action) cannot be reached through the ABI: no handle has more executors than
    # sss_create takes, so what is checked is that one - the two calls keep their own check as the last line of defence, as
    # sss_decima_policy and sss_rollout_decima do
    with pytest.raises(ValueError, match=r"num_executors must be in \[1, 128\]"):
        make_env({**TINY, "num_executors": 129}, 1, pack, device, lib)
    # the single-decision outputs, the score and profile pointers are ignored and may be NULL
    assert topk(args(stage_idx_dev=None, num_exec_dev=None, stage_sel_dev=None, job_idx_dev=None, exec_sel_dev=None, lgprob_dev=None)) == 0
    for bad in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            policy.topk_env(env, bad)
    with pytest.raises(ValueError, match="out\\['count'\\]"):
        policy.topk_env(env, 2, out={"stage_idx": o["si"][:, :2].contiguous(), "num_exec": o["ne"][:, :2].contiguous(), "lgprob": o["lg"][:, :2].contiguous(),
                                     "count": o["cnt"].long()})

    some = i32(env, [0, 0, 0, 0])
    sit = i32(env, [-1, -1, -1, -1])

    def action(a, pol=some, par=some, fs=some, fe=sit, n=5):
        return L.sss_rollout_action(env._h, C.byref(a) if a is not None else None, 1, ptr(pol), ptr(par), ptr(fs), ptr(fe), n, None, None, None, None)

    for a in (None, args()):
        refused(action(a, fs=None), -57, "first_stage_in_dev / first_exec_in_dev is NULL")
        refused(action(a, fe=None), -57, "first_stage_in_dev / first_exec_in_dev is NULL")
        refused(action(a, n=-1), -57, "n_steps must be >= 0")
    refused(action(None, pol=None), -57, "policy_dev / param_dev is NULL")
    refused(action(None, par=None), -57, "policy_dev / param_dev is NULL")
    for f in ("w_prep_dev", "w_msg_dev", "w_upd_dev", "w_dag_dev", "w_glob_dev", "w_stage_dev", "w_exec_dev"):
        refused(action(args(**{f: None})), -57, "weight pointer")
    for f in ("node_scratch_dev", "job_scratch_dev"):
        refused(action(args(**{f: None})), -57, "scratch")
    for f in ("stage_idx_dev", "num_exec_dev", "stage_sel_dev", "job_idx_dev", "exec_sel_dev", "lgprob_dev"):
        refused(action(args(**{f: None})), -57, "output pointer")
    nonnull = ws["lgprob"].data_ptr()
    refused(action(args(active_dev=nonnull)), -57, "active_dev must be NULL")
    refused(action(args(stage_scores_dev=nonnull)), -57, "must be NULL")
    refused(action(args(exec_scores_dev=nonnull)), -57, "must be NULL")
    refused(action(args(prof_dev=nonnull)), -57, "prof_dev must be NULL")
    refused(action(args(), pol=None), -57, "policy_dev and param_dev come together")
    refused(action(args(), par=None), -57, "policy_dev and param_dev come together")
    with pytest.raises(ValueError, match="n_steps must be >= 0"):
        env.rollout_action(some, some, -1, some, sit)
    with pytest.raises(ValueError, match="int32"):
        env.rollout_action(some, some, 5, some.long(), sit)
    with pytest.raises(ValueError, match="int32"):
        policy.rollout_action_env(env, 5, some, sit.long())
    with pytest.raises(ValueError, match="together"):
        policy.rollout_action_env(env, 5, some, sit, policy=some)
    env.enable_timeline(8)
    with pytest.raises(ValueError, match="not available while a timeline is recorded"):
        env.rollout_action(some, some, 5, some, sit)
    with pytest.raises(ValueError, match="not available while a timeline is recorded"):
        policy.rollout_action_env(env, 5, some, sit)
    env.disable_timeline()
    assert differing(whole, batch_bytes(env)) == [], "a refused call touched an env"
    # the scheduler's arguments: the existing class's
    la = make_env(TINY, 8, pack, device, lib)
    for kw, msg in ((dict(decima=None, k=2), "needs decima="), (dict(decima=policy, k=0), "k must be in"), (dict(decima=policy, k=65), "k must be in"),
                    (dict(decima=policy, k=4), "need 10 envs"), (dict(decima=policy, k=2, samples=1024), "at most 1024"),
                    (dict(decima=policy, k=2, children=[2, 3, 4, 4]), "distinct"), (dict(decima=policy, k=2, children=[0, 3, 4, 5]), "disjoint")):
        with pytest.raises(ValueError, match=msg):
            ActionLookaheadScheduler(la, [0, 1], **kw)
    with pytest.raises(ValueError, match="distinct env ids"):
        ActionLookaheadScheduler(la, [0, 0], policy, 1)
    with pytest.raises(KeyError):
        ActionLookaheadScheduler(la, [0], policy, 2, base=("no_such_policy", 0))
    with pytest.raises(TypeError):
        ActionLookaheadScheduler(la, [0], policy, 2, horizon=1e5)  # there is no time-bounded form
    sched = ActionLookaheadScheduler(la, [0, 1], policy, 3, base=("sjfcp", 0))
    assert sched._cand["policy"].tolist() == [4, 4, 4] and sched._cand["first_policy"].tolist() == [4, 4, 4] and sched.children == list(range(2, 8))
    # ... and what tests/fused_decima_util.py pins of the policy lookahead stays so
    with pytest.raises(ValueError, match="cannot be combined with a horizon"):
        LookaheadScheduler(la, [0], [("fair", 0), ("decima", 0)], decima=policy, horizon=1e5)
    la.close(), env.close()
    # an env whose node slots do not leave room for both working sets in one workgroup: refused with policy arguments, taken without
    big = make_env({**TINY, "job_arrival_cap": 500}, 1, pack, device, lib)
    big.reset(seed=[1])
    held = batch_bytes(big)
    one, m1 = i32(big, [0]), i32(big, [-1])
    with pytest.raises(ValueError, match="LDS working set does not fit"):
        make_policy(TINY, device).rollout_action_env(big, 5, one, m1)
    assert differing(held, batch_bytes(big)) == []
    assert big.rollout_action(one, one, 3, one, one * 0)["steps"].tolist() == [3]
    big.close()


def check_heuristic_base_and_evaluation(pack, device, lib) -> None:
    """`base` may be a heuristic (the kernel without policy arguments), and evaluation.run_lookahead takes the new scheduler"""
    P, k = 2, 2
    policy = make_policy(TINY, device)
    env = make_env(TINY, P * (1 + k), pack, device, lib)
    sched = ActionLookaheadScheduler(env, [0, 1], policy, k, base=("fair", 0), max_steps=6)
    r = evaluation.run_lookahead(env, sched, [3, 4], check_every=3)
    assert sched.decisions == 6 and r["steps"].tolist() == [6, 6] and r["winners"].shape == (6, P)
    assert (sched.parent_out["steps"][:P] == 1).all()
    env.close()
