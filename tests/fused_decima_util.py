"""The checks of the fused Decima rollout (include/sss.h sss_rollout_decima; DecimaPolicy.rollout_env, evaluation.run_episodes and
evaluation.continuations with fused=True, lookahead.LookaheadScheduler with a Decima candidate), shared by
tests/test_emu_fused_decima.py (the CPU wave emulator) and tests/test_gpu_fused_decima.py (the kernels). Every check takes
(device, lib): ("cpu", the emulator's library) or ("cuda:0", None). What the new path is held to is the existing ones - `act_env` +
`step_async` in lock step, `env.rollout_each`, `fork`, `job_stats` - bit for bit on the envs' bytes with the tick counters masked.
There are no tolerances. The weights are the reference's published model (tests/golden/decima_reference_model.npz): a randomly
initialised policy has near-tied scores."""
from __future__ import annotations

import collections
import os.path as osp

import numpy as np
import torch

from decima_util import AGENT
from fork_util import SKIP, TINY, env_bytes, same_bytes
from golden_util import GOLDEN_DIR
from lookahead_util import i32, live_image, no_ticks, per_env
from spark_sched_sim_amd import VecSparkSchedSimEnv, evaluation
from spark_sched_sim_amd.binding import POLICY_DECIMA, POLICY_IDS
from spark_sched_sim_amd.decima import DecimaPolicy
from spark_sched_sim_amd.lookahead import LookaheadScheduler
from spark_sched_sim_amd.vec_env import HDR_OFF, HDR_PROF

WIDE = {**TINY, "num_executors": 100}
CONFIGS = {"narrow": TINY, "wide": WIDE}
# Where the compared stretch starts and how long it is. An episode of these configs takes 70 to 400 steps and the emulator plays
# about 50 steps of 8 envs a second, so the envs first play under the fair heuristic (existing paths): all of them `prefix` steps,
# the envs of `late` another `extra`. The `steps` steps after that are compared: the early envs then hold the largest observations
# (more than 64 nodes; at 100 executors more than 64 committable ones), the late ones reach the end of their episodes.
STRETCH = {"narrow": dict(seeds=list(range(21, 29)), prefix=20, late=(1, 3, 5), extra=40, steps=60),
           "wide": dict(seeds=list(range(1, 9)), prefix=10, late=(1, 5, 6), extra=150, steps=60)}
SEED, COUNTER0 = 5, 1000  # of the sampled runs: the draws' seed and the counter of the stretch's first step


def make_policy(cfg: dict, device) -> DecimaPolicy:
    z = np.load(osp.join(GOLDEN_DIR, "decima_reference_model.npz"))
    policy = DecimaPolicy(num_executors=cfg["num_executors"], **AGENT).eval()
    policy.load_state_dict(collections.OrderedDict((k, torch.from_numpy(z[k])) for k in z.files))
    return policy.to(device)


def make_env(cfg: dict, n: int, pack, device, lib) -> VecSparkSchedSimEnv:
    return VecSparkSchedSimEnv(cfg, n, device=device, pack=pack, _lib=lib)


def prepared(which: str, pack, device, lib) -> VecSparkSchedSimEnv:
    s = STRETCH[which]
    env = make_env(CONFIGS[which], len(s["seeds"]), pack, device, lib)
    env.reset(seed=s["seeds"])
    env.rollout("fair", s["prefix"])
    pol, par = per_env(env, {e: ("fair", 0) for e in s["late"]})
    env.rollout_each(pol, par, s["extra"])
    return env


def batch_bytes(env) -> dict[str, np.ndarray]:
    """everything the envs own, one row per env, without the header's shader-clock counters (lookahead_util.no_ticks for all envs)"""
    out = {"state": env._env_view, "nodes": env.nodes, "edge_links": env.edge_links, "dag_ptr": env.dag_ptr, "exec_supplies": env.exec_supplies,
           "obs_i32": env.obs_i32, "obs_f64": env.obs_f64}
    out = {k: v.cpu().numpy().copy().reshape(env.num_envs, -1).view(np.uint8) for k, v in out.items()}
    out["state"][:, HDR_PROF: HDR_PROF + 40] = 0
    return out


def image(env, e: int) -> dict:
    """lookahead_util.live_image without the header's three event-loop census counters (n_fast, n_batched, n_rounds: how many fast
    runs, batches and rounds the env's event loop took). Like the commitment entries behind the live ones they show where the launch
    boundaries were - a round ends with its launch - and belong to no state: the heuristics' `rollout_each(n)` and n x
    `rollout_each(1)` differ in them just the same at 100 executors. For comparisons between DIFFERENT splits into launches only."""
    b = live_image(env, e)
    b["state"][HDR_OFF["n_fast"]: HDR_OFF["n_rounds"] + 8] = 0
    return b


def differing(a: dict, b: dict) -> list[tuple[str, int]]:
    return [(k, e) for k in a for e in range(a[k].shape[0]) if not np.array_equal(a[k][e], b[k][e])]


def dag_depth(env, e: int) -> int:
    """edges on the longest path of env e's observed graph"""
    n, ne = int(env.obs_i32[e, 0]), int(env.obs_i32[e, 1])
    el = env.edge_links[e, :ne].cpu().numpy()
    gen = np.zeros(max(n, 1), dtype=np.int64)
    for _ in range(n + 1):
        moved = False
        for u, v in el:
            if gen[v] < gen[u] + 1:
                gen[v], moved = gen[u] + 1, True
        if not moved:
            break
    return int(gen.max())


def live_mask(env) -> torch.Tensor:
    return (env.obs_i32[:, 6] == 0) & (env.obs_i32[:, 7] == 0)


# ---- 1. one launch equals many ---------------------------------------------------------------------

def check_one_launch_equals_many(which: str, greedy: bool, pack, device, lib) -> None:
    cfg, N = CONFIGS[which], STRETCH[which]["steps"]
    policy = make_policy(cfg, device)
    a, b = prepared(which, pack, device, lib), prepared(which, pack, device, lib)
    before = a.header_field("ep_steps").clone()
    out = policy.rollout_env(a, N, greedy=greedy, seed=SEED, counter=COUNTER0)
    last = {k: policy._ws[k].clone() for k in ("stage_idx", "num_exec")}  # the hand-over arrays hold every env's last decision
    steps = torch.zeros_like(out["steps"])
    first = None
    for t in range(N):
        one = policy.rollout_env(b, 1, greedy=greedy, seed=SEED, counter=COUNTER0 + t)
        first = first or {k: v.clone() for k, v in one.items()}
        steps += one["steps"]
    print(which, "greedy" if greedy else "sampled", "steps:", out["steps"].tolist())
    assert torch.equal(out["steps"], steps) and torch.equal(out["steps"], a.header_field("ep_steps") - before)
    assert torch.equal(out["first_stage_idx"], first["first_stage_idx"]) and torch.equal(out["first_num_exec"], first["first_num_exec"])
    assert (out["steps"] < N).any() and (out["steps"] == N).any(), "want an episode that ends inside the launch and one that does not"
    assert bool((a.header_field("terminated")[out["steps"] < N] == 1).all()) and bool((a.obs_i32[:, 7] == 0).all())
    assert torch.equal(last["stage_idx"], policy._ws["stage_idx"]) and torch.equal(last["num_exec"], policy._ws["num_exec"])
    for e in range(a.num_envs):
        bad = same_bytes(image(a, e), image(b, e))
        assert bad == [], f"env {e}: one launch of {N} steps and {N} launches of one differ in {bad}"
    a.close(), b.close()


# ---- 2. + 3. every decision is the lock-step kernel's, and the strides really ran ------------------

def check_decisions_equal_lock_step(which: str, greedy: bool, pack, device, lib) -> None:
    cfg, N = CONFIGS[which], STRETCH[which]["steps"]
    E = cfg["num_executors"]
    policy = make_policy(cfg, device)
    a, b = prepared(which, pack, device, lib), prepared(which, pack, device, lib)
    B = a.num_envs
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=a.device)
    assert differing(batch_bytes(a), batch_bytes(b)) == []
    seen = dict(nodes=0, depth=0, commit=0, ended=0, decisions=0)
    for t in range(N):
        live = live_mask(b)
        assert torch.equal(live, live_mask(a))
        if not bool(live.any()):
            break
        oi = b.obs_i32.cpu().numpy()
        lv = live.cpu().numpy()
        big = int(np.argmax(np.where(lv, oi[:, 0], -1)))
        seen["nodes"] = max(seen["nodes"], int(oi[big, 0]))
        if oi[big, 0] > 64:
            seen["depth"] = max(seen["depth"], dag_depth(b, big))
        seen["commit"] = max(seen["commit"], int(np.where(lv, oi[:, 4], 0).max()))
        act, _ = policy.act_env(b, COUNTER0 + t, seed=SEED, greedy=greedy)
        want_si, want_ne = act["stage_idx"].clone(), act["num_exec"].clone()
        b.step_async(torch.where(live, want_si, skip).contiguous(), want_ne)
        got = policy.rollout_env(a, 1, greedy=greedy, seed=SEED, counter=COUNTER0 + t)
        assert got["steps"].tolist() == live.to(torch.int32).tolist()
        assert torch.equal(got["first_stage_idx"][live], want_si[live]) and torch.equal(got["first_num_exec"][live], want_ne[live]), \
            f"step {t}: the fused kernel decided {got['first_stage_idx'].tolist()} / {got['first_num_exec'].tolist()}, act_env {want_si.tolist()} / {want_ne.tolist()}"
        bad = differing(batch_bytes(a), batch_bytes(b))
        assert bad == [], f"step {t}: (buffer, env) that differ from act_env + step: {bad}"
        seen["decisions"] += int(live.sum())
        seen["ended"] += int((live & ~live_mask(b)).sum())
    print(which, "greedy" if greedy else "sampled", seen)
    # the strides really ran: more nodes than lanes on a graph with layers, an episode's end, and - wide - more counts than lanes
    assert seen["nodes"] > 64 and seen["depth"] >= 2, seen
    assert seen["ended"] >= 1, seen
    if E > 64:
        assert seen["commit"] > 64, seen
    a.close(), b.close()


# ---- 4. per-env policies -----------------------------------------------------------------------------

def check_per_env_policies(which: str, pack, device, lib) -> None:
    cfg, n = CONFIGS[which], 30
    policy = make_policy(cfg, device)
    a, ref = prepared(which, pack, device, lib), prepared(which, pack, device, lib)
    B = a.num_envs
    assert B == 8
    D, F, S = POLICY_DECIMA, POLICY_IDS["fair"], POLICY_IDS["sjfcp"]
    #            0   1   2  3  4  5  6  7
    pol = i32(a, [-1, -1, F, S, D, D, F, 9])
    par = i32(a, [0, 0, 0, 0, 77, 0, 0, 0])  # (Decima's param is ignored)
    fpol = i32(a, [-1, -1, -1, -1, -1, S, D, -1])
    fpar = i32(a, [0] * 8)
    held = {e: env_bytes(a, e) for e in (0, 1, 7)}
    before = a.header_field("ep_steps").tolist()
    out = policy.rollout_env(a, n, greedy=True, policy=pol, param=par, first_policy=fpol, first_param=fpar)
    for e in (0, 1, 7):
        assert same_bytes(held[e], env_bytes(a, e)) == [], f"env {e} sits out (or has a bad id) and changed"
    assert out["steps"].tolist()[:2] == [0, 0] and int(out["steps"][7]) == -1 and (out["first_stage_idx"][[0, 1, 7]] == -1).all()
    # the expectation of every env that played, from existing calls, on the twin
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=a.device)

    def decima_steps(ids, k):
        sel = torch.zeros(B, dtype=torch.bool)
        sel[list(ids)] = True
        sel = sel.to(ref.device)
        firsts = None
        for _ in range(k):
            act, _ = policy.act_env(ref, 0, greedy=True)
            live = sel & live_mask(ref)
            firsts = firsts or (act["stage_idx"].clone(), act["num_exec"].clone())
            ref.step_async(torch.where(live, act["stage_idx"], skip).contiguous(), act["num_exec"])
        return firsts

    h_pol, h_par = per_env(ref, {2: ("fair", 0), 3: ("sjfcp", 0)})
    h = ref.rollout_each(h_pol, h_par, n)
    d4 = decima_steps([4], n)
    p5, q5 = per_env(ref, {5: ("sjfcp", 0)})
    h5 = ref.rollout_each(p5, q5, 1)
    decima_steps([5], n - 1)
    d6 = decima_steps([6], 1)
    p6, q6 = per_env(ref, {6: ("fair", 0)})
    ref.rollout_each(p6, q6, n - 1)
    for e in (2, 3, 4, 5, 6):
        bad = same_bytes(image(ref, e), image(a, e))
        assert bad == [], f"env {e}: {bad}"
        assert int(out["steps"][e]) == ref.header(e)["ep_steps"] - before[e] > 0
    want_first = {2: (h["first_stage_idx"][2], h["first_num_exec"][2]), 3: (h["first_stage_idx"][3], h["first_num_exec"][3]), 4: (d4[0][4], d4[1][4]),
                  5: (h5["first_stage_idx"][5], h5["first_num_exec"][5]), 6: (d6[0][6], d6[1][6])}
    for e, (si, ne) in want_first.items():
        assert int(out["first_stage_idx"][e]) == int(si) and int(out["first_num_exec"][e]) == int(ne), f"env {e}: first action"
    a.close(), ref.close()


# ---- 5. the lookahead with a Decima candidate --------------------------------------------------------

LA_CANDIDATES = [("fair", 0), ("sjfcp", 0), ("decima", 0)]


def compose_decision(env, policy, parents, kids, base, max_steps=5000):
    """one decision of the scheduler written with the calls that existed before it knew Decima: fork; candidate k's children take
    candidate k's first step and then the base's (or k's own) to the end - a heuristic by rollout_each, Decima by act_env(greedy) +
    step in lock step -; job_stats column 1; arg-min with ties to the lowest k; the parents take the winner's step. Returns the winners."""
    B, P, K = env.num_envs, len(parents), len(LA_CANDIDATES)
    skip = torch.full((B,), SKIP, dtype=torch.int32, device=env.device)

    def play(ids, name, param, n):
        if n <= 0:
            return
        if name != "decima":
            pol, par = per_env(env, {e: (name, param) for e in ids})
            env.rollout_each(pol, par, n)
            return
        sel = torch.zeros(B, dtype=torch.bool)
        sel[list(ids)] = True
        sel = sel.to(env.device)
        for t in range(n):
            live = sel & live_mask(env)
            if t % 16 == 0 and not bool(live.any()):
                break
            act, _ = policy.act_env(env, 0, greedy=True)
            env.step_async(torch.where(live, act["stage_idx"], skip).contiguous(), act["num_exec"])

    cost = np.full((P, K), np.nan)
    for k, (name, param) in enumerate(LA_CANDIDATES):
        ids = [int(c) for c in kids[:, k, 0]]
        env.fork(parents, ids)
        play(ids, name, param, 1)
        after = base or (name, param)
        play(ids, after[0], after[1], max_steps)
        stats = env.job_stats()["stats"].cpu().numpy()
        ok = ((env.header_field("terminated") != 0) & (env.header_field("err") == 0)).cpu().numpy()
        cost[:, k] = np.where(ok[ids], stats[ids, 1], np.nan)
    best = [int(np.nanargmin(cost[i])) for i in range(P)]  # (the first of equal minima)
    for k, (name, param) in enumerate(LA_CANDIDATES):
        play([p for i, p in enumerate(parents) if best[i] == k], name, param, 1)
    return best, cost


def check_lookahead_first_decisions(base, decisions: int, pack, device, lib) -> None:
    P, K = 2, len(LA_CANDIDATES)
    B = P * (1 + K)
    parents, kids = list(range(P)), np.arange(P, B).reshape(P, K, 1)
    policy = make_policy(TINY, device)
    env, ref = make_env(TINY, B, pack, device, lib), make_env(TINY, B, pack, device, lib)
    seeds = [3, 4] + [0] * (B - P)
    for e in (env, ref):
        e.reset(seed=seeds)
        e.rollout("fair", 30)  # (a state with several jobs: the candidates disagree there)
    sched = LookaheadScheduler(env, parents, LA_CANDIDATES, base=base, decima=policy)
    winners = []
    for d in range(decisions):
        sched.decide_and_step()
        best, cost = compose_decision(ref, policy, parents, kids, base)
        got = sched.last_scores.cpu().numpy()
        assert np.array_equal(got.view(np.uint64), cost.view(np.uint64)), (d, got, cost)
        assert sched.last_best.tolist() == best, (d, sched.last_best.tolist(), best)
        assert (sched.parent_out["steps"][:P] == 1).all()
        for p in parents:
            bad = same_bytes(image(ref, p), image(env, p))
            assert bad == [], f"decision {d}, parent {p}: {bad}"
        winners.append(best)
    print("base", base, "winners", winners)
    env.close(), ref.close()


def check_lookahead_never_ends_above_a_candidate(pack, device, lib) -> None:
    """whole episodes (the GPU's share): with deterministic children every policy is a function of the state - Decima's arg-max
    included - so the parents end at or below every candidate's own episode from the same seeds; likewise over Decima as the base"""
    seeds = [0, 1]
    P, K = len(seeds), len(LA_CANDIDATES)
    policy = make_policy(TINY, device)
    solo = make_env(TINY, P, pack, device, lib)
    own = {}
    for name, param in LA_CANDIDATES:
        r = evaluation.run_episodes(solo, policy, seeds, greedy=True, fused=True, chunk=5000) if name == "decima" else evaluation.run_episodes(solo, name, seeds, param=param)
        assert bool(r["ok"].all()), f"{name} ended in an env error"
        own[name] = r["total_job_time"].cpu().numpy()
    solo.close()
    env = make_env(TINY, P * (1 + K), pack, device, lib)
    for base in (None, ("decima", 0)):
        r = evaluation.run_lookahead(env, LookaheadScheduler(env, list(range(P)), LA_CANDIDATES, base=base, decima=policy), seeds, check_every=32)
        assert bool(r["ok"].all()) and r["fallbacks"] == 0
        total = r["total_job_time"].cpu().numpy()
        print("base", base, "own:", {k: v.tolist() for k, v in own.items()}, "lookahead:", total.tolist())
        for name, v in own.items():
            if base is None or name == "decima":
                assert (total <= v).all(), (base, name, total, v)
    env.close()


# ---- 6. run_episodes(fused=True) and continuations(policy=<DecimaPolicy>) ----------------------------

def check_run_episodes(which: str, max_steps: int, pack, device, lib) -> None:
    """the per-env job statistics of fused greedy episodes are those of the lock-step one_launch=True ones; `max_steps` bounds both
    (the emulator plays a stretch, the GPU whole episodes)"""
    cfg = CONFIGS[which]
    policy = make_policy(cfg, device)
    a, b = make_env(cfg, 4, pack, device, lib), make_env(cfg, 4, pack, device, lib)
    seeds = [11, 12, 13, 14]
    ra = evaluation.run_episodes(a, policy, seeds, max_steps=max_steps, greedy=True, fused=True, chunk=max(1, max_steps // 2 + 1))
    b.reset(seed=seeds)
    skip = torch.full((4,), SKIP, dtype=torch.int32, device=b.device)
    for t in range(max_steps):
        live = live_mask(b)
        if t % 32 == 0 and not bool(live.any()):
            break
        act, _ = policy.schedule_env(b, one_launch=True, greedy=True)
        b.step_async(torch.where(live, act["stage_idx"], skip).contiguous(), act["num_exec"])
    rb = evaluation._summarize(b, (25, 50, 75, 100))
    assert set(ra) == set(rb)
    for k in ra:
        x, y = ra[k].cpu().numpy(), rb[k].cpu().numpy()
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    print(which, "steps", ra["steps"].tolist(), "ok", ra["ok"].tolist())
    a.close(), b.close()


def check_continuations(pack, device, lib) -> None:
    policy = make_policy(TINY, device)
    env = prepared("narrow", pack, device, lib)
    ref = prepared("narrow", pack, device, lib)
    held = {e: env_bytes(env, e) for e in (0, 1, 2, 3, 6, 7)}
    r = evaluation.continuations(env, [0, 1], [4, 5], policy, max_steps=3000, fused=True)
    assert bool(r["ok"].all())
    for e in held:
        assert same_bytes(held[e], env_bytes(env, e)) == [], f"env {e} took no part and changed"
    ref.fork([0, 1], [4, 5])
    pol = i32(ref, [-1, -1, -1, -1, POLICY_DECIMA, POLICY_DECIMA, -1, -1])
    policy.rollout_env(ref, 3000, greedy=True, policy=pol, param=i32(ref, [0] * 8))
    want = ref.job_stats()["stats"][[4, 5]].cpu().numpy()
    assert np.array_equal(r["total_job_time"].cpu().numpy().view(np.uint64), want[:, 1].view(np.uint64))
    env.close(), ref.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------

def check_refusals(pack, device, lib) -> None:
    import ctypes as C

    import pytest
    from spark_sched_sim_amd import binding as B
    from spark_sched_sim_amd.binding import SssDecimaPolicyArgs

    policy = make_policy(TINY, device)
    env = make_env(TINY, 4, pack, device, lib)
    env.reset(seed=[51, 52, 53, 54])
    L = env._b.lib
    assert "sss_rollout_decima" in B.EXPORTS and hasattr(L, "sss_rollout_decima") and B.POLICY_DECIMA == 5 and "decima" not in B.POLICY_IDS
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

    def call(a, pol=None, par=None, fpol=None, fpar=None, n=5):
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return L.sss_rollout_decima(env._h, C.byref(a) if a is not None else None, 1, ptr(pol), ptr(par), ptr(fpol), ptr(fpar), n, None, None, None, None)

    def refused(rc, message):
        assert rc == -55 and message in L.sss_last_error().decode(), (rc, L.sss_last_error().decode())

    some = i32(env, [0, 0, 0, 0])
    nonnull = ws["lgprob"].data_ptr()
    refused(call(None), "policy arguments are NULL")
    for f in ("w_prep_dev", "w_msg_dev", "w_upd_dev", "w_dag_dev", "w_glob_dev", "w_stage_dev", "w_exec_dev"):
        refused(call(args(**{f: None})), "weight pointer")
    for f in ("node_scratch_dev", "job_scratch_dev"):
        refused(call(args(**{f: None})), "scratch")
    for f in ("stage_idx_dev", "num_exec_dev", "stage_sel_dev", "job_idx_dev", "exec_sel_dev", "lgprob_dev"):
        refused(call(args(**{f: None})), "output pointer")
    refused(call(args(active_dev=nonnull)), "active_dev must be NULL")
    refused(call(args(stage_scores_dev=nonnull)), "must be NULL")
    refused(call(args(exec_scores_dev=nonnull)), "must be NULL")
    refused(call(args(prof_dev=nonnull)), "prof_dev must be NULL")
    refused(call(args(), pol=some), "policy_dev and param_dev come together")
    refused(call(args(), fpol=some), "first_policy_dev and first_param_dev come together")
    refused(call(args(), fpar=some), "first_policy_dev and first_param_dev come together")
    refused(call(args(), n=-1), "n_steps must be >= 0")
    with pytest.raises(ValueError, match="n_steps must be >= 0"):
        policy.rollout_env(env, -1)
    with pytest.raises(ValueError, match="together"):
        policy.rollout_env(env, 5, policy=some)
    with pytest.raises(ValueError, match="together"):
        policy.rollout_env(env, 5, first_param=some)
    with pytest.raises(ValueError, match="int32"):
        policy.rollout_env(env, 5, policy=some.long(), param=some)
    env.enable_timeline(8)
    with pytest.raises(ValueError, match="not available while a timeline is recorded"):
        policy.rollout_env(env, 5)
    env.disable_timeline()
    assert differing(whole, batch_bytes(env)) == [], "a refused call touched an env"
    # the existing entry points go on refusing the id and the name
    five = i32(env, [5, 5, 5, 5])
    assert env.rollout_each(five, some, 5)["steps"].tolist() == [-1] * 4
    assert env.rollout_until(five, some, float("inf"), 5)["steps"].tolist() == [-1] * 4
    assert L.sss_policy(env._h, 5, 0, ws["stage_idx"].data_ptr(), ws["num_exec"].data_ptr(), None) != 0
    for call_ in (lambda: env.policy_actions("decima"), lambda: env.rollout("decima", 5)):
        with pytest.raises(KeyError):
            call_()
    assert differing(whole, batch_bytes(env)) == []
    # the scheduler's arguments
    la = make_env(TINY, 8, pack, device, lib)
    with pytest.raises(ValueError, match="needs decima="):
        LookaheadScheduler(la, [0], LA_CANDIDATES)
    with pytest.raises(ValueError, match="needs decima="):
        LookaheadScheduler(la, [0], [("fair", 0), ("sjfcp", 0)], base=("decima", 0))
    with pytest.raises(ValueError, match="cannot be combined with a horizon"):
        LookaheadScheduler(la, [0], LA_CANDIDATES, decima=policy, horizon=1e5)
    with pytest.raises(ValueError, match="fused=True"):
        evaluation.continuations(la, [0], [1], policy)
    sched = LookaheadScheduler(la, [0], LA_CANDIDATES, decima=policy, base=("decima", 0))
    assert sched._cand["first_policy"].tolist() == [0, 4, 5] and sched._cand["policy"].tolist() == [5, 5, 5]
    la.close(), env.close()
    # an env whose node slots do not leave room for both working sets in one workgroup
    big = make_env({**TINY, "job_arrival_cap": 500}, 1, pack, device, lib)
    big.reset(seed=[1])
    held = batch_bytes(big)
    with pytest.raises(ValueError, match="LDS working set does not fit"):
        make_policy(TINY, device).rollout_env(big, 5)
    assert differing(held, batch_bytes(big)) == []
    big.close()
