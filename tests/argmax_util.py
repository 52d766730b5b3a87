"""shared by the emulator and GPU arg-max tests (test_emu_argmax.py, test_gpu_argmax.py): sss_decima_argmax (the arg-max
instantiation of sss_decima_sample's two kernels, csrc/sss_decima_policy.h) on synthetic score tables - driven as sampler_util's
SampleRig drives the draws - and the greedy routes of DecimaPolicy on live envs."""
import ctypes

import numpy as np
import torch

from sampler_util import SampleRig, check_lgprob, log_softmax64

STAGE_COUNTS = (1, 2, 63, 64, 65, 130, 200)
EXEC_COUNTS = (1, 10, 64, 65, 128)
NEG = -np.inf


class ArgmaxRig(SampleRig):
    """SampleRig with sss_decima_argmax in place of sss_decima_sample (the seed and the counter are ignored by it)"""

    def _launch(self, which):
        stream = torch.cuda.current_stream(self.dev).cuda_stream if self.dev.type == "cuda" else 0
        self.b.check(self.b.lib.sss_decima_argmax(self.B, which, ctypes.byref(self.a), stream))


def argmax_candidates(scores, sched=None):
    """index of the first largest score among the candidates (schedulable, not -inf, not NaN), or -1"""
    s = np.asarray(scores, np.float32).astype(np.float64)
    ok = ~np.isnan(s) & (s != NEG)
    if sched is not None:
        ok &= np.asarray(sched, bool)
    if not ok.any():
        return -1
    return int(np.argmax(np.where(ok, s, NEG)))  # (np.argmax: the first of equal maxima)


def run_stage(binding, device, scores, sched=None, B=3, **kw):
    """the stage arg-max alone over B identical envs: (node index chosen or -1, the result dict rows [B])"""
    n = len(scores)
    sched_a = np.ones(n, bool) if sched is None else np.asarray(sched, bool)
    r = ArgmaxRig(binding, device, scores, B, exec_scores=np.zeros(1, np.float32), sched=sched, **kw).run(0, [0], exec=False)
    r = {k: v[0] for k, v in r.items()}
    cand = np.flatnonzero(sched_a)
    assert (r["stage_sel"] == r["stage_sel"][0]).all() and (r["any_stage"] == r["any_stage"][0]).all()
    node = int(cand[r["stage_sel"][0]]) if r["any_stage"][0] else -1
    return node, r


def run_exec(binding, device, es, B=3):
    """the executor-count arg-max alone (any_stage preset to 1, lgprob to 0)"""
    r = ArgmaxRig(binding, device, np.zeros(1, np.float32), B, exec_scores=es).run(0, [0], stage=False)
    r = {k: v[0] for k, v in r.items()}
    assert (r["exec_sel"] == r["exec_sel"][0]).all() and (r["num_exec"] == r["exec_sel"] + 1).all()
    return int(r["exec_sel"][0]), r


def check_random_scores(binding, device):
    """random float32 scores at every size: the selection is np.argmax over the candidates, lgprob within sampler_util.lgprob_tol
    of the fp64 log-softmax, and on the rows where the sampler draws the same index its lgprob has the same bits"""
    rng = np.random.default_rng(5)
    same_rows = 0
    for n in STAGE_COUNTS:
        s = rng.normal(0.0, 1.5, n).astype(np.float32)
        sched = np.ones(n, bool)
        if n > 2:
            sched[rng.integers(0, n, n // 4)] = False
            s[~sched] = 40.0  # stale finite scores outside the schedulable stages
        want = argmax_candidates(s, sched)
        node, r = run_stage(binding, device, s, sched)
        assert node == want, (n, node, want)
        live = np.where(sched, s, NEG)
        check_lgprob(r["lgprob"], log_softmax64(live)[want], int(sched.sum()), what=("stage", n))
        assert (r["stage_idx"] == r["stage_sel"]).all() and (r["job_idx"] == 0).all() and (r["job_gid"] == np.arange(len(r["job_gid"]))).all()
        d = SampleRig(binding, device, s, 16, exec_scores=np.zeros(1, np.float32), sched=sched).run(11, range(8), exec=False)
        hit = np.flatnonzero(sched)[d["stage_sel"]] == want
        assert (d["lgprob"][hit].view(np.uint32) == r["lgprob"][0].view(np.uint32)).all(), ("stage lgprob bits", n)
        same_rows += int(hit.sum())
    for E in EXEC_COUNTS:
        es = rng.normal(0.0, 1.5, E).astype(np.float32)
        if E > 2:
            es[rng.integers(0, E, E // 4)] = NEG
        want = argmax_candidates(es)
        c, r = run_exec(binding, device, es)
        assert c == want, (E, c, want)
        check_lgprob(r["lgprob"], 0.0, 0, log_softmax64(es)[want], int(np.isfinite(es).sum()), what=("exec", E))
        d = SampleRig(binding, device, np.zeros(1, np.float32), 16, exec_scores=es).run(12, range(8), stage=False)
        hit = d["exec_sel"] == want
        assert (d["lgprob"][hit].view(np.uint32) == r["lgprob"][0].view(np.uint32)).all(), ("exec lgprob bits", E)
        same_rows += int(hit.sum())
    assert same_rows >= 2 * 128  # (n = 1 and E = 1 alone give that many rows with the same selection)


def check_both_decisions(binding, device):
    """both launches behind each other: the executor scores of the chosen stage's job, lgprob the sum of the two terms"""
    rng = np.random.default_rng(6)
    n, E, J = 130, 65, 4
    s = rng.normal(0.0, 1.0, n).astype(np.float32)
    node_job = np.arange(n) * J // n
    es = rng.normal(0.0, 1.0, (J, E)).astype(np.float32)
    es[:, 40:] = NEG
    r = ArgmaxRig(binding, device, s, 5, exec_scores=es, node_job=node_job, n_jobs=J).run(0, [0])
    r = {k: v[0] for k, v in r.items()}
    want = argmax_candidates(s)
    j = int(node_job[want])
    c = argmax_candidates(es[j])
    assert (r["stage_sel"] == want).all() and (r["job_idx"] == j).all() and (r["exec_sel"] == c).all() and (r["num_exec"] == c + 1).all()
    assert (r["job_gid"] == np.arange(5) * J + j).all() and (r["any_stage"] == 1).all()
    check_lgprob(r["lgprob"], log_softmax64(s)[want], n, log_softmax64(es[j])[c], 40, what="both")


def check_ties(binding, device):
    """the tie rule: all candidates equal -> the lowest candidate; an equal maximum at i and i + 64 (the same lane, a later
    stride) and at i and i + 1 (neighbouring lanes) -> the lower one; -0.0 ties with +0.0"""
    for n in STAGE_COUNTS:
        for v in (0.0, -3.5, 1e4):
            sched = np.ones(n, bool)
            if n > 2:
                sched[0] = False  # the lowest slot is no candidate: the lowest CANDIDATE wins
            node, _ = run_stage(binding, device, np.full(n, v, np.float32), sched)
            assert node == int(np.flatnonzero(sched)[0]), (n, v, node)
    for E in EXEC_COUNTS:
        es = np.full(E, 0.25, np.float32)
        if E > 2:
            es[0] = NEG
        c, _ = run_exec(binding, device, es)
        assert c == int(np.flatnonzero(np.isfinite(es))[0]), (E, c)
    rng = np.random.default_rng(7)
    for n, i, step in ((130, 3, 64), (200, 70, 64), (200, 5, 128), (130, 17, 1), (65, 63, 1), (200, 127, 1), (2, 0, 1)):
        s = rng.normal(0.0, 1.0, n).astype(np.float32)
        s[i] = s[i + step] = 5.0
        node, _ = run_stage(binding, device, s)
        assert node == i, ("stage tie", n, i, step, node)
        # ... and in the other order of writing: a larger value later in the same lane / the next lane still wins
        s[i + step] = 5.5
        node, _ = run_stage(binding, device, s)
        assert node == i + step, ("stage later maximum", n, i, step, node)
    for E, i, step in ((128, 2, 64), (65, 0, 64), (128, 40, 1), (65, 63, 1), (10, 8, 1)):
        es = rng.normal(0.0, 1.0, E).astype(np.float32)
        es[i] = es[i + step] = 5.0
        c, _ = run_exec(binding, device, es)
        assert c == i, ("exec tie", E, i, step, c)
        es[i + step] = 5.5
        c, _ = run_exec(binding, device, es)
        assert c == i + step, ("exec later maximum", E, i, step, c)
    s = np.full(70, -1.0, np.float32)
    s[[4, 9]] = [-0.0, 0.0]
    assert run_stage(binding, device, s)[0] == 4
    s[[4, 9]] = [0.0, -0.0]
    assert run_stage(binding, device, s)[0] == 4
    es = np.full(70, -1.0, np.float32)
    es[[68, 3]] = [0.0, -0.0]
    assert run_exec(binding, device, es)[0] == 3


def check_masking(binding, device):
    """what must lose: a slot that is no schedulable stage holding +1e30, a -inf slot, a NaN candidate; nothing schedulable:
    stage_idx -1 and lgprob 0; no allowed count: num_exec 1 and lgprob untouched"""
    rng = np.random.default_rng(8)
    n = 130
    s = rng.normal(0.0, 1.0, n).astype(np.float32)
    sched = np.ones(n, bool)
    sched[[0, 64, 129]] = False
    s[[0, 64, 129]] = 1e30
    s[[1, 65]] = NEG
    want = argmax_candidates(s, sched)
    node, r = run_stage(binding, device, s, sched)
    assert node == want and sched[node] and np.isfinite(s[node])
    check_lgprob(r["lgprob"], log_softmax64(np.where(sched, s, NEG))[want], int((sched & np.isfinite(s)).sum()), what="masked")
    # a NaN never wins (it does poison the log-sum-exp, as it does the draw's: only the selection is defined)
    s2 = s.copy()
    s2[[2, 66]] = np.nan
    node, _ = run_stage(binding, device, s2, sched)
    assert node == argmax_candidates(s2, sched) and node not in (2, 66)
    only_nan = np.full(70, np.nan, np.float32)
    only_nan[69] = -7.0
    assert run_stage(binding, device, only_nan)[0] == 69
    es = rng.normal(0.0, 1.0, 65).astype(np.float32)
    es[[0, 64]] = np.nan
    es[5] = NEG
    assert run_exec(binding, device, es)[0] == argmax_candidates(es)
    # nothing schedulable
    stale = np.full(n, 30.0, np.float32)
    for kw in (dict(sched=np.zeros(n, bool)), dict(n_nodes=0), dict(scores=np.full(n, NEG, np.float32))):
        sc = kw.pop("scores", stale)
        r = ArgmaxRig(binding, device, sc, 4, exec_scores=np.zeros(10, np.float32), **kw).run(0, [0])
        r = {k: v[0] for k, v in r.items()}
        assert (r["any_stage"] == 0).all() and (r["stage_idx"] == -1).all() and (r["lgprob"] == 0.0).all(), kw
        assert (r["stage_sel"] == 0).all() and (r["job_idx"] == 0).all() and (r["job_gid"] == 0).all(), kw
        assert (r["exec_sel"] == 0).all() and (r["num_exec"] == 1).all(), kw
    # no allowed count: lgprob keeps the stage term's bits
    none = np.full(100, NEG, np.float32)
    alone = ArgmaxRig(binding, device, s, 4, exec_scores=none, sched=sched).run(0, [0], exec=False)
    r = ArgmaxRig(binding, device, s, 4, exec_scores=none, sched=sched).run(0, [0])
    assert (r["exec_sel"] == 0).all() and (r["num_exec"] == 1).all() and (r["any_stage"] == 1).all()
    assert np.array_equal(r["lgprob"].view(np.uint32), alone["lgprob"].view(np.uint32)) and np.isfinite(r["lgprob"]).all()


# ---- the greedy routes of DecimaPolicy on live envs ---------------------------------------------------------------------------
def greedy_env(device, lib):
    """4 envs, 10 executors, 20 jobs (the sizing of test_emu_decima.py's greedy test) and a Decima policy"""
    from decima_util import AGENT
    from spark_sched_sim_amd import VecSparkSchedSimEnv
    from spark_sched_sim_amd.decima import DecimaPolicy

    cfg = dict(num_executors=10, job_arrival_cap=20, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
    env = VecSparkSchedSimEnv(cfg, 4, device=device, auto_reset=True, _lib=lib)
    torch.manual_seed(3)
    policy = DecimaPolicy(num_executors=10, **AGENT).to(device).eval()
    env.reset(seed=70)
    return env, policy


def _first_argmax(row):
    row = np.asarray(row, np.float32)
    return argmax_candidates(row)


def check_policy_greedy(device, lib, steps=25, no_transfer=False):
    """`schedule_env(greedy=True)` against the kernels' own scores (`scores_out` of the same pass), `one_launch=True` against
    `act_env(want_scores=True)`; the draw counter `_calls` does not move and the sampled actions after the greedy calls are what
    they are without them; info["err"] stays clean. `no_transfer`: the on-device route runs under
    torch.cuda.set_sync_debug_mode("error")"""
    from spark_sched_sim_amd.binding import device_of

    env, policy = greedy_env(device, lib)
    policy.bind_kernels(env._b)
    assert policy._use_kernels() and env.graph_kernel_fits
    gen = torch.Generator(device=device)
    gen.manual_seed(9)
    policy.schedule_env(env, gen)  # one sampled step: sizes the work space and moves the counter off zero
    calls = policy._calls
    for t in range(steps):
        if no_transfer:
            torch.cuda.synchronize()
            prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                act, aux = policy.schedule_env(env, greedy=True)
            finally:
                torch.cuda.set_sync_debug_mode(prev)
        else:
            act, aux = policy.schedule_env(env, greedy=True)
        act = {k: v.clone() for k, v in act.items()}
        lg = aux["lgprob"].clone()
        assert policy._calls == calls
        # the kernels' scores of the same observations
        g = env.decima_graph_on_device()
        with device_of(g["x"].device):
            stream = torch.cuda.current_stream(g["x"].device).cuda_stream if g["x"].device.type == "cuda" else 0
            h = policy._encode_kernels(g, stream)
            so = {}
            ref = policy._sample_kernels(g, h, policy._stage_scores_kernels(g, h, stream), None, scores_out=so, _stream=stream, greedy=True)
        assert policy._calls == calls
        ss, es = so["stage_scores"].cpu().numpy(), so["exec_scores"].cpu().numpy()
        n_nodes = g["obs_nodes"].cpu().numpy()
        off = g["obs_node_off"].cpu().numpy()
        rank = g["sched_rank"].cpu().numpy()
        for b in range(env.num_envs):
            row = ss[b, : n_nodes[b]]
            rk = rank[off[b]: off[b] + n_nodes[b]]
            want = argmax_candidates(row, rk >= 0)
            if want < 0:
                assert int(act["stage_idx"][b]) == -1 and int(act["num_exec"][b]) == 1
                continue
            assert int(act["stage_idx"][b]) == int(rk[want]), (t, b)
            c = _first_argmax(es[b])
            assert int(act["num_exec"][b]) == (c + 1 if c >= 0 else 1), (t, b)
            n_c = int(((rk >= 0) & np.isfinite(row)).sum())
            check_lgprob(np.array([float(lg[b])]), log_softmax64(np.where(rk >= 0, row, NEG))[want], n_c,
                         log_softmax64(es[b])[c] if c >= 0 else 0.0, int(np.isfinite(es[b]).sum()), what=("pipeline", t, b))
        assert torch.equal(ref["env_stage_idx"], act["stage_idx"]) and torch.equal(ref["env_num_exec"], act["num_exec"])
        # the one-launch kernel against its own scores
        act1, aux1 = policy.schedule_env(env, greedy=True, one_launch=True)
        assert policy._calls == calls
        act1 = {k: v.clone() for k, v in act1.items()}
        _, ak = policy.act_env(env, 0, want_scores=True, greedy=True)
        ss1, es1 = ak["stage_scores"].cpu().numpy(), ak["exec_scores"].cpu().numpy()
        for b in range(env.num_envs):
            fin = np.flatnonzero(ss1[b] != NEG)
            if fin.size == 0:
                assert int(act1["stage_idx"][b]) == -1
                continue
            want = argmax_candidates(ss1[b])
            assert int(act1["stage_idx"][b]) == int(np.searchsorted(fin, want)), (t, b)
            c = _first_argmax(es1[b])
            assert int(act1["num_exec"][b]) == (c + 1 if c >= 0 else 1), (t, b)
            check_lgprob(np.array([float(ak["lgprob"][b])]), log_softmax64(ss1[b])[want], fin.size,
                         log_softmax64(es1[b])[c] if c >= 0 else 0.0, int(np.isfinite(es1[b]).sum()), what=("one launch", t, b))
        obs, r, term, trunc, info = env.step(act)
        assert not info["err"].any()
    # the sampled stream is where it was: the next draw uses counter calls + 1
    _, a = policy.schedule_env(env, gen)
    assert policy._calls == calls + 1 and a["rng"][1] == calls + 1
    env.close()
