"""shared by tests/test_emu_inference_fp64.py (CPU, emulator library) and tests/test_gpu_inference_fp64.py: Decima's INFERENCE forward pass
on the hand-written kernels - every route `DecimaPolicy` has to an embedding or a score - against the same forward pass in fp64 on the
CPU: a deep copy of the policy taken before `bind_kernels`, `.double()`, whose `encode` / `stage_scores` / `exec_scores` (over all jobs)
run on the env's graph moved to the CPU with `x` as fp64. That reference uses no kernel entry point. The second reference is the same
three calls in fp32 tensor ops on the test's device; its error against fp64, measured in the same run, sizes the tolerances (`compare`).

Routes (each on the same graph, against the same reference; `ROUTES` below):
  one_call_mode1 / one_call_mode2    `_encode_one_call` (sss_gnn_encode) with `_layers_mode` 1 (a launch per layer) / 2 (all layers in one launch)
                                     (with the graph kernel's own lists present nothing the host can see tells the two apart: that the
                                     library honoured mode 2 is taken from the stale-lists run below, and `expected_skips` fails a
                                     matrix-core build that falls back)
  launches                           the launch-by-launch path of `_encode_kernels`: the graph dict without `max_depth`
  stale_lists_mode1 / _mode2         the graph without its `_layer_lists`: the scan + list kernel runs inside sss_gnn_encode (mode 1); mode 2 needs
                                     no lists - which is how a build WITHOUT the one-launch kernel (emulator, vecforms: it falls back to the launches
                                     per layer, and those build the lists) is told from one with it
  capacity                           the capacity graph `env.decima_graph_on_device()`: leading `totals_dev` rows of the embeddings, and both heads on it
  stage_list / stage_nolist          `_stage_scores_kernels` with and without the graph kernel's `sched_list`
  exec                               `_exec_scores_kernels` over all jobs
  act_env                            the one-launch policy kernel `act_env(want_scores=True)`: its stage scores, and the executor scores of the job it
                                     chose against the reference's row of that job
On the GPU every route runs on the product library (matrix-core forms) and on the `vecforms` test build (tests/gpu_variant.py), each
against fp64. A route that a case or a build cannot reach is reported as skipped with its reason, never dropped.

Run as a script on a GPU box (`python tests/inference_fp64_util.py [cpu]`) it prints the tables of profiles/inference_fp64.md."""
import copy
import os.path as osp
import statistics
import sys

if __name__ == "__main__":
    sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

import pytest
import torch

from decima_util import AGENT, SCORE_ATOL
from update_fp64_util import FACTOR, KERNELS_OFF, SPIED, _excl_cumsum, _to

# chosen on the fp64 reference alone: with it no observation of the decision cases is a near-tie (check_near_ties); seed 5, the update
# test's, has exact fp64 ties between twin stages on `deep` and executor-score gaps of 9e-8 on `deep` and `e128`
POLICY_SEED = 8
# a bound above this fails the case as ill-conditioned (a noisy reference cannot hide a failure). It is what the older tests grant;
# 10 x the largest bound of the committed tables (3.35e-6, `saturated` executor scores: profiles/inference_fp64.md) would be above it
CEILING = SCORE_ATOL
QUANTITIES = ("node", "dag", "glob", "stage", "exec")
EMBEDDINGS = ("node", "dag", "glob")
ROUTES = ("one_call_mode1", "one_call_mode2", "launches", "stale_lists_mode1", "stale_lists_mode2", "capacity", "stage_list", "stage_nolist", "exec", "act_env")
ENCODER_KINDS = ("prep", "sink", "daghid", "dagsum", "globhid", "globsum")
NEAR_TIE_CAP = 0.05

_C2 = dict(num_executors=10, job_arrival_cap=20, job_arrival_rate=4.0e-5)
_DONE = dict(num_executors=10, job_arrival_cap=3, job_arrival_rate=4.0e-5, auto_reset=False)
# the smallest shapes at which this code can still go wrong (not the workload's sizes)
CASES = {
    "one_env_reset": dict(_C2, envs=1, steps=0, max_nodes=31),
    "one_env": dict(_C2, envs=1, steps=3, max_nodes=31),
    "small": dict(_C2, envs=48, steps=60, min_depth=6),
    "small16": dict(_C2, envs=16, steps=60, min_depth=6),
    "e1": dict(num_executors=1, job_arrival_cap=6, job_arrival_rate=1.0e-4, envs=8, steps=40, single_count=True),
    "e128": dict(num_executors=128, job_arrival_cap=30, job_arrival_rate=3.0e-4, envs=8, steps=60),
    "deep": dict(pack="deep", num_executors=50, job_arrival_cap=20, job_arrival_rate=1.2e-4, envs=8, steps=30, min_depth=10),
    "c3cap": dict(num_executors=50, job_arrival_cap=200, job_arrival_rate=4.0e-5, envs=4, steps=1500),
    "some_done": dict(_DONE, envs=12, steps=60, some_empty=True),
    "all_done": dict(_DONE, envs=12, steps=100, empty=True),
    "all_done6": dict(_DONE, envs=6, steps=400, empty=True),
    "saturated": dict(_C2, envs=16, steps=60, min_depth=6, head_scale=50.0),
}
DECISION_CASES = ("small", "deep", "e128")


def open_env(case: str, device, lib=None):
    """the env of a case after its fused rollout (the caller closes it)"""
    from spark_sched_sim_amd import VecSparkSchedSimEnv, workload

    c = CASES[case]
    cfg = dict(num_executors=c["num_executors"], job_arrival_cap=c["job_arrival_cap"], job_arrival_rate=c["job_arrival_rate"], moving_delay=2000.0, warmup_delay=1000.0)
    pack = workload.profile_pack(c["pack"]) if c.get("pack") else workload.default_pack()
    env = VecSparkSchedSimEnv(cfg, c["envs"], device=device, pack=pack, auto_reset=c.get("auto_reset", True), _lib=lib)
    env.reset(seed=13)
    if c["steps"]:
        env.rollout("fair", c["steps"])
    return env


def make_policy(case: str, seed: int = POLICY_SEED):
    """the case's policy on the CPU in fp32, unbound: biases N(0, 0.1) as everywhere in the suite; `head_scale`: both heads' first Linear
    (weight and bias) times that"""
    from spark_sched_sim_amd.decima import DecimaPolicy

    torch.manual_seed(seed)
    pol = DecimaPolicy(num_executors=CASES[case]["num_executors"], **AGENT).eval()
    with torch.no_grad():
        for name, p in pol.named_parameters():
            if "bias" in name:
                p.normal_(0.0, 0.1)
        s = CASES[case].get("head_scale")
        if s:
            for net in (pol.stage_policy_network, pol.exec_policy_network):
                net.mlp_score[0].weight.mul_(s)
                net.mlp_score[0].bias.mul_(s)
    return pol


def _padded(g, flat, idx):
    out = torch.full((g["n_obs"], g["n_pad"]), float("-inf"), dtype=flat.dtype, device=flat.device)
    out[g["node_obs"][idx], g["node_loc"][idx]] = flat
    return out


@torch.no_grad()
def forward_tensor_ops(pol, g, hidden=None):
    """{node, dag, glob, stage f[n_obs, n_pad], exec f[J, E]} by `encode`, `stage_scores` and `exec_scores` over all jobs. `hidden`: a dict
    that receives the |tanh| outputs of both heads' hidden layers"""
    hooks = []
    if hidden is not None:
        for name, net in (("stage", pol.stage_policy_network), ("exec", pol.exec_policy_network)):
            for m in net.mlp_score:
                if isinstance(m, torch.nn.Tanh):
                    hooks.append(m.register_forward_hook(lambda _m, _i, o, name=name: hidden.setdefault(name, []).append(o.detach().abs().reshape(-1))))
    try:
        h = pol.encode(g)
        s, idx = pol.stage_scores(g, h)
        es = pol.exec_scores(g, h, torch.arange(g["job_obs"].numel(), device=g["x"].device))
    finally:
        for k in hooks:
            k.remove()
    return {"node": h["node"], "dag": h["dag"], "glob": h["glob"], "stage": _padded(g, s, idx), "exec": es}


def reference_fp64(policy, g, hidden=None):
    """the forward pass in fp64 on the CPU: a deep copy of the (unbound) policy as `.double()`, x as double"""
    assert getattr(policy, "_kb", None) is None, "the reference is a copy of the policy from before bind_kernels"
    return forward_tensor_ops(copy.deepcopy(policy).cpu().double(), _to(g, "cpu", torch.float64), hidden)


def tensor_op_fp32(policy, g, device):
    """the second reference: the same three calls in fp32 tensor ops on `device`, no binding - and no training kernel either
    (train_kernels.MIN_ROWS out of reach, every entry point spied on)"""
    from spark_sched_sim_amd import train_kernels as tk

    assert getattr(policy, "_kb", None) is None
    calls = []
    with pytest.MonkeyPatch.context() as m:
        m.setattr(tk, "MIN_ROWS", KERNELS_OFF)
        for name in SPIED:
            m.setattr(tk, name, (lambda name: lambda *a, **k: calls.append(name))(name))
        out = forward_tensor_ops(copy.deepcopy(policy).to(device), _to(g, device))
    assert not calls, calls
    return out


def check_inputs(case: str, ref, g, hidden):
    """what a case must be for its comparison to mean anything, asserted on the REFERENCE and the graph before anything is compared"""
    c = CASES[case]
    M, J = g["x"].shape[0], g["job_obs"].numel()
    for k in QUANTITIES:
        assert not bool(torch.isnan(ref[k]).any()) and not bool(torch.isposinf(ref[k]).any()), k
    if c.get("empty"):
        assert M == 0 and J == 0 and int(g["obs_nodes"].sum()) == 0
        return
    assert M > 0 and J > 0 and bool(torch.isfinite(ref["stage"]).any())
    assert int(g["obs_depth"].max()) >= c.get("min_depth", 1), int(g["obs_depth"].max())
    if c.get("single_count"):
        assert int(g["job_cap"].max()) == 1
    else:
        assert int(g["job_cap"].max()) > 1
    if c.get("some_empty"):
        assert int(g["obs_nodes"].min()) == 0 < int(g["obs_nodes"].max()) and int(g["obs_jobs"].min()) == 0
    if "max_nodes" in c:
        assert M <= c["max_nodes"], M
    if c.get("head_scale"):
        for name in ("stage", "exec"):
            t = torch.cat(hidden[name])
            assert bool((t > 1 - 1e-6).any()) and bool((t < 0.5).any()), (name, float(t.max()), float(t.min()))


def _errors(ref, got, failures, route):
    """{quantity: error of `got` against the fp64 reference} for the quantities `got` holds: embeddings over max(1, the reference's
    largest entry), scores absolute over the finite entries - whose pattern must be EQUAL"""
    out = {}
    for k, v in got.items():
        r = ref[k]
        v = v.detach().double().cpu()
        assert v.shape == r.shape, (route, k, v.shape, r.shape)
        if k in EMBEDDINGS:
            assert bool(torch.isfinite(v).all()), (route, k)
            out[k] = float((v - r).abs().max()) / max(1.0, float(r.abs().max())) if r.numel() else 0.0
        else:
            fin = torch.isfinite(r)
            if not torch.equal(torch.isfinite(v), fin) or bool(torch.isnan(v).any()) or bool(torch.isposinf(v).any()):
                failures.append(f"{route}/{k}: the -inf pattern differs from the reference's")
                out[k] = float("inf")
            else:
                out[k] = float((v - r)[fin].abs().max()) if bool(fin.any()) else 0.0
    return out


def _half_ulp(v: torch.Tensor) -> torch.Tensor:
    """half the spacing of fp32 at |v| (0 at 0): what rounding an exact value of that size to fp32 can cost"""
    v = v.abs().double()
    return torch.where(v > 0, torch.exp2(torch.floor(torch.log2(v.clamp(min=1e-300))) - 24), torch.zeros_like(v))


# the (build, case) pairs whose bound gets a term derived from the arithmetic on top of the rule, and for which quantities: the one
# place where the rule's own inputs fall below what fp32 can hold. `some_done` has 7 nodes; under the emulator torch's errors there
# are 1.5e-8 (median) and 3.6e-9 (stage scores), so the rule grants 6.07e-8 - about one spacing of fp32 in [0.5, 1), where the scores
# lie - and the kernels' stage scores (6.32e-8) and observation summaries (7.48e-8) miss it. No other case, and no GPU row, needs one.
ARITHMETIC_TERMS = {("emu", "some_done"): ("glob", "stage")}


def arithmetic_terms(build: str, case: str, policy, g, ref):
    """{quantity: term} for the pairs of ARITHMETIC_TERMS (else None): the rounding of the quantity's LAST fp32 stage alone, every input
    of that stage taken as exact - computed from the fp64 reference's values, never from a kernel's result.
      stage  a score is stored as one fp32 number: half a spacing of fp32 at the largest finite reference score.
      glob   an observation summary is the fp32 sum of its jobs' rows y_j = global MLP(job summary j): every y_j is an fp32 number
             (half a spacing at |y_j| each) and each of the n - 1 additions rounds its partial sum (half a spacing at that partial
             sum); the largest total over observations and columns, over max(1, largest entry) like the error itself."""
    which = ARITHMETIC_TERMS.get((build, case))
    if which is None:
        return None
    out = {}
    if "stage" in which:
        fin = ref["stage"][torch.isfinite(ref["stage"])]
        out["stage"] = float(_half_ulp(fin.abs().max()))
    if "glob" in which:
        with torch.no_grad():
            y = copy.deepcopy(policy).cpu().double().encoder.global_encoder.mlp(ref["dag"])
        off, worst_sum = g["obs_job_off"].cpu().tolist(), 0.0
        for b, n in enumerate(g["obs_jobs"].cpu().tolist()):
            if n:
                rows = y[off[b]: off[b] + n]
                e = _half_ulp(rows).sum(0) + _half_ulp(torch.cumsum(rows, 0)[1:]).sum(0)
                worst_sum = max(worst_sum, float(e.max()))
        out["glob"] = worst_sum / max(1.0, float(ref["glob"].abs().max()))
    return out


def bounds_of(ref, top):
    """({quantity: bound}, {quantity: tensor-op error}, failures): bound = FACTOR x max(err(tensor-op fp32), median of the tensor-op
    errors over the case's quantities) - update_fp64_util.compare's rule and factor. Never from a kernel route's own error."""
    failures = []
    e_top = _errors(ref, top, failures, "tensor-op fp32")
    med = statistics.median(e_top[k] for k in QUANTITIES)
    bound = {k: FACTOR * max(e_top[k], med) for k in QUANTITIES}
    for k in QUANTITIES:
        if not bound[k] <= CEILING:
            failures.append(f"{k}: ill-conditioned, bound {bound[k]:.3g} > ceiling {CEILING:.3g}")
    return bound, e_top, failures


def compare(ref, top, routes, extra_bound=None):
    """(failures, rows): for every route and quantity, err(route) <= bound (`bounds_of`; `extra_bound`: {quantity: term}, `arithmetic_terms`, added to it;
    the ceiling holds for the sum). rows: (route, quantity, tensor-op error, route's error or the reason it was skipped, bound)"""
    bound, e_top, failures = bounds_of(ref, top)
    if extra_bound:
        bound = {k: bound[k] + extra_bound.get(k, 0.0) for k in bound}
        failures += [f"{k}: bound with its arithmetic term {bound[k]:.3g} > ceiling {CEILING:.3g}" for k in extra_bound if not bound[k] <= CEILING]
    rows = []
    for route, got in routes.items():
        if isinstance(got, str):
            rows.append((route, "-", None, got, None))
            continue
        for k, e in _errors(ref, got, failures, route).items():
            if not e <= bound[k]:
                failures.append(f"{route}/{k}: error {e:.3g} > bound {bound[k]:.3g} (tensor-op error {e_top[k]:.3g})")
            rows.append((route, k, e_top[k], e, bound[k]))
    return failures, rows


def table(rows) -> str:
    fmt = lambda v: "-" if v is None else v if isinstance(v, str) else f"{v:.2e}"  # noqa: E731
    lines = ["| route | quantity | tensor-op fp32 | kernel route | bound |", "|---|---|---|---|---|"]
    lines += [f"| `{r}` | {k} | {fmt(a)} | {fmt(b)} | {fmt(c)} |" for r, k, a, b, c in rows]
    return "\n".join(lines)


# ---- the routes ----------------------------------------------------------------------------------------------------------------

class Spy:
    """counts the calls of a bound policy's Python entry points (`_encode_one_call`, `_launch` by kind, `act_env`)"""

    def __init__(self, policy):
        self.policy, self.counts = policy, {}

    def __enter__(self):
        p, c = self.policy, self.counts
        one, launch, act_env = p._encode_one_call, p._launch, p.act_env

        def spy_one(*a, **k):
            c["one_call"] = c.get("one_call", 0) + 1
            return one(*a, **k)

        def spy_launch(kind, *a, **k):
            c[kind] = c.get(kind, 0) + 1
            return launch(kind, *a, **k)

        def spy_act_env(*a, **k):
            c["act_env"] = c.get("act_env", 0) + 1
            return act_env(*a, **k)
        p._encode_one_call, p._launch, p.act_env = spy_one, spy_launch, spy_act_env
        return self

    def __exit__(self, *exc):
        del self.policy._encode_one_call, self.policy._launch, self.policy.act_env

    def take(self):
        out = dict(self.counts)
        self.counts.clear()
        return out


def _scratch_totals(policy, dev):
    """the list lengths sss_gnn_encode's own scan + list kernel writes (work space of `_encode_one_call`, one per stream)"""
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    sc = policy.__dict__.get("_enc_scratch", {}).get((dev, stream))
    return None if sc is None else sc["tot"]


def bind(policy, env):
    return copy.deepcopy(policy).to(env.device).eval().bind_kernels(env._b)


@torch.no_grad()
def run_routes(case: str, env, policy, g=None, graph_edit=None, head_edit=None):
    """{route: {quantity: tensor} or "skipped: <reason>"} on `env`'s current observations with the BOUND `policy`; every route asserts,
    from the calls it spied on, that it was the route it claims to be. `g`: the exact-size graph (default: a new one).
    Negative controls: `graph_edit(g)` -> the graph every encoder route gets, `head_edit(g)` -> the graph the heads get."""
    c = CASES[case]
    dev = env.device
    g = env.decima_graph() if g is None else g
    M, J, B = g["x"].shape[0], g["job_obs"].numel(), g["n_obs"]
    empty = M == 0
    n_recv = [int(((g["node_recv"] >> l) & 1).sum()) for l in range(32)] if M else [0] * 32
    depth = max((l + 1 for l in range(32) if n_recv[l]), default=0)
    ge = graph_edit or (lambda x: x)
    he = head_edit or (lambda x: x)
    out = {}
    enc = lambda h, m=None, j=None: {"node": h["node"][:m].clone(), "dag": h["dag"][:j].clone(), "glob": h["glob"].clone()}  # noqa: E731
    with Spy(policy) as spy:
        # the encoder through sss_gnn_encode, the graph kernel's own lists
        for mode in (1, 2):
            policy._layers_mode = mode
            assert g["_layer_lists"][0]["epoch"] == g["_layer_lists"][1]
            out[f"one_call_mode{mode}"] = enc(policy._encode_kernels(ge(dict(g))))
            assert spy.take() == ({} if empty else {"one_call": 1}), (case, mode)
        # launch by launch
        policy._layers_mode = 0
        out["launches"] = enc(policy._encode_kernels(ge({k: v for k, v in g.items() if k != "max_depth"})))
        want = {} if empty else dict({k: 1 for k in ENCODER_KINDS}, **({"layer": depth} if depth else {}))
        assert spy.take() == want, (case, want)
        # the graph without its lists: sss_gnn_encode scans and lists by itself (mode 1); mode 2 needs no lists
        has_one_launch = None
        for mode in (1, 2):
            policy._layers_mode = mode
            tot = _scratch_totals(policy, dev)
            if tot is not None:
                tot.zero_()
            h = enc(policy._encode_kernels(ge({k: v for k, v in g.items() if k != "_layer_lists"})))
            assert spy.take() == ({} if empty else {"one_call": 1}), (case, mode)
            listed = [] if empty else _scratch_totals(policy, dev).tolist()
            if empty:
                out[f"stale_lists_mode{mode}"] = h
            elif mode == 1:
                assert listed == n_recv, (case, listed, n_recv)  # (the scan + list kernel ran, on this graph)
                out["stale_lists_mode1"] = h
            elif depth == 0:
                out["stale_lists_mode2"] = "skipped: no DAG layer in this graph, so no layer launch of either kind"
            else:
                has_one_launch = not any(listed)
                assert has_one_launch or listed == n_recv
                out["stale_lists_mode2"] = h if has_one_launch else "skipped: this build has no one-launch layers kernel (it took the launches per layer)"
        if has_one_launch is False or (not empty and depth == 0):
            out["one_call_mode2"] = out["stale_lists_mode2"]
        policy._layers_mode = 0
        # both heads on the exact-size graph, embeddings of the first route
        hk = {k: v for k, v in out["one_call_mode1"].items()}
        gh = he(dict(g))
        out["stage_list"] = {"stage": policy._stage_scores_kernels(gh, hk)}
        assert "sched_list" in gh and spy.take() == ({} if empty else {"stage": 1})
        out["stage_nolist"] = {"stage": policy._stage_scores_kernels({k: v for k, v in gh.items() if k != "sched_list"}, hk)}
        assert spy.take() == ({} if empty else {"stage": 1})
        jobs = torch.arange(J, device=dev)
        out["exec"] = {"exec": policy._exec_scores_kernels(gh, hk, jobs)}
        assert spy.take() == ({} if empty else {"exec": 1})
        # the capacity graph: only the leading totals_dev rows mean anything
        if graph_edit is not None or head_edit is not None:
            out["capacity"] = "skipped: the controls edit the exact-size graph"
        elif not env.graph_kernel_fits:
            out["capacity"] = "skipped: the graph kernel does not take this node capacity"
        else:
            gc = env.decima_graph_on_device()
            tot = gc["totals_dev"].tolist()
            assert (tot[0], tot[2]) == (M, J) and "totals_dev" not in g
            hc = policy._encode_kernels(gc)
            assert spy.take() == {"one_call": 1}
            res = enc(hc, M, J)
            res["stage"] = policy._stage_scores_kernels(gc, hc).clone()
            res["exec"] = policy._exec_scores_kernels(gc, hc, jobs) if J else torch.empty((0, policy.num_executors), device=dev)
            assert spy.take() == dict({"stage": 1}, **({"exec": 1} if J else {}))
            out["capacity"] = res
        # the one-launch policy kernel
        if graph_edit is not None or head_edit is not None:
            out["act_env"] = "skipped: the controls edit the graph, which this kernel does not read"
        else:
            try:
                acts, a = policy.act_env(env, counter=7, seed=3, want_scores=True)
            except ValueError as e:  # (refused by the library before anything is launched: 20 bytes of LDS per node slot)
                assert "node capacity too large for the Decima policy kernel" in str(e), e
                out["act_env"] = "skipped: the one-launch policy kernel does not take this node capacity"
            else:
                out["act_env"] = {"stage": a["stage_scores"]}
                out["act_env/exec"] = (acts, a)
            assert spy.take() == {"act_env": 1}
    assert set(ROUTES) <= set(out), sorted(set(ROUTES) - set(out))
    return out


def chosen_exec_rows(g, ref, routes, failures):
    """act_env's executor scores are those of the job it chose: moves them into an [J, E] matrix that holds the REFERENCE's rows
    everywhere else, so that `compare` looks at exactly the chosen jobs' rows (an env without a schedulable stage: all -inf, no job)"""
    pair = routes.pop("act_env/exec", None)
    if pair is None:
        return
    acts, a = pair
    any_stage = a["any_stage"].cpu()
    want_any = torch.isfinite(ref["stage"]).any(1)
    if not torch.equal(any_stage, want_any):
        failures.append("act_env: any_stage differs from the reference's")
        return
    es = a["exec_scores"].double().cpu()
    full = ref["exec"].clone()
    gid = (g["obs_job_off"].cpu() + a["job_idx"].cpu())[any_stage]
    assert bool((a["job_idx"].cpu()[any_stage] < g["obs_jobs"].cpu()[any_stage]).all())
    full[gid] = es[any_stage]
    if bool(torch.isfinite(es[~any_stage]).any()):
        failures.append("act_env: executor scores for an env without a schedulable stage")
    routes["act_env"]["exec"] = full


def run_case(case: str, env, policy, ref, top, g=None, extra_bound=None):
    """(failures, rows) of all routes of a case"""
    g = env.decima_graph() if g is None else g
    routes = run_routes(case, env, policy, g)
    failures = []
    chosen_exec_rows(g, ref, routes, failures)
    f, rows = compare(ref, top, routes, extra_bound)
    return failures + f, rows


def expected_skips(case: str, g, one_launch_kernel: bool) -> set:
    """the routes a case cannot reach on a build with / without the one-launch layers kernel (matrix cores only)"""
    if g["x"].shape[0] == 0:
        return set()  # (nothing is launched on any route)
    out = {"act_env"} if case == "c3cap" else set()
    if not one_launch_kernel or int(g["obs_depth"].max()) == 0:
        out |= {"one_call_mode2", "stale_lists_mode2"}
    return out


def prepare(case: str, device, lib=None):
    """(env, unbound policy on the CPU, exact-size graph, fp64 reference, fp32 tensor-op reference) with the case's input conditions
    checked on the reference"""
    env = open_env(case, device, lib)
    pol = make_policy(case)
    g = env.decima_graph()
    hidden = {}
    ref = reference_fp64(pol, g, hidden)
    check_inputs(case, ref, g, hidden)
    top = tensor_op_fp32(pol, g, env.device)
    return env, pol, g, ref, top


def same_graph(g, other) -> bool:
    return all(torch.equal(g[k], other[k]) for k in ("x", "src", "dst", "job_cap", "stage_mask", "obs_nodes", "node_recv"))


def check_no_node_routes(env, pol, ref):
    """every env finished, no auto-reset: `act` on the exact-size graph (kernels bound, and tensor ops alone), `schedule_env` on the
    exact-size and on the capacity graph and `act_env` agree - no stage anywhere, the action `env.step` takes for "nothing to schedule"""
    B = env.num_envs
    bound = bind(pol, env)
    assert not bool(torch.isfinite(ref["stage"]).any()) and ref["node"].shape == (0, 16) and ref["glob"].shape == (B, 16)
    h = bound._encode_kernels(env.decima_graph())
    assert h["node"].shape == (0, 16) and h["dag"].shape == (0, 16) and h["glob"].shape == (B, 16) and not bool(h["glob"].any())
    want, _ = bound.schedule_env(env, host_sync=False, fresh_outputs=True)  # the capacity route: what run_episodes' tail has always taken
    assert bool((want["stage_idx"] == -1).all())
    plain = copy.deepcopy(pol).to(env.device)  # (never bound: tensor ops alone)
    acts = {"act, kernels bound": bound.act(env.decima_graph()), "act, tensor ops": plain.act(_to(env.decima_graph(), env.device))}
    results = {**{k: bound.env_actions(a) for k, a in acts.items()},
               "schedule_env, exact sizes": bound.schedule_env(env, host_sync=True, fresh_outputs=True)[0],
               "schedule_env, greedy": bound.schedule_env(env, greedy=True, fresh_outputs=True)[0],
               "act_env": bound.act_env(env, counter=1)[0]}
    for name, act in results.items():
        assert torch.equal(act["stage_idx"].long(), want["stage_idx"].long()), name
    for name, a in acts.items():
        assert a["any_stage"].shape == (B,) and not bool(a["any_stage"].any()), name


# ---- decisions -----------------------------------------------------------------------------------------------------------------

def reference_choices(g, ref, bound):
    """per observation: (rank of the fp64 arg-max among the schedulable stages, whether its lead over the runner-up exceeds 2 x the stage
    bound, the executor count - 1 with the largest fp64 score for that stage's job, whether ITS lead exceeds 2 x the exec bound, whether
    the observation has a choice of stage / the job a choice of count)"""
    s = ref["stage"]
    fin = torch.isfinite(s)
    n_fin = fin.sum(1)
    top2 = torch.topk(s, min(2, s.shape[1]), 1).values
    loc = s.argmax(1)
    rank = (fin & (torch.arange(s.shape[1])[None, :] < loc[:, None])).sum(1)
    clear_s = (n_fin >= 1) & ((n_fin == 1) | ((top2[:, 0] - top2[:, -1]) > 2 * bound["stage"]))
    node = (g["obs_node_off"].cpu() + loc).clamp(max=max(g["x"].shape[0] - 1, 0))
    job = g["node_job"].cpu()[node]
    es = ref["exec"][job]
    n_e = torch.isfinite(es).sum(1)
    e2 = torch.topk(es, min(2, es.shape[1]), 1).values
    clear_e = (n_e >= 1) & ((n_e == 1) | ((e2[:, 0] - e2[:, -1]) > 2 * bound["exec"]))
    return {"rank": rank, "clear_stage": clear_s, "count": es.argmax(1), "clear_exec": clear_s & clear_e,
            "stage_choice": n_fin >= 2, "exec_choice": (n_fin >= 1) & (n_e >= 2), "any": n_fin >= 1}


def check_near_ties(ch):
    """the condition on the INPUTS: at most 5 % of the observations with a choice are left out as near-ties (reference alone)"""
    for what, clear in (("stage", "clear_stage"), ("exec", "clear_exec")):
        have = ch[what + "_choice"]
        left_out = int((have & ~ch[clear]).sum())
        assert int(have.sum()) > 0 and left_out <= NEAR_TIE_CAP * int(have.sum()), (what, left_out, int(have.sum()))


def check_decisions(env, policy, g, ref, bound):
    """`schedule_env(greedy=True)` - the pipeline and `one_launch=True` - chooses the fp64 arg-max wherever that one is clear"""
    ch = reference_choices(g, ref, bound)
    check_near_ties(ch)
    calls = getattr(policy, "_calls", 0)
    n = {}
    for one_launch in (False, True):
        act, _ = policy.schedule_env(env, greedy=True, one_launch=one_launch, fresh_outputs=True)
        stage, count = act["stage_idx"].cpu().long(), act["num_exec"].cpu().long() - 1
        assert bool((stage[~ch["any"]] == -1).all())
        cs, ce = ch["clear_stage"], ch["clear_exec"]
        assert torch.equal(stage[cs], ch["rank"][cs]), (one_launch, (stage[cs] != ch["rank"][cs]).nonzero().tolist())
        assert torch.equal(count[ce], ch["count"][ce]), (one_launch, (count[ce] != ch["count"][ce]).nonzero().tolist())
        n[one_launch] = (int(cs.sum()), int(ce.sum()))
    assert getattr(policy, "_calls", 0) == calls
    return n


# ---- negative controls: a slightly wrong VALUE handed on by a Python entry point (no fault, no out-of-range access) ----------------

def _control_update_bias(policy, g, fired):
    """one entry of the packed `update` image's last bias (the image's last entry) moved by 1e-5"""
    w = policy._packed_weights()["update"]
    w[-1] += 1e-5
    fired.append(float(w[-1]))
    return {}


def _control_out_deg(policy, g, fired):
    def edit(gg):
        i = int((gg["out_deg"] >= 2).nonzero()[0])
        gg["out_deg"] = gg["out_deg"].clone()
        gg["out_deg"][i] -= 1  # (its last child's message is left out)
        fired.append(i)
        return gg
    return {"graph_edit": edit}


def _control_job_nodes(policy, g, fired):
    def edit(gg):
        j = int((gg["job_nodes"] >= 2).nonzero()[0])
        gg["job_nodes"] = gg["job_nodes"].clone()
        gg["job_nodes"][j] -= 1
        fired.append(j)
        return gg
    return {"graph_edit": edit}


def _control_swap_columns(policy, g, fired):
    def edit(gg):
        x = gg["x"].clone()
        x[:, 0], x[:, 2] = gg["x"][:, 2], gg["x"][:, 0]  # (both heads read columns 0..2)
        assert not torch.equal(x, gg["x"])
        gg["x"] = x
        fired.append(1)
        return gg
    return {"head_edit": edit}


def _control_count_feature(policy, g, fired):
    """the executor head sees (e + 1) / E for e / E: its first Linear's bias gains that feature's weight column / E"""
    lin = policy.exec_policy_network.mlp_score[0]
    with torch.no_grad():
        lin.bias.add_(lin.weight[:, -1] / policy.num_executors)
    policy.invalidate_kernel_weights()
    fired.append(1)
    return {}


CONTROLS = {"update_image_last_bias_plus_1e-5": _control_update_bias, "out_deg_one_short": _control_out_deg, "job_nodes_one_short": _control_job_nodes,
            "head_feature_columns_swapped": _control_swap_columns, "exec_count_feature_shifted": _control_count_feature}


def run_control(name, case, env, policy, g, ref, top):
    """(failures, rows) of the routes with control `name` switched on, on a fresh binding of `policy` (the control must have fired)"""
    pol = bind(policy, env)
    fired = []
    kw = CONTROLS[name](pol, g, fired)
    routes = run_routes(case, env, pol, g, **kw)
    assert fired, name
    routes.pop("act_env/exec", None)
    return compare(ref, top, routes)


def worst(rows):
    """(route, quantity, error, error / bound) of the row that is furthest out"""
    r = max((r for r in rows if r[4] is not None), key=lambda r: r[3] / r[4] if r[4] > 0 else (float("inf") if r[3] > 0 else 0.0))
    return r[0], r[1], r[3], (r[3] / r[4] if r[4] > 0 else float("inf"))


def _report(device):  # pragma: no cover - the tables of profiles/inference_fp64.md
    if device != "cpu":
        from gpu_variant import load_variant
        libs = {"matrix-core forms (product library)": ("mfma", None), "vector-unit forms (`vecforms` test build)": ("vecforms", load_variant("vecforms"))}
    else:
        from emu_util import load_emu
        libs = {"wave emulator (vector-unit forms)": ("emu", load_emu())}
    print(f"factor {FACTOR:g}, ceiling {CEILING:g}\n")
    largest = 0.0
    for case in CASES:
        for build, (tag, lib) in libs.items():
            env, pol, g, ref, top = prepare(case, device, lib)
            extra = arithmetic_terms(tag, case, pol, g, ref)
            failures, rows = run_case(case, env, bind(pol, env), ref, top, g, extra)
            largest = max([largest] + [r[4] for r in rows if r[4] is not None])
            plain = bounds_of(ref, top)[0]
            leaning = [f"`{r[0]}` {r[1]} ({r[3]:.2e} against the rule's {plain[r[1]]:.2e})" for r in rows if r[4] is not None and r[3] > plain[r[1]]]
            print(f"## {case}, {build}\n\n{g['n_obs']} observations, {g['x'].shape[0]} nodes, {g['job_obs'].numel()} jobs, {int(g['stage_mask'].sum())} schedulable stages, "
                  f"depth {int(g['obs_depth'].max()) if g['x'].shape[0] else 0}, largest |node embedding| {float(ref['node'].abs().max()) if g['x'].shape[0] else 0.0:.3g}\n\n{table(rows)}\n\nfailures: {failures or 'none'}"
                  + (f"; arithmetic terms added to the bound: {({k: float(f'{v:.3g}') for k, v in extra.items()})}; rows beyond the plain rule: {', '.join(leaning) or 'none'}" if extra else "") + "\n")
            if case in DECISION_CASES:
                n = check_decisions(env, bind(pol, env), g, ref, bounds_of(ref, top)[0])
                print(f"decisions: the greedy pipeline and the one-launch kernel choose the fp64 arg-max on {n[False][0]} / {n[True][0]} of {g['n_obs']} observations "
                      f"(stage) and {n[False][1]} / {n[True][1]} (executor count); the rest are near-ties\n")
            if case in ("small16", "one_env"):
                for name in CONTROLS:
                    f, crows = run_control(name, case, env, pol, g, ref, top)
                    w = worst(crows)
                    under = all(r[3] <= SCORE_ATOL for r in crows if r[4] is not None)
                    print(f"control `{name}`: {'caught' if f else 'NOT caught'}, {len(f)} (route, quantity) pairs out of bounds; the furthest out: `{w[0]}` {w[1]}, "
                          f"error {w[2]:.2e} = {w[3]:.1f} x its bound; every error under SCORE_ATOL = {SCORE_ATOL:g}: {under}\n")
            env.close()
    print(f"largest bound: {largest:.3g}")


if __name__ == "__main__":
    _report(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
