"""shared by tests/test_update_reference.py (CPU, emulator library) and tests/test_gpu_update_fp64.py: the assembled PPO update,
`training.ppo_loss(...)` + `.backward()`, on the hand-written kernels (spark_sched_sim_amd.train_kernels) against the same update in
fp64 on the CPU - a deep copy of the policy, `.double()`, whose tensor-op forms use none of those kernels.

Run as a script on a GPU box (`python tests/update_fp64_util.py`) it prints the per-tensor tables of profiles/update_fp64.md."""
import copy
import os.path as osp
import statistics
import sys

if __name__ == "__main__":
    sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))

import pytest
import torch

from decima_util import AGENT, SCORE_ATOL

CLIP_RANGE, ENTROPY_COEFF = 0.2, 0.04
PERM_SEED = 2
TWO_OBS = (5, 6)  # positions in the seed-2 permutation: the chosen job of the second one allows more than one executor count
# the kernels add the same fp32 terms as torch in another order (per-wave partials, MFMA accumulation chains, ordered adds): round-off
# of the same size as torch's own, not equal to it. 4 x (torch's own error against fp64) is the bound; see `compare`.
FACTOR = 4.0
GRAD_CEILING, EXEC_HEAD_CEILING = 2e-4, 1e-3  # a bound above these: the case is ill-conditioned (a noisy reference cannot hide a failure)
SCALAR_CEILING = SCORE_ATOL
# exactly zero by the softmax's shift invariance (the reference shows ~1e-17 there): the only two entries no comparison looks at
SHIFT_INVARIANT = ("stage_policy_network.mlp_score.4.bias", "exec_policy_network.mlp_score.4.bias")
KERNELS_OFF = 1 << 62
SPIED = ("rows_op", "rows_concat", "mlp_forward", "mlp_backward_wgrad", "_segcat_call")
SCALARS = ("node", "dag", "glob", "scores", "lgprobs", "entropies", "loss")

# the smallest shapes at which the wiring can still go wrong (not the workload's sizes); `mix` is what a real update launches:
# some operators above train_kernels.MIN_ROWS, some below
CASES = {
    "small": dict(pack=None, num_executors=10, job_arrival_rate=4.0e-5, envs=48, steps=60, min_depth=6),
    "wide_head": dict(pack=None, num_executors=100, job_arrival_rate=1.2e-4, envs=48, steps=80, min_depth=6),
    "deep": dict(pack="deep", num_executors=50, job_arrival_rate=1.2e-4, envs=24, steps=30, min_depth=10),
    "mix": dict(pack=None, num_executors=10, job_arrival_rate=4.0e-5, envs=512, steps=150, min_depth=6),
}


def record(case: str, device, lib=None):
    """the env of a case after its fused rollout (the caller closes it)"""
    from spark_sched_sim_amd import VecSparkSchedSimEnv, workload

    c = CASES[case]
    cfg = dict(num_executors=c["num_executors"], job_arrival_cap=20, job_arrival_rate=c["job_arrival_rate"], moving_delay=2000.0, warmup_delay=1000.0)
    pack = workload.profile_pack(c["pack"]) if c["pack"] else workload.default_pack()
    env = VecSparkSchedSimEnv(cfg, c["envs"], device=device, pack=pack, auto_reset=True, _lib=lib)
    env.reset(seed=13)
    env.rollout("fair", c["steps"])
    return env


def _excl_cumsum(v):
    return torch.cumsum(v, 0) - v


def _to(sub, device, dtype=None):
    """the minibatch on `device` (x as `dtype`), without what `graph_layers` / `select_observations` cached in it"""
    out = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in sub.items() if k != "layers" and not k.startswith("_")}
    if dtype is not None:
        out["x"] = out["x"].to(dtype)
    return out


def make_minibatch(env, policy_seed: int, keep=None):
    """(policy on the CPU in fp32, minibatch graph on the env's device, (stage_sel, job_idx, exec_sel), advantages f64, old_lgprobs f32)
    from the env's current observations: cut with `select_observations` in PERMUTED order (as PPO.train_on_rollouts does), `keep` =
    positions in that permutation (None: all). The recorded actions are integer arithmetic on the graph, not samples - `Generator`
    streams differ between devices, and the CPU leg and the GPU leg must see the same minibatch. Observations without a schedulable
    stage are left out."""
    from spark_sched_sim_amd.decima import DecimaPolicy, select_observations

    g = env.decima_graph(None)
    dev, n_obs, E = g["x"].device, g["n_obs"], env.num_executors
    perm = torch.randperm(n_obs, generator=torch.Generator().manual_seed(PERM_SEED))
    ids = (perm if keep is None else perm[list(keep)]).to(dev)
    n_sched = torch.zeros(n_obs, dtype=torch.long, device=dev).index_add_(0, g["node_obs"].long(), g["stage_mask"].long())
    ids = ids[n_sched[ids] > 0]
    sub = select_observations(g, ids)
    stage_sel = (7 * ids + 3) % n_sched[ids]
    job_idx = (5 * ids + 1) % g["obs_jobs"][ids].long()
    cap = sub["job_cap"][_excl_cumsum(sub["obs_jobs"].long()) + job_idx].long()
    exec_sel = (3 * ids + 2) % cap.clamp(min=1, max=E)
    acts = (stage_sel, job_idx, exec_sel)
    torch.manual_seed(policy_seed)
    pol = DecimaPolicy(num_executors=E, **AGENT)
    with torch.no_grad():  # (biases start at zero: give them values so that their gradients are exercised)
        for name, p in pol.named_parameters():
            if "bias" in name:
                p.normal_(0.0, 0.1)
    gen = torch.Generator().manual_seed(policy_seed + 1)
    k = int(ids.numel())
    adv = torch.randn(k, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        lg = copy.deepcopy(pol).double().evaluate_actions(_to(sub, "cpu", torch.float64), *[a.cpu() for a in acts])["lgprobs"]
    old = (lg + 0.05 * torch.randn(k, generator=gen, dtype=torch.float64)).float()
    return pol, sub, acts, adv, old


def _update(pol, sub, acts, adv, old):
    """one ppo_loss + backward; what the pass itself computed on the way (the three embeddings of `encode`, the flat stage scores,
    lgprobs, entropies) is recorded from inside it, the loss and every parameter's gradient after it"""
    from spark_sched_sim_amd.training import ppo_loss

    seen = {}
    encode, stage_scores, evaluate_actions = pol.encode, pol.stage_scores, pol.evaluate_actions

    def spy_encode(g, per_obs_skip=True):
        h = encode(g, per_obs_skip)
        seen.update({k: v.detach().clone() for k, v in h.items()})
        return h

    def spy_scores(g, h):
        s, idx = stage_scores(g, h)
        seen["scores"] = s.detach().clone()
        return s, idx

    def spy_evaluate(*args):
        res = evaluate_actions(*args)
        seen.update({k: res[k].detach().clone() for k in ("lgprobs", "entropies")})
        return res

    pol.encode, pol.stage_scores, pol.evaluate_actions = spy_encode, spy_scores, spy_evaluate
    try:
        pol.zero_grad()
        loss, _ = ppo_loss(pol, sub, *acts, adv, old, CLIP_RANGE, ENTROPY_COEFF)
        loss.backward()
    finally:
        del pol.encode, pol.stage_scores, pol.evaluate_actions
    seen["loss"] = loss.detach().clone()
    seen["grads"] = {k: p.grad.detach().clone() for k, p in pol.named_parameters()}
    return seen


def reference_fp64(policy, sub, acts, adv, old):
    """the update in fp64 on the CPU: a deep copy of the policy as `.double()`, x as double - every operator takes its tensor-op form"""
    pol = copy.deepcopy(policy).cpu().double()
    return _update(pol, _to(sub, "cpu", torch.float64), [a.cpu() for a in acts], adv.cpu(), old.cpu())


def run_fp32(policy, sub, acts, adv, old, min_rows: int, deterministic: bool = False, device="cuda:0", sabotage=None):
    """(the same quantities in fp32 on `device`, {entry point: number of calls}) with train_kernels.MIN_ROWS = `min_rows` - every gate
    reads the module attribute when called, so one patch switches them all: 1 = every operator on the kernels, 8192 = the product's
    own mix, KERNELS_OFF = torch's fp32 operators (the second reference: it sizes the tolerances). `sabotage`: {entry point:
    f(real function) -> wrapped function}, the negative controls."""
    from spark_sched_sim_amd import train_kernels as tk

    pol = copy.deepcopy(policy).to(device)
    counts = dict.fromkeys(SPIED, 0)

    def spy(name, fn):
        def call(*args, **kw):
            counts[name] += 1
            return fn(*args, **kw)
        return call

    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    with pytest.MonkeyPatch.context() as m:
        m.setattr(tk, "MIN_ROWS", min_rows)
        for name in SPIED:
            fn = getattr(tk, name)
            if sabotage and name in sabotage:
                fn = sabotage[name](fn)
            m.setattr(tk, name, spy(name, fn))
        torch.use_deterministic_algorithms(deterministic)
        try:
            out = _update(pol, _to(sub, device), [a.to(device) for a in acts], adv.to(device), old.to(device))
        finally:
            torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
    return out, counts


def check_inputs(ref, sub, acts, min_depth: int = 6, above_threshold: bool = False):
    """what a case must be for its comparison to mean anything, asserted on the REFERENCE before anything is compared"""
    for k, g in ref["grads"].items():
        assert bool(torch.isfinite(g).all()), k
        if k not in SHIFT_INVARIANT:
            assert float(g.abs().max()) > 1e-8, (k, float(g.abs().max()))  # (e.g. no chosen job with a choice: the executor head gets no gradient)
    for k in SHIFT_INVARIANT:
        assert float(ref["grads"][k].abs().max()) < 1e-12, k
    assert sub["n_obs"] >= 2
    cap = sub["job_cap"][_excl_cumsum(sub["obs_jobs"].long()) + acts[1]]
    assert int(cap.min()) >= 1 and int(cap.max()) > 1, (int(cap.min()), int(cap.max()))
    assert int(sub["obs_depth"].max()) >= min_depth, int(sub["obs_depth"].max())
    if above_threshold:
        assert sub["x"].shape[0] >= 8192 and int(sub["stage_mask"].sum()) >= 8192, (sub["x"].shape[0], int(sub["stage_mask"].sum()))


def _errors(ref, got):
    """{quantity: error of `got` against the fp64 reference}: a gradient tensor's largest deviation over the reference's largest
    entry; absolute for the others (an embedding's over max(1, its largest entry))"""
    d = lambda a, b: float((a.detach().double().cpu() - b).abs().max())  # noqa: E731
    out = {}
    for k in SCALARS:
        scale = max(1.0, float(ref[k].abs().max())) if k in ("node", "dag", "glob") else 1.0
        assert got[k].shape == ref[k].shape, k
        out[k] = d(got[k], ref[k]) / scale
    for k, g in ref["grads"].items():
        if k not in SHIFT_INVARIANT:
            assert got["grads"][k].shape == g.shape, k
            out["grad " + k] = d(got["grads"][k], g) / float(g.abs().max())
    return out


def compare(ref, tensor_op, kernel=None, factor: float = FACTOR):
    """(failures, rows): for every quantity t, err(kernel, t) <= factor * max(err(tensor-op fp32, t), median of err(tensor-op fp32, .)
    over the quantities of t's kind) - tolerances come from the reference's own error, never from the kernels'. The median floor
    keeps a tensor on which torch happens to be nearly exact from setting an unattainable bound; a bound above its ceiling fails the
    case as ill-conditioned. rows: (quantity, tensor-op error, kernel error, bound). Every entry of every quantity is compared but
    the two SHIFT_INVARIANT scalars. `kernel=None`: the conditions on the reference alone."""
    e_top = _errors(ref, tensor_op)
    e_ker = _errors(ref, kernel) if kernel is not None else {}
    med_scalar = statistics.median(e_top[k] for k in SCALARS)
    med_grad = statistics.median(v for k, v in e_top.items() if k.startswith("grad "))
    failures, rows = [], []
    for k, e in e_top.items():
        grad = k.startswith("grad ")
        bound = factor * max(e, med_grad if grad else med_scalar)
        ceiling = SCALAR_CEILING if not grad else EXEC_HEAD_CEILING if k.startswith("grad exec_policy_network.") else GRAD_CEILING
        if not bound <= ceiling:
            failures.append(f"{k}: ill-conditioned, bound {bound:.3g} > ceiling {ceiling:.3g}")
        if kernel is not None and not e_ker[k] <= bound:
            failures.append(f"{k}: kernel error {e_ker[k]:.3g} > bound {bound:.3g} (tensor-op error {e:.3g})")
        rows.append((k, e, e_ker.get(k), bound))
    return failures, rows


def table(rows) -> str:
    fmt = lambda v: "-" if v is None else f"{v:.2e}"  # noqa: E731
    lines = ["| quantity | tensor-op fp32 | kernel path | bound |", "|---|---|---|---|"]
    lines += [f"| `{k}` | {fmt(a)} | {fmt(b)} | {fmt(c)} |" for k, a, b, c in rows]
    return "\n".join(lines)


def same_bits(a, b) -> bool:
    return all(torch.equal(a[k], b[k]) for k in SCALARS) and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])


# ---- negative controls: a subtly wrong VALUE out of a Python entry point (no fault, no out-of-range access) ----------------------

def _drop_last_scatter_row(fired):
    def wrap(rows_op):
        def call(op, idx, a, b, *args, **kw):
            if op == 1 and a.shape[0] >= 2:  # ROWS_SCATTER_ADD without the list's last row
                fired.append(int(a.shape[0]))
                return rows_op(op, idx[:-1], a[:-1], b, *args, **kw)
            return rows_op(op, idx, a, b, *args, **kw)
        return call
    return {"rows_op": wrap}


def _shorten_last_segment(fired):
    def wrap(rows_op):
        def call(op, idx, a, b, *args, **kw):
            if op == 5 and idx.numel() >= 2 and int(idx[-1]) > int(idx[-2]):  # ROWS_SEGMENT_SUM: the last segment loses its last row
                fired.append(int(idx[-1]))
                idx = idx.clone()
                idx[-1] -= 1
            return rows_op(op, idx, a, b, *args, **kw)
        return call
    return {"rows_op": wrap}


def _swap_concat_columns(fired):
    def wrap(rows_concat):
        def call(op, out, tables, idxs, **kw):
            if op == 1:  # backward: two equal-width parts get each other's columns of the gradient rows
                widths = [t if isinstance(t, int) else t.shape[1] for t in tables]
                offs = [sum(widths[:k]) for k in range(len(widths))]
                pairs = [(a, b) for a in range(len(widths)) for b in range(a + 1, len(widths))
                         if widths[a] == widths[b] and not isinstance(tables[a], int) and not isinstance(tables[b], int)]
                if pairs:
                    (a, b), w = pairs[0], widths[pairs[0][0]]
                    fired.append((a, b))
                    swapped = out.clone()
                    swapped[:, offs[a]:offs[a] + w] = out[:, offs[b]:offs[b] + w]
                    swapped[:, offs[b]:offs[b] + w] = out[:, offs[a]:offs[a] + w]
                    out = swapped
            return rows_concat(op, out, tables, idxs, **kw)
        return call
    return {"rows_concat": wrap}


def _shift_chosen_in_backward(fired):
    def wrap(segcat):
        def call(backward, scores, ptr, chosen, *args, **kw):
            if backward:  # the next row of the segment (mod its size) is taken for the chosen one
                fired.append(int(chosen.numel()))
                chosen = (chosen + 1) % (ptr[1:] - ptr[:-1]).clamp(min=1)
            return segcat(backward, scores, ptr, chosen, *args, **kw)
        return call
    return {"_segcat_call": wrap}


CONTROLS = {"scatter_add_drops_last_row": _drop_last_scatter_row, "segment_sum_last_offset_minus_one": _shorten_last_segment,
            "concat_backward_columns_swapped": _swap_concat_columns, "segcat_backward_chosen_shifted": _shift_chosen_in_backward}


def run_control(name, mb, ref, tensor_op, min_rows: int = 1, device="cuda:0"):
    """what `compare` reports (failures, rows) for the kernel path with control `name` switched on (the control must have fired)"""
    fired = []
    got, _ = run_fp32(*mb, min_rows=min_rows, device=device, sabotage=CONTROLS[name](fired))
    assert fired, name
    return compare(ref, tensor_op, got)


def _report():  # pragma: no cover - the tables of profiles/update_fp64.md
    import time

    dev = "cuda:0"
    print(f"factor {FACTOR:g}; ceilings: gradients {GRAD_CEILING:g}, executor head {EXEC_HEAD_CEILING:g}, other quantities {SCALAR_CEILING:g}\n")
    for case in ("small", "two_obs", "wide_head", "deep", "mix"):
        t0 = time.time()
        base = "small" if case == "two_obs" else case
        env = record(base, dev)
        mb = make_minibatch(env, 5, keep=TWO_OBS if case == "two_obs" else None)
        env.close()
        ref = reference_fp64(*mb)
        check_inputs(ref, mb[1], mb[2], CASES[base]["min_depth"], above_threshold=case == "mix")
        top, _ = run_fp32(*mb, min_rows=KERNELS_OFF)
        min_rows = 8192 if case == "mix" else 1
        sub = mb[1]
        print(f"## {case}\n\n{sub['n_obs']} observations, {sub['x'].shape[0]} nodes, {sub['src'].numel()} edges, {int(sub['stage_mask'].sum())} schedulable stages, "
              f"{sub['job_obs'].numel()} jobs, depth {int(sub['obs_depth'].max())}; MIN_ROWS = {min_rows}\n")
        for det in ((False, True) if case in ("small", "two_obs", "mix") else (False,)):
            got, counts = run_fp32(*mb, min_rows=min_rows, deterministic=det)
            failures, rows = compare(ref, top, got)
            print(f"### {'deterministic' if det else 'default'} mode\n\ncalls: {counts}\n\n{table(rows)}\n\nfailures: {failures or 'none'}\n")
        for name in (CONTROLS if case == "two_obs" else ("scatter_add_drops_last_row",) if case in ("small", "mix") else ()):
            f, rows = run_control(name, mb, ref, top, min_rows)
            worst = max(rows, key=lambda r: r[2] / r[3])
            print(f"control `{name}`: {'caught' if f else 'NOT caught'}, {len(f)} quantities out of bounds; the furthest out: `{worst[0]}`, "
                  f"error {worst[2]:.2e} = {worst[2] / worst[3]:.1f} x its bound\n")
        print(f"({time.time() - t0:.1f} s)\n")


if __name__ == "__main__":
    _report()
