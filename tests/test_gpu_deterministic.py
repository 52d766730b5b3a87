"""The deterministic PPO mode on the GPU: `SSS_ROWS_ORDERED_ADD` (csrc/sss_rows.h), the autograd functions of
spark_sched_sim_amd.train_kernels under `torch.use_deterministic_algorithms(True)`, and twin training runs that must end with
the same bits"""
import contextlib
import os
import subprocess
import sys
import textwrap

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


@contextlib.contextmanager
def torch_flag(on: bool = True):
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


def test_ordered_add_kernel():
    """bit for bit against the in-order host sum at n = 100 003; the 16-byte and the 4-byte forms give the same bits; against
    index_add_ within check_rows_ops' tolerance"""
    from deterministic_util import check_ordered_add, check_rejected_ops

    from spark_sched_sim_amd.binding import Binding
    from spark_sched_sim_amd.train_kernels import ROWS_ORDERED_ADD, rows_op

    b = Binding()
    forms = check_ordered_add(b, DEV, n=100_003, seed=7)
    for width in (16, 36, 64):  # whole list: 16 bytes per lane; column slice at offset 3 of rows of width + 7: 4 bytes per lane
        for p_none in (True, False):
            assert torch.equal(forms[(width, p_none, "whole")], forms[(width, p_none, "slice")]), (width, p_none)
    check_rejected_ops(b, DEV)
    gen = torch.Generator().manual_seed(2)
    n, rows = 100_003, 33_334  # (check_rows_ops' shape: ~3 rows per key - long runs are checked bit for bit above)
    for width in (1, 5, 16, 21, 64):
        keys = torch.sort(torch.randint(0, rows, (n,), generator=gen))[0].to(DEV)
        perm = torch.randperm(n, generator=gen).to(DEV)
        src = torch.randn((n, width + 4), generator=gen).to(DEV)
        table = torch.randn((rows, width), generator=gen).to(DEV)
        for a in (src[:, :width].contiguous(), src[:, 2:2 + width]):
            acc = table.clone()
            rows_op(ROWS_ORDERED_ADD, keys, a, acc, perm=perm)
            assert torch.allclose(acc, table.clone().index_add_(0, keys, a[perm]), rtol=1e-5, atol=1e-5), width


def test_autograd_functions_under_the_flag_repeat_and_match_the_default_forms():
    """concat_rows (sorted hint and not), gather_rows (with repeats) and segment_sum("") forward and backward under the flag:
    the same bits twice, and the default (atomic) forms' values within test_rows_kernels_match_torch_indexing's tolerances"""
    from spark_sched_sim_amd.train_kernels import concat_rows, gather_rows, segment_sum

    torch.manual_seed(5)
    n, rows = 50_000, 9_000
    t1 = torch.randn((rows, 16), device=DEV, requires_grad=True)
    t2 = torch.randn((rows // 3, 16), device=DEV, requires_grad=True)
    x = torch.randn((rows, 5), device=DEV)
    i1, i2 = torch.randint(0, rows, (n,), device=DEV), torch.randint(0, rows // 3, (n,), device=DEV)
    s1, s2 = torch.sort(i1)[0], torch.sort(i2)[0]
    w = torch.randn((n, 37), device=DEV)
    y = torch.randn((n, 16), device=DEV, requires_grad=True)
    wv = torch.randn((rows, 16), device=DEV)

    def run():
        out = []
        for (a, b), hint in (((i1, i2), False), ((s1, s2), True), ((s1, i2), (False, True, False))):
            got = concat_rows([(x, a), (t1, a), (t2, b)], sorted_idx=hint)
            out.append((got.detach(),) + torch.autograd.grad((got * w).sum(), (t1, t2)))
        out.append(torch.autograd.grad((gather_rows(t1, i1) * w[:, :16]).sum(), t1))
        s = segment_sum(y, i1, rows, "")
        out.append((s.detach(),) + torch.autograd.grad((s * wv).sum(), y))
        return out

    with torch_flag():
        first, second = run(), run()
    default = run()
    for ta, tb, tc in zip(first, second, default):
        for a, b, c in zip(ta, tb, tc):
            assert torch.equal(a, b)
            assert torch.allclose(a, c, rtol=1e-4, atol=1e-4)
    with torch_flag():  # (the sorted hint saves the sort, it changes no bit)
        plain = torch.autograd.grad((concat_rows([(x, s1), (t1, s1), (t2, s2)]) * w).sum(), (t1, t2))
    assert all(torch.equal(a, b) for a, b in zip(first[1][1:], plain))


@pytest.fixture(scope="module")
def deep_minibatch():
    """a recorded minibatch of the deep trace set (fan-in, up to 12 DAG layers) large enough for every row kernel: the compact
    graph of one step of 2048 envs, actions sampled by the policy, made-up advantages and old log-probabilities"""
    from decima_util import AGENT
    from spark_sched_sim_amd import VecSparkSchedSimEnv, workload
    from spark_sched_sim_amd.decima import DecimaPolicy, select_observations

    cfg = dict(num_executors=10, job_arrival_cap=20, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)
    env = VecSparkSchedSimEnv(cfg, 2048, device=DEV, pack=workload.profile_pack("deep"), auto_reset=True)
    env.reset(seed=13)
    env.rollout("fair", 120)
    g = env.decima_graph(None)
    torch.manual_seed(9)
    pol = DecimaPolicy(num_executors=10, **AGENT, opt_cls="Adam", opt_kwargs=dict(lr=3e-4), max_grad_norm=0.5).to(DEV)
    with torch.no_grad():  # (biases start at zero: give them values so that their gradients are exercised)
        for name, p in pol.named_parameters():
            if "bias" in name:
                p.normal_(0.0, 0.1)
    a = pol.act(g, torch.Generator(device=DEV).manual_seed(1), fresh_outputs=True)
    keep = a["any_stage"].nonzero(as_tuple=True)[0]
    sub = select_observations(g, keep)
    acts = [a[k][keep].long() for k in ("stage_sel", "job_idx", "exec_sel")]
    gen = torch.Generator(device=DEV).manual_seed(3)
    adv = torch.randn(keep.numel(), device=DEV, generator=gen, dtype=torch.float64)
    old = (a["lgprob"][keep] + 0.05 * torch.randn(keep.numel(), device=DEV, generator=gen)).float()
    env.close()
    from spark_sched_sim_amd import train_kernels
    assert sub["x"].shape[0] >= train_kernels.MIN_ROWS and int(sub["stage_mask"].sum()) >= train_kernels.MIN_ROWS
    assert int(sub["obs_depth"].max()) >= 6
    # every network takes part: a minibatch in which no chosen job allows more than one executor count gives the executor head
    # gradients of exactly 0.0, and "the two modes agree" is then 0 <= 0 there (the two last biases: zero by the softmax's shift invariance)
    _, grads = _loss_and_grads(pol, sub, acts, adv, old)
    pol.zero_grad()
    for k, gr in grads.items():
        if k not in ("stage_policy_network.mlp_score.4.bias", "exec_policy_network.mlp_score.4.bias"):
            assert float(gr.abs().max()) > 0.0, k
    return pol, sub, acts, adv, old


def _loss_and_grads(pol, sub, acts, adv, old):
    from spark_sched_sim_amd.training import ppo_loss

    pol.zero_grad()
    loss, _ = ppo_loss(pol, sub, *acts, adv, old, 0.2, 0.04)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in pol.named_parameters()}


def test_ppo_update_under_the_flag_launches_no_atomic_sums(deep_minibatch, monkeypatch):
    """one ppo_loss + backward on the recorded deep-set minibatch under the flag: no ROWS_SCATTER_ADD and no concat op 1
    launched, at least one ROWS_ORDERED_ADD; the loss and every gradient the same bits twice"""
    from spark_sched_sim_amd import train_kernels as tk

    ops, concat_ops = [], []
    rows_op, rows_concat = tk.rows_op, tk.rows_concat

    def spy_rows(op, *args, **kw):
        ops.append(op)
        return rows_op(op, *args, **kw)

    def spy_concat(op, *args, **kw):
        concat_ops.append(op)
        return rows_concat(op, *args, **kw)

    monkeypatch.setattr(tk, "rows_op", spy_rows)
    monkeypatch.setattr(tk, "rows_concat", spy_concat)
    with torch_flag():
        first = _loss_and_grads(*deep_minibatch)
        assert tk.ROWS_SCATTER_ADD not in ops and 1 not in concat_ops, (sorted(set(ops)), sorted(set(concat_ops)))
        assert ops.count(tk.ROWS_ORDERED_ADD) >= 6, ops.count(tk.ROWS_ORDERED_ADD)
        second = _loss_and_grads(*deep_minibatch)
    assert torch.equal(first[0], second[0])
    for k in first[1]:
        assert torch.equal(first[1][k], second[1][k]), k
    ops.clear()
    _loss_and_grads(*deep_minibatch)  # (the default mode does use the atomic forms on this minibatch)
    assert tk.ROWS_SCATTER_ADD in ops and tk.ROWS_ORDERED_ADD not in ops


def test_deterministic_and_default_gradients_agree(deep_minibatch):
    """the same minibatch and parameters, before any optimiser step: the loss and every parameter gradient of the two modes
    agree to 1e-4 of each gradient tensor's largest entry (the order of the additions is the only difference)"""
    loss_d, grads_d = None, None
    with torch_flag():
        loss_d, grads_d = _loss_and_grads(*deep_minibatch)
    loss_f, grads_f = _loss_and_grads(*deep_minibatch)
    assert torch.allclose(loss_d, loss_f, rtol=1e-5, atol=1e-6)
    for k in grads_f:
        a, b = grads_d[k], grads_f[k]
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-4 * max(scale, 1e-12), (k, float((a - b).abs().max()), scale)


def test_message_passing_under_the_flag(deep_minibatch):
    """_MessagePassFn alone (the node encoder on the kernel path) under the flag: embeddings and gradients the same bits twice,
    and within test_message_passing_function_matches_the_tensor_op_form's tolerances of the default form"""
    pol, sub = deep_minibatch[0], deep_minibatch[1]
    enc = pol.encoder.node_encoder
    w = torch.randn((sub["x"].shape[0], 16), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))

    def run():
        pol.zero_grad()
        h = enc(sub, per_obs_skip=False)
        assert enc._kernel_message_passing(enc.mlp_prep(sub["x"]))
        (h * w).sum().backward()
        return h.detach().clone(), {k: p.grad.clone() for k, p in enc.named_parameters()}

    with torch_flag():
        first, second = run(), run()
    default = run()
    assert torch.equal(first[0], second[0]) and all(torch.equal(first[1][k], second[1][k]) for k in first[1])
    assert torch.allclose(first[0], default[0], rtol=1e-4, atol=2e-5)
    for k in first[1]:
        a, b = first[1][k], default[1][k]
        assert torch.allclose(a, b, rtol=2e-3, atol=2e-3 * max(1.0, float(b.abs().max()))), k


TWIN = textwrap.dedent("""
    import hashlib, sys, tempfile
    sys.path[:0] = [%r, %r]
    import torch
    from decima_util import AGENT
    from spark_sched_sim_amd import train_kernels as tk, training, workload
    fill = sys.argv[1] == "fill"
    if fill:  # the same training with torch's fill of uninitialised memory on: no result may depend on that memory
        scope = training.deterministic_scope
        training.deterministic_scope = lambda fill_uninitialized_memory=False: scope(fill_uninitialized_memory=True)
    n6 = [0]
    rows_op = tk.rows_op
    def spy(op, *a, **kw):
        n6[0] += op == tk.ROWS_ORDERED_ADD
        return rows_op(op, *a, **kw)
    tk.rows_op = spy
    with tempfile.TemporaryDirectory() as tmp:
        train = dict(trainer_cls="PPO", num_iterations=2, num_sequences=8, num_rollouts=4, seed=11, checkpointing_freq=50,
                     num_epochs=2, num_batches=3, clip_range=0.2, target_kl=None, entropy_coeff=0.04, beta_discount=5.0e-3,
                     opt_cls="Adam", opt_kwargs=dict(lr=3.0e-4), max_grad_norm=0.5, artifacts_dir=tmp)
        env = dict(num_executors=10, job_arrival_cap=20, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0, mean_time_limit=2.0e7)
        tr = training.Trainer(dict(AGENT, agent_cls="DecimaScheduler"), env, train, device="cuda:0", pack=workload.profile_pack("deep"), deterministic=True)
        hist = tr.train(verbose=False)
        assert not torch.are_deterministic_algorithms_enabled()
        h = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        for k, v in tr.policy.state_dict().items():
            print("param", k, h(v))
        for pid, st in sorted(tr.policy.optim.state_dict()["state"].items()):
            for k, v in sorted(st.items()):
                print("adam", pid, k, h(v) if torch.is_tensor(v) else repr(v))
        for rec in hist:
            print("history", repr(sorted(rec.items())))
        tr.close()
    print("op6", n6[0])
""") % (os.path.dirname(HERE), HERE)


def test_twin_training_runs_give_the_same_bits(tmp_path):
    """Trainer(deterministic=True), 2 iterations on the deep trace set, in three fresh processes one after the other: the
    parameters, Adam's state and the history agree bit for bit, also with torch's fill of uninitialised memory on"""
    script = tmp_path / "twin.py"
    script.write_text(TWIN)
    outs = []
    for mode in ("plain", "plain", "fill"):
        res = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=400)
        assert res.returncode == 0, (mode, res.returncode, res.stdout[-2000:], res.stderr[-4000:])
        outs.append(res.stdout)
    n6 = int(outs[0].strip().splitlines()[-1].split()[1])
    assert n6 > 0 and "param" in outs[0] and "adam" in outs[0]
    assert outs[1] == outs[0]
    assert outs[2] == outs[0]


def test_trainer_restores_the_flag_and_the_sync_pipeline_holds_under_it(tmp_path):
    from decima_util import AGENT
    from training_util import check_sync_pipeline

    from spark_sched_sim_amd.training import Trainer

    train = dict(trainer_cls="PPO", num_iterations=1, num_sequences=2, num_rollouts=2, seed=42, checkpointing_freq=50,
                 num_epochs=1, num_batches=2, clip_range=0.2, target_kl=0.01, entropy_coeff=0.04, beta_discount=5.0e-3,
                 opt_cls="Adam", opt_kwargs=dict(lr=3.0e-4), max_grad_norm=0.5, artifacts_dir=str(tmp_path), deterministic=True)
    env = dict(num_executors=10, job_arrival_cap=10, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0, mean_time_limit=1.0e6)
    tr = Trainer(dict(AGENT, agent_cls="DecimaScheduler"), env, train, device=DEV)
    assert tr.deterministic
    import torch.utils.deterministic as tud
    for before in ((False, False), (True, True)):
        with torch_flag(before[0]):
            if before[0]:
                torch.use_deterministic_algorithms(True, warn_only=True)
            tr.train(verbose=False)
            assert (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()) == before
            assert tud.fill_uninitialized_memory
    tr.close()
    with torch_flag():
        check_sync_pipeline(DEV, None)
