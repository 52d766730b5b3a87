"""The inputs and the reference of tests/test_gpu_update_fp64.py, checkable without a GPU: the cases are recorded with the emulator
library, the input conditions are asserted on the fp64 update, and the fp32 tensor-op update on the CPU stays within the ceilings of
it (the reference pinned against itself: `update_fp64_util.compare` sizes the kernels' tolerances from exactly this error)"""
import pytest
import torch

import update_fp64_util as U
from emu_util import load_emu


@pytest.fixture(scope="module")
def recorded():
    """{case: (minibatch, fp64 update)}; `two_obs` is cut from the env of `small`"""
    out = {}
    for case in ("small", "wide_head"):
        env = U.record(case, "cpu", load_emu())
        out[case] = U.make_minibatch(env, 5)
        if case == "small":
            out["two_obs"] = U.make_minibatch(env, 5, keep=U.TWO_OBS)
        env.close()
    return {k: (mb, U.reference_fp64(*mb)) for k, mb in out.items()}


@pytest.mark.parametrize("case", ["small", "two_obs", "wide_head"])
def test_inputs_meet_their_conditions_and_fp32_tensor_ops_stay_under_the_ceilings(recorded, case):
    mb, ref = recorded[case]
    sub = mb[1]
    U.check_inputs(ref, sub, mb[2], U.CASES["small" if case == "two_obs" else case]["min_depth"])
    if case == "two_obs":
        assert sub["n_obs"] == 2
    if case == "wide_head":  # executor softmax segments of up to 100 rows
        cap = sub["job_cap"][U._excl_cumsum(sub["obs_jobs"].long()) + mb[2][1]]
        assert int(cap.max()) > 64 and int(cap.clamp(max=100).sum()) >= 500
    top, counts = U.run_fp32(*mb, min_rows=U.KERNELS_OFF, device="cpu")
    assert not any(counts.values()), counts
    failures, rows = U.compare(ref, top)
    print(U.table(rows))
    assert not failures, failures


def test_the_minibatch_is_cut_in_permuted_order_and_its_actions_are_in_range(recorded):
    mb, _ = recorded["small"]
    pol, sub, (stage_sel, job_idx, exec_sel), adv, old = mb
    n_sched = torch.zeros(sub["n_obs"], dtype=torch.long).index_add_(0, sub["node_obs"], sub["stage_mask"].long())
    assert bool((n_sched > 0).all()) and bool(((stage_sel >= 0) & (stage_sel < n_sched)).all())
    assert bool(((job_idx >= 0) & (job_idx < sub["obs_jobs"])).all())
    cap = sub["job_cap"][U._excl_cumsum(sub["obs_jobs"].long()) + job_idx]
    assert bool(((exec_sel >= 0) & (exec_sel < cap.clamp(min=1, max=pol.num_executors))).all())
    assert adv.dtype == torch.float64 and old.dtype == torch.float32 and adv.numel() == old.numel() == sub["n_obs"]
    # (the observations' node counts in arena order would ascend with the env id only by accident: the cut is a permutation)
    perm = torch.randperm(U.CASES["small"]["envs"], generator=torch.Generator().manual_seed(U.PERM_SEED))
    assert not torch.equal(perm, torch.sort(perm)[0]) and sub["n_obs"] <= perm.numel()


def test_compare_reports_a_wrong_gradient_and_an_ill_conditioned_case(recorded):
    """`compare` on made-up results: the tensor-op form itself passes; one entry of one gradient tensor off by 1e-3 of the tensor's
    largest entry fails that tensor alone; a tensor-op form that is itself far from the reference fails as ill-conditioned"""
    mb, ref = recorded["two_obs"]
    top, _ = U.run_fp32(*mb, min_rows=U.KERNELS_OFF, device="cpu")
    assert U.compare(ref, top, top)[0] == []
    name = "encoder.node_encoder.mlp_msg.2.weight"
    bad = dict(top, grads={k: v.clone() for k, v in top["grads"].items()})
    bad["grads"][name].view(-1)[7] += 1e-3 * float(ref["grads"][name].abs().max())
    failures = U.compare(ref, top, bad)[0]
    assert len(failures) == 1 and failures[0].startswith("grad " + name), failures
    noisy = dict(top, grads={k: v * (1.01 if k == name else 1.0) for k, v in top["grads"].items()})
    failures = U.compare(ref, noisy, top)[0]
    assert any("ill-conditioned" in f and name in f for f in failures), failures
