"""The PPO update's kernel path end to end - `ppo_loss(...)` + `.backward()` with every operator of spark_sched_sim_amd.train_kernels
inside the real graph wiring - against the same update in fp64 on the CPU, which uses none of those kernels (update_fp64_util).
Tolerances come from the fp32 tensor-op form's own error against fp64, measured in the same run; the measured tables are in
profiles/update_fp64.md."""
import pytest
import torch

import update_fp64_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOTH_MODES = ("small", "two_obs", "mix")


@pytest.fixture(scope="module")
def prepared():
    """case -> (minibatch, fp64 update, fp32 tensor-op update on the GPU), made once per case: the input conditions hold on the
    reference, and with the kernels off no kernel entry point is called"""
    cache = {}

    def get(case):
        if case not in cache:
            base = "small" if case == "two_obs" else case
            env = U.record(base, DEV)
            made = {base: U.make_minibatch(env, 5)}
            if base == "small":
                made["two_obs"] = U.make_minibatch(env, 5, keep=U.TWO_OBS)
            env.close()
            for k, mb in made.items():
                ref = U.reference_fp64(*mb)
                U.check_inputs(ref, mb[1], mb[2], U.CASES[base]["min_depth"], above_threshold=k == "mix")
                top, counts = U.run_fp32(*mb, min_rows=U.KERNELS_OFF)
                assert not any(counts.values()), counts
                cache[k] = (mb, ref, top)
        return cache[case]
    return get


@pytest.mark.parametrize("case,deterministic", [(c, False) for c in ("small", "two_obs", "wide_head", "deep", "mix")] + [(c, True) for c in BOTH_MODES])
def test_kernel_update_matches_the_fp64_update(prepared, case, deterministic):
    """embeddings, stage scores, log-probabilities, entropies, the loss and every entry of every parameter gradient (but the two
    shift-invariant scalars) within 4 x the tensor-op form's own error of fp64; every kernel entry point was called. Deterministic
    mode: the same bounds, and a second run gives the same bits."""
    from spark_sched_sim_amd import train_kernels as tk

    mb, ref, top = prepared(case)
    min_rows = tk.MIN_ROWS if case == "mix" else 1  # (mix: the product's own threshold, unpatched - some operators above it, some below)
    assert tk.MIN_ROWS == 8192
    got, counts = U.run_fp32(*mb, min_rows=min_rows, deterministic=deterministic)
    assert all(v > 0 for v in counts.values()), counts
    failures, rows = U.compare(ref, top, got)
    print(f"{case}, {'deterministic' if deterministic else 'default'} mode, calls {counts}\n{U.table(rows)}")
    assert not failures, failures
    if deterministic:
        again, _ = U.run_fp32(*mb, min_rows=min_rows, deterministic=True)
        assert U.same_bits(got, again)


def test_wide_head_has_long_executor_segments(prepared):
    mb = prepared("wide_head")[0]
    sub, job_idx = mb[1], mb[2][1]
    cap = sub["job_cap"][U._excl_cumsum(sub["obs_jobs"].long()) + job_idx]
    assert int(cap.max()) > 64 and int(cap.clamp(max=100).sum()) >= 500


@pytest.mark.parametrize("control", list(U.CONTROLS))
def test_the_comparison_fails_a_subtly_wrong_kernel_result(prepared, control):
    """negative controls on `two_obs`: a Python entry point hands on a slightly wrong value (a list row left out, a segment one row
    short, two parts' gradient columns swapped, the neighbour of the chosen row) - `compare` must report it"""
    mb, ref, top = prepared("two_obs")
    failures, _ = U.run_control(control, mb, ref, top)
    print(control, len(failures), failures[:3])
    assert failures
