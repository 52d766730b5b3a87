"""Differential (average-reward) returns on the GPU: the window kernels and the returns kernel of csrc/sss_returns.h (include/sss.h
sss_reward_window_update / sss_differential_returns) against the reference's recorded numbers and the host class
training.DifferentialReturns - bit for bit -, PPO.preprocess with `reward_buff_cap` without a synchronising call, and twin
deterministic training runs."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def test_reference_fixture_is_reproduced_exactly():
    from differential_util import check_reference_fixture

    check_reference_fixture(None, DEV)


def test_random_records_match_the_host_class_bit_for_bit():
    from differential_util import check_random_records

    check_random_records(None, DEV)


def test_config5_share_record_matches_the_host_class_bit_for_bit():
    """one rank's share of BASELINE config 5: T = 7441 steps, 1024 envs, the reference's window of 200 000 rows; two calls (the
    first one brings millions of rows for a 200 000-row window, the second one again: every slot is rewritten through the overflow
    path) and a third, short record that shifts the window by a few thousand rows"""
    from differential_util import compare_with_host_class, random_record

    gen = torch.Generator().manual_seed(77)
    T, B = 7441, 1024
    lengths = torch.randint(T // 3, T + 1, (B,), generator=gen)
    lengths[5], lengths[1000] = 0, T
    recs = [random_record(gen, T, B, lengths=lengths), random_record(gen, T, B, lengths=lengths.flip(0)), random_record(gen, 90, B, zero_frac=0.5)]
    host, devc = compare_with_host_class(None, DEV, 200_000, recs, "config 5 share")
    assert np.isfinite(devc.avg_num_jobs) and devc.avg_num_jobs > 0


def test_window_far_above_the_row_count_and_sums_at_200k():
    """cap = 200 000 with a record of a few thousand rows: most of the window stays zero and the ordered sums still walk all of it"""
    from differential_util import compare_with_host_class, random_record

    gen = torch.Generator().manual_seed(78)
    compare_with_host_class(None, DEV, 200_000, [random_record(gen, 300, 40), random_record(gen, 500, 64)], "sparse window")


def test_more_envs_than_one_round_of_the_scan():
    """B above the 1024 envs the scan's workgroup takes per round (the running total carried from round to round), short T"""
    from differential_util import compare_with_host_class, random_record

    gen = torch.Generator().manual_seed(79)
    compare_with_host_class(None, DEV, 20_000, [random_record(gen, 70, 1025), random_record(gen, 9, 2500), random_record(gen, 130, 3000)], "B > 1024")
    compare_with_host_class(None, DEV, 1000, [random_record(gen, 66, 2049)], "B > 1024, overflow")


def _collected_record():
    from decima_util import AGENT
    from spark_sched_sim_amd.training import Trainer

    train = dict(trainer_cls="PPO", num_iterations=1, num_sequences=4, num_rollouts=4, seed=5, checkpointing_freq=50, num_epochs=1, num_batches=2,
                 clip_range=0.2, target_kl=0.01, entropy_coeff=0.04, reward_buff_cap=3000, opt_cls="Adam", opt_kwargs=dict(lr=3.0e-4), max_grad_norm=0.5)
    env = dict(num_executors=10, job_arrival_cap=10, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0, mean_time_limit=1.0e6)
    tr = Trainer(dict(AGENT, agent_cls="DecimaScheduler"), env, train, device=DEV)
    tr.policy.eval()
    return tr, tr.collector.collect_sync()


def test_preprocess_picks_the_device_class_and_does_not_synchronise():
    from differential_util import bits
    from spark_sched_sim_amd.training import DeviceDifferentialReturns, DifferentialReturns

    tr, ro = _collected_record()
    assert type(tr.ppo.diff) is DifferentialReturns and int(ro.active.sum()) > 100  # (no record seen yet)
    host = DifferentialReturns(3000)
    tr.ppo.preprocess(ro)  # (first call: the record is on the GPU -> the device class; the window tensors are created, code objects load)
    assert type(tr.ppo.diff) is DeviceDifferentialReturns
    host(ro)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        returns, baselines = tr.ppo.preprocess(ro)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    want = host(ro)
    assert np.array_equal(bits(returns), bits(want))
    assert bits(tr.ppo.diff.avg_num_jobs) == bits(float(host.avg_num_jobs))
    assert np.array_equal(bits(tr.ppo.diff.data), bits(host.data))
    assert baselines.shape == returns.shape and bool(torch.isfinite(baselines).all())
    tr.close()


TWIN = textwrap.dedent("""
    import hashlib, sys, tempfile
    sys.path[:0] = [%r, %r]
    import torch
    from decima_util import AGENT
    from spark_sched_sim_amd import training
    with tempfile.TemporaryDirectory() as tmp:
        train = dict(trainer_cls="PPO", num_iterations=3, num_sequences=4, num_rollouts=4, seed=11, checkpointing_freq=50,
                     num_epochs=2, num_batches=3, clip_range=0.2, target_kl=None, entropy_coeff=0.04, reward_buff_cap=4000,
                     opt_cls="Adam", opt_kwargs=dict(lr=3.0e-4), max_grad_norm=0.5, artifacts_dir=tmp, deterministic=True)
        env = dict(num_executors=10, job_arrival_cap=12, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0, mean_time_limit=2.0e6)
        tr = training.Trainer(dict(AGENT, agent_cls="DecimaScheduler"), env, train, device="cuda:0")
        hist = tr.train(verbose=False)
        assert type(tr.ppo.diff) is training.DeviceDifferentialReturns
        h = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        for k, v in tr.policy.state_dict().items():
            print("param", k, h(v))
        for rec in hist:
            print("avg_num_jobs", float(rec["avg_num_jobs"]).hex())
        print("window", hashlib.sha256(tr.ppo.diff.data.tobytes()).hexdigest())
        tr.close()
""") % (os.path.dirname(HERE), HERE)


def test_twin_deterministic_runs_with_differential_returns_agree(tmp_path):
    """Trainer(reward_buff_cap=.., deterministic=True), 3 iterations, twice in fresh processes: identical parameters and an
    identical avg_num_jobs history (the window's sums are ordered by definition: there is nothing to switch)"""
    script = tmp_path / "twin.py"
    script.write_text(TWIN)
    outs = []
    for _ in range(2):
        res = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=400)
        assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
        outs.append(res.stdout)
    lines = outs[0].strip().splitlines()
    assert sum(l.startswith("avg_num_jobs") for l in lines) == 3 and any(l.startswith("param") for l in lines)
    assert all("nan" not in l for l in lines if l.startswith("avg_num_jobs"))
    assert outs[1] == outs[0]
