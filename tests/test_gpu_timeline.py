"""-m gpu: the executor timelines on a real MI355X - the kernels that record them (csrc/sss_hip_sim_tl.hip, sss_hip_wide_tl.hip)
against the reference's histories (tests/golden/timeline_*.npz) on every path, the rasteriser kernel (csrc/sss_timeline.h)
against the numpy rasteriser, a 1024-env batch fused against step-wise with the record's invariants, and the arena / outputs
of the recording kernels against those of the plain ones."""
import numpy as np
import pytest
import torch

from spark_sched_sim_amd import SparkSchedSimEnv, VecSparkSchedSimEnv
from test_emu_timeline import render_cases, whole_episode_states
from timeline_util import HASH_NONE_PERMILLE, SETS, TimelineGolden, check_final, expected_frames, replay

pytestmark = pytest.mark.gpu

C1 = dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)


@pytest.mark.parametrize("name", list(SETS))
def test_step_replay_records_the_reference_histories_gpu(name, pack):
    tg = TimelineGolden(name)
    env, bad = replay(tg, tg.seeds, pack, "cuda:0")
    assert not bad, "\n".join(bad[:10])
    for k, s in enumerate(tg.seeds):
        assert env.timeline(k) == tg.history(s)
    env.close()


@pytest.mark.parametrize("name", ["c1_fair", "c1_hash", "c1_fifo", "c3_fair", "e100_hash", "e120_hash", "deep_c1_fair_beta"])
def test_fused_rollout_records_the_same_gpu(name, pack):
    tg = TimelineGolden(name)
    env = tg.make_env(tg.seeds, pack, "cuda:0")
    env.rollout(tg.policy, max(tg.steps(s) for s in tg.seeds), HASH_NONE_PERMILLE if tg.policy == "hash" else 0)
    bad = [m for k, s in enumerate(tg.seeds) for m in check_final(tg, env, k, s)]
    assert not bad, "\n".join(bad[:10])
    env.close()


@pytest.mark.parametrize("max_events", [1, 7])
@pytest.mark.parametrize("name", ["tiny_fair_tlimit", "stall", "c1_hash", "e120_hash"])
def test_bounded_steps_record_the_same_gpu(name, max_events, pack):
    tg = TimelineGolden(name)
    env, bad = replay(tg, tg.seeds, pack, "cuda:0", bounded=max_events, check_counts=False)
    assert not bad, "\n".join(bad[:10])
    env.close()


def test_overflow_keeps_the_prefix_gpu(pack):
    tg = TimelineGolden("c1_hash")
    seeds, cap, G = [100, 101], 4, 64
    env = tg.make_env(seeds, pack, "cuda:0", timeline=False)
    B, E = len(seeds), env.num_executors
    raw_t = torch.full((G + B * E * cap + G,), 12345.5, dtype=torch.float64, device="cuda:0")
    raw_j = torch.full((G + B * E * cap + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    raw_c = torch.full((G + B * E + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    env._timeline = (raw_t[G: G + B * E * cap].view(B, E, cap), raw_j[G: G + B * E * cap].view(B, E, cap), raw_c[G: G + B * E].view(B, E))
    env._bind_timeline()
    env.reset(seed=seeds, options={"time_limit": tg.time_limit})
    env, bad = replay(tg, seeds, pack, "cuda:0", cap=cap, env=env)
    assert not bad, "\n".join(bad[:10])
    for raw, fill in ((raw_t, 12345.5), (raw_j, 0x5A5A5A5A), (raw_c, 0x5A5A5A5A)):
        assert bool((raw[:G] == fill).all()) and bool((raw[-G:] == fill).all())
    with pytest.raises(RuntimeError, match="overflowed"):
        env.timeline(0)
    env.close()


def test_frames_equal_the_numpy_rasteriser_gpu(pack):
    for what, got, exp in render_cases(pack, "cuda:0", None):
        got = got.cpu().numpy()
        assert got.shape == exp.shape and np.array_equal(got, exp), (what, int((got != exp).any(axis=-1).sum()))


def test_frames_at_unaligned_addresses_gpu(pack):
    """the band writer's head / tail bytes: frames written at every byte offset mod 4, with guard bytes around them"""
    import ctypes as C

    from spark_sched_sim_amd.binding import SssTimelineRenderArgs
    tg = TimelineGolden("c1_fair")
    env = tg.make_env([0, 1], pack, "cuda:0")
    env.rollout("fair", 300)
    for W, H in ((33, 7), (1, 3), (130, 37)):
        exp = expected_frames(env, [0, 1], W, H)
        n = exp.size
        for off in range(4):
            raw = torch.full((64 + n + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
            base = 16 + ((-raw.data_ptr()) % 16) + off
            a = SssTimelineRenderArgs(None, 2, W, H, 0, raw.data_ptr() + base)
            env._b.check(env._b.lib.sss_timeline_render(env._h, C.byref(a), env._stream()))
            got = raw.cpu().numpy()
            assert np.array_equal(got[base: base + n].reshape(exp.shape), exp), (W, H, off)
            assert (got[:base] == 0x5A).all() and (got[base + n:] == 0x5A).all(), (W, H, off)
    env.close()


def test_large_batch_fused_equals_stepwise_with_invariants(pack):
    """1024 envs with distinct seeds: rollout("fair") and policy_actions + step_async leave the same records; release times
    never decrease and never exceed the clock; an executor that belongs to job j has an open entry of job j; count >= 1"""
    B, T, cap = 1024, 150, 128
    a = VecSparkSchedSimEnv(C1, B, device="cuda:0", pack=pack)
    b = VecSparkSchedSimEnv(C1, B, device="cuda:0", pack=pack)
    for e in (a, b):
        e.enable_timeline(cap)
        e.reset(seed=5000)
    a.rollout("fair", T)
    for _ in range(T):
        b.step_async(**b.policy_actions("fair"))
    torch.cuda.synchronize()
    (ta, ja, ca), (tb, jb, cb) = a.timeline_arrays(), b.timeline_arrays()
    assert torch.equal(ca, cb) and int(ca.min()) >= 1 and int(ca.max()) <= cap and int(ca.max()) > 3
    k = torch.arange(cap, device="cuda:0")[None, None, :]
    live = k < ca[:, :, None]
    closed = k < ca[:, :, None] - 1
    assert torch.equal(ja[live], jb[live])
    assert torch.equal(ta[closed].view(torch.int64), tb[closed].view(torch.int64))
    is_open = k == ca[:, :, None] - 1
    assert bool(torch.isnan(ta[is_open]).all()) and not bool(torch.isnan(ta[closed]).any())
    wall = a.header_field("wall_time")
    assert bool((torch.where(closed, ta, torch.zeros_like(ta)) <= wall[:, None, None]).all())
    nxt = torch.where(closed[:, :, 1:], ta[:, :, 1:], torch.full_like(ta[:, :, 1:], float("inf")))
    prev = torch.where(closed[:, :, 1:], ta[:, :, :-1], torch.zeros_like(ta[:, :, 1:]))
    assert bool((prev <= nxt).all()) and bool((torch.where(closed, ta, torch.zeros_like(ta)) >= 0).all())
    # executor.job_id (SssHot::ex_job) against the open entries
    from spark_sched_sim_amd.vec_env import HOT_EX_JOB_OFF
    off = HOT_EX_JOB_OFF[64]
    hot = a._env_view[:, off: off + 2 * C1["num_executors"]].contiguous().view(torch.int16).int()
    open_job = ja.gather(2, (ca[:, :, None] - 1).long()).squeeze(2)
    at_job = hot >= 0
    assert int(at_job.sum()) > 0 and torch.equal(open_job[at_job], hot[at_job])
    a.close(), b.close()


def test_recording_kernels_leave_the_same_arena_and_outputs_gpu(pack):
    never, unbound, bound = whole_episode_states(pack, "cuda:0", None)
    for other in (unbound, bound):
        for x, y in zip(never, other):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_facade_rgb_array_gpu(pack):
    tg = TimelineGolden("c1_fifo")
    env = SparkSchedSimEnv(dict(tg.cfg, render_mode="rgb_array"), device="cuda:0")
    env.reset(seed=5)
    st, ne = tg.actions(5)
    for i in range(tg.steps(5)):
        env.step({"stage_idx": int(st[i]), "num_exec": int(ne[i])})
    assert [e.history for e in env.executors] == tg.history(5)
    frame = env.render()
    assert frame.shape == (300, 400, 3) and np.array_equal(frame, expected_frames(env._vec, [0], 400, 300)[0])
    env.close()
