"""Executor timelines (include/sss.h sss_bind_timeline / sss_timeline_render; csrc/sss_sim.h tl_append, csrc/sss_timeline.h) under
the CPU wave emulator: the rows the kernels record equal the reference's `Executor.history` (tests/golden/
make_timeline_golden.py replays the recorded action streams in the reference) after every step and at the end, bit for bit, in
both instantiations and on every path (step, bounded step, fused rollout); resets restart rows, skipped envs keep them; a
capacity that is too small loses nothing but the entries beyond it and writes nowhere else; with nothing bound the env is
byte for byte what it is without the feature; frames equal a numpy rasteriser written from the header's rules."""
import ctypes as C
import glob
import os
import os.path as osp
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from emu_util import load_emu
from spark_sched_sim_amd import SparkSchedSimEnv, VecSparkSchedSimEnv
from spark_sched_sim_amd.binding import SssTimeline, SssTimelineRenderArgs
from spark_sched_sim_amd.vec_env import HDR_PROF
from timeline_util import HASH_NONE_PERMILLE, SETS, TimelineGolden, check_final, expected_frames, replay

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(HERE)
SKIP = -2147483648
TINY = dict(num_executors=5, job_arrival_cap=8, job_arrival_rate=1.0e-4, moving_delay=1500.0, warmup_delay=500.0)


@pytest.mark.parametrize("name", list(SETS))
def test_step_replay_records_the_reference_histories(name, pack):
    """every set, every seed: counts after every step, entries at the end"""
    tg = TimelineGolden(name)
    env, bad = replay(tg, tg.seeds, pack, "cpu", load_emu())
    assert not bad, "\n".join(bad[:10])
    for k, s in enumerate(tg.seeds):   # ... and in the reference's own shape
        assert env.timeline(k) == tg.history(s)
    env.close()


@pytest.mark.parametrize("name,seeds", [("c1_fair", [0, 1]), ("c1_hash", [100]), ("c1_fifo", [5]), ("e100_hash", [2]), ("deep_c1_fair_beta", [4])])
def test_fused_rollout_records_the_same(name, seeds, pack):
    tg = TimelineGolden(name)
    env = tg.make_env(seeds, pack, "cpu", load_emu())
    env.rollout(tg.policy, max(tg.steps(s) for s in seeds), HASH_NONE_PERMILLE if tg.policy == "hash" else 0)
    bad = [m for k, s in enumerate(seeds) for m in check_final(tg, env, k, s)]
    assert not bad, "\n".join(bad[:10])
    env.close()


@pytest.mark.parametrize("max_events", [1, 7])
@pytest.mark.parametrize("name,seeds", [("tiny_fair_tlimit", [0, 1, 2, 3]), ("stall", [2002]), ("c1_fair", [2]), ("e120_hash", [1])])
def test_bounded_steps_record_the_same(name, seeds, max_events, pack):
    """a step cut at its event budget writes its entries as the events happen: same counts after every step, same final record"""
    tg = TimelineGolden(name)
    env, bad = replay(tg, seeds, pack, "cpu", load_emu(), bounded=max_events)
    assert not bad, "\n".join(bad[:10])
    env.close()


def _arrays(env):
    return [x.clone() for x in env.timeline_arrays()]


@pytest.mark.parametrize("fused", [0, 1])
def test_auto_reset_restarts_the_rows(fused, pack):
    """an env that starts its next episode inside a step / rollout launch: its rows are those of a fresh env reset with that seed"""
    lib = load_emu()
    a = VecSparkSchedSimEnv(TINY, 2, device="cpu", pack=pack, _lib=lib, auto_reset=True, seed_stride=7)
    a.enable_timeline(64)
    a.reset(seed=[3, 4])
    for _ in range(400):
        if fused:
            a.rollout("fair", 1)
        else:
            a.step_async(**a.policy_actions("fair"))
        if all(a.header(k)["seed"] != 3 + k and a.header(k)["ep_steps"] >= 15 for k in range(2)):   # both are in a later episode
            break
    hdr = [a.header(k) for k in range(2)]
    for k in range(2):
        b = VecSparkSchedSimEnv(TINY, 1, device="cpu", pack=pack, _lib=lib)
        b.enable_timeline(64)
        b.reset(seed=[hdr[k]["seed"]])
        assert hdr[k]["seed"] > 3 + k and (hdr[k]["seed"] - 3 - k) % 7 == 0
        b.rollout("fair", hdr[k]["ep_steps"])
        assert b.header(0)["wall_time"] == hdr[k]["wall_time"]
        # (entries beyond count are whatever the previous episode left there: the record is count and the entries below it)
        assert torch.equal(a.timeline_arrays()[2][k], b.timeline_arrays()[2][0])
        assert a.timeline(k) == b.timeline(0) and max(len(h) for h in a.timeline(k)) > 1
        b.close()
    a.close()


def test_masked_reset_and_skipped_envs(pack):
    env = VecSparkSchedSimEnv(TINY, 3, device="cpu", pack=pack, _lib=load_emu())
    env.enable_timeline(32)
    env.reset(seed=[0, 1, 2])
    env.rollout("fair", 12)
    before = _arrays(env)
    assert int(before[2].max()) > 1
    env.reset(seed=[0, 1, 2], mask=torch.tensor([0, 1, 0], dtype=torch.uint8))
    after = _arrays(env)
    for k in (0, 2):   # not in the mask: untouched
        for x, y in zip(before, after):
            assert torch.equal(torch.nan_to_num(x[k], nan=-1.0), torch.nan_to_num(y[k], nan=-1.0))
    assert env.timeline(1) == [[[None, -1]] for _ in range(TINY["num_executors"])]
    # SSS_SKIP_ENV: env 0 sits the steps out, env 2 goes on
    for _ in range(30):
        act = env.policy_actions("fair")
        si = act["stage_idx"].clone()
        si[0] = SKIP
        env.step_async(si, act["num_exec"])
    later = _arrays(env)
    for x, y in zip(before, later):
        assert torch.equal(torch.nan_to_num(x[0], nan=-1.0), torch.nan_to_num(y[0], nan=-1.0))
    assert int(later[2][1].sum()) > TINY["num_executors"] and not torch.equal(later[2][2], before[2][2])
    env.close()


def test_overflow_keeps_the_prefix_and_writes_nowhere_else(pack):
    """cap = 4 on an episode with up to ~90 entries per executor: count is the true count after every step, the stored prefix is
    the fixture's, guard words around all three arrays are intact, and timeline() names the capacity that would have sufficed"""
    tg = TimelineGolden("c1_hash")
    seeds, cap, G = [100, 101], 4, 64
    env = tg.make_env(seeds, pack, "cpu", load_emu(), timeline=False)
    B, E = len(seeds), env.num_executors
    raw_t = torch.full((G + B * E * cap + G,), 12345.5, dtype=torch.float64)
    raw_j = torch.full((G + B * E * cap + G,), 0x5A5A5A5A, dtype=torch.int32)
    raw_c = torch.full((G + B * E + G,), 0x5A5A5A5A, dtype=torch.int32)
    env._timeline = (raw_t[G: G + B * E * cap].view(B, E, cap), raw_j[G: G + B * E * cap].view(B, E, cap), raw_c[G: G + B * E].view(B, E))
    env._bind_timeline()
    env.reset(seed=seeds, options={"time_limit": tg.time_limit})
    env, bad = replay(tg, seeds, pack, "cpu", cap=cap, env=env)
    assert not bad, "\n".join(bad[:10])
    for raw, fill in ((raw_t, 12345.5), (raw_j, 0x5A5A5A5A), (raw_c, 0x5A5A5A5A)):
        assert bool((raw[:G] == fill).all()) and bool((raw[-G:] == fill).all())
    most = int(np.diff(tg.ep(100, "hist_ptr")).max())
    assert int(env.timeline_arrays()[2][0].max()) == most > cap
    with pytest.raises(RuntimeError, match=f"cap={most}"):
        env.timeline(0)
    env.close()


def _everything(env):
    st = env._env_view.clone()
    st[:, HDR_PROF: HDR_PROF + 40] = 0   # shader-clock profiling counters: the only timing-dependent bytes of an env
    return [st, env.nodes.clone(), env.edge_links.clone(), env.dag_ptr.clone(), env.exec_supplies.clone(), env.obs_i32.clone(), env.obs_f64.clone()]


def whole_episode_states(pack, device, lib):
    """one c1 batch through a whole episode (steps, then the fused rollout) three times: nothing ever bound / bound and unbound
    again / bound. Returns the three (arena + every observation buffer)."""
    tg = TimelineGolden("c1_fair")
    out = []
    for mode in ("never", "unbound", "bound"):
        env = tg.make_env([0, 1, 2], pack, device, lib, timeline=False)
        if mode != "never":
            env.enable_timeline(64)
        if mode == "unbound":
            env.disable_timeline()
        env.reset(seed=[0, 1, 2])
        for _ in range(40):
            env.step_async(**env.policy_actions("fair"))
        env.rollout("fair", 600)
        assert int(env.obs_i32[:, 6].sum()) == 3   # all three episodes are over
        out.append(_everything(env))
        env.close()
    return out


def test_state_and_outputs_do_not_depend_on_the_recording(pack):
    never, unbound, bound = whole_episode_states(pack, "cpu", load_emu())
    for other in (unbound, bound):
        for x, y in zip(never, other):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_bind_timeline_names_what_it_refuses(pack):
    env = VecSparkSchedSimEnv(TINY, 2, device="cpu", pack=pack, _lib=load_emu())
    lib = env._b.lib
    t, j, c = torch.zeros(2 * 5 * 8, dtype=torch.float64), torch.zeros(2 * 5 * 8, dtype=torch.int32), torch.ones(10, dtype=torch.int32)
    for args, what in (((None, j.data_ptr(), c.data_ptr(), 8), b"t_dev"), ((t.data_ptr(), None, c.data_ptr(), 8), b"job_dev"),
                       ((t.data_ptr(), j.data_ptr(), None, 8), b"count_dev"), ((t.data_ptr(), j.data_ptr(), c.data_ptr(), 0), b"cap"),
                       ((t.data_ptr(), j.data_ptr(), c.data_ptr(), -3), b"cap")):
        assert lib.sss_bind_timeline(env._h, C.byref(SssTimeline(*args, 0))) != 0 and what in lib.sss_last_error()
    with pytest.raises(ValueError, match="cap"):
        env.enable_timeline(0)
    # nothing bound: rendering is refused, and says why
    rgb = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    assert lib.sss_timeline_render(env._h, C.byref(SssTimelineRenderArgs(None, 1, 4, 4, 0, rgb.data_ptr())), None) != 0 and b"no timeline" in lib.sss_last_error()
    with pytest.raises(RuntimeError, match="enable_timeline"):
        env.render()
    assert lib.sss_bind_timeline(env._h, C.byref(SssTimeline(t.data_ptr(), j.data_ptr(), c.data_ptr(), 8, 0))) == 0
    assert lib.sss_timeline_render(env._h, C.byref(SssTimelineRenderArgs(None, 1, 0, 4, 0, rgb.data_ptr())), None) != 0 and b"width" in lib.sss_last_error()
    assert lib.sss_bind_timeline(env._h, None) == 0   # unbind
    env.close()


def test_abi_of_the_two_entry_points(tmp_path):
    """both symbols are in the emulator library and in EXPORTS, `sss_abi_sizeof` knows both structures and agrees with the ctypes
    mirrors, and every field of a mirror sits where the header compiled with gcc (as a C caller sees it) puts it"""
    import re

    from spark_sched_sim_amd import binding as B
    lib = load_emu()
    for sym in ("sss_bind_timeline", "sss_timeline_render"):
        assert sym in B.EXPORTS and hasattr(lib, sym)
    assert set(B.ABI_PLAIN_STRUCTS) == {"sss_timeline", "sss_timeline_render_args"}
    header = open(osp.join(ROOT, "include", "sss.h")).read()
    assert set(re.findall(r"^struct (sss_[a-z_]+) \{", header, re.M)) - set(B.ABI_TAGGED_STRUCTS) == set(B.ABI_PLAIN_STRUCTS)
    lib.sss_abi_sizeof.argtypes = [C.c_char_p]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{osp.join(ROOT, "include", "sss.h")}"', "int main(void) {"]
    for cname, cls in B.ABI_PLAIN_STRUCTS.items():
        assert lib.sss_abi_sizeof(cname.encode()) == C.sizeof(cls), cname
        lines.append(f'  printf("{cname} %zu\\n", sizeof(struct {cname}));')
        for fname, *_ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof(struct {cname}, {fname}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")], check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in B.ABI_PLAIN_STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, *_ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_recording_kernels_keep_their_register_and_scratch_figures():
    """tests/test_abi.py holds the plain simulator kernels to their scratch / spill / register budget; the recording
    instantiations (`*_tl`: csrc/sss_hip_sim_tl.hip, sss_hip_wide_tl.hip, compiled with machine LICM off like the plain units) are
    held here to the figures they were merged with (profiles/timeline.md section 1), so that a toolchain that brings the spills
    back - the 272 / 640 bytes of scratch per lane spark_sched_sim_amd/build.py describes - fails instead of going unseen"""
    from spark_sched_sim_amd import build

    sys.path.insert(0, osp.join(ROOT, "tools"))
    from isa_counts import kernel_metadata

    md = kernel_metadata(build.build())
    for kernel, scratch_max, spill_max in (("sss_step_kernel_tl", 32, 0), ("sss_step_bounded_kernel_tl", 32, 0), ("sss_rollout_kernel_tl", 64, 6),
                                           ("sss_rollout_heur_kernel_tl", 48, 6), ("sss_reset_kernel_tl", 0, 0),
                                           ("sss_step_kernel_wide_tl", 32, 0), ("sss_step_bounded_kernel_wide_tl", 32, 0), ("sss_rollout_kernel_wide_tl", 80, 11),
                                           ("sss_rollout_heur_kernel_wide_tl", 64, 11), ("sss_reset_kernel_wide_tl", 0, 0)):
        k = md[kernel]
        assert k["private_segment_fixed_size"] <= scratch_max, (kernel, k)
        assert k["vgpr_spill_count"] <= spill_max and k["vgpr_count"] <= 128, (kernel, k)
    rast = [k for k in md if "sss_timeline_render_kernel" in k]
    assert rast and all(md[k]["private_segment_fixed_size"] == 0 and md[k]["vgpr_spill_count"] == 0 and md[k]["vgpr_count"] <= 64 for k in rast)


def test_ex_job_offset_matches_layout(tmp_path):
    """vec_env.HOT_EX_JOB_OFF (what tests/test_gpu_timeline.py reads executor.job_id through) mirrors struct SssHot of both instantiations"""
    from spark_sched_sim_amd.vec_env import HOT_EX_JOB_OFF

    for cap, flag in ((64, []), (128, ["-DSSS_WIDE"])):
        src = tmp_path / f"off{cap}.cpp"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sss_layout.h"\nint main(){ printf("%zu %d\\n", offsetof(SssHot, ex_job), (int)SSS_MAX_EXEC); return 0; }\n')
        exe = tmp_path / f"off{cap}"
        subprocess.run(["g++", *flag, "-I", osp.join(ROOT, "spark_sched_sim_amd", "csrc"), str(src), "-o", str(exe)], check=True)
        off, n = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
        assert (off, n) == (HOT_EX_JOB_OFF[cap], cap)


def render_cases(pack, device, lib):
    """(what, frames from the library, frames from the numpy rasteriser) for the cases of the issue"""
    out = []
    tg = TimelineGolden("c1_fair")
    env = tg.make_env([0, 1, 2], pack, device, lib)
    out.append(("T = 0 right after reset", env.render(width=64, height=20), expected_frames(env, [0, 1, 2], 64, 20)))
    env.rollout("fair", 260)   # mid-episode: open entries of jobs, completed jobs (markers) and running ones
    assert 0 < env.header(0)["n_completed"] < env.header(0)["J"]
    for W, H in ((400, 300), (130, 37), (64, 5)):   # (a width that is no multiple of 64; rh = 1 with rows clipped: 5 rows, 10 executors)
        out.append((f"c1 {W}x{H}", env.render(width=W, height=H), expected_frames(env, [0, 1, 2], W, H)))
    out.append(("env subset", env.render(env_ids=[2, 0], width=97, height=33), expected_frames(env, [2, 0], 97, 33)))
    out.append(("one env", env.render(env_ids=torch.tensor([1]), width=33, height=10), expected_frames(env, [1], 33, 10)))
    env.rollout("fair", 600)   # finished: every job has its marker
    out.append(("c1 finished", env.render(width=200, height=40), expected_frames(env, [0, 1, 2], 200, 40)))
    env.close()
    tg = TimelineGolden("c1_hash")   # an overflowed row: cap 4 where executors collect ~90 entries
    env = tg.make_env([100], pack, device, lib, cap=4)
    env.rollout("hash", 300, HASH_NONE_PERMILLE)
    assert int(env.timeline_arrays()[2].max()) > 4
    out.append(("overflow", env.render(width=256, height=30), expected_frames(env, [0], 256, 30)))
    env.close()
    tg = TimelineGolden("e120_hash")   # the wide instantiation, more executors than pixel rows in the second frame
    env = tg.make_env([0, 1], pack, device, lib)
    env.rollout("hash", 150, HASH_NONE_PERMILLE)
    out.append(("E = 120", env.render(width=160, height=240), expected_frames(env, [0, 1], 160, 240)))
    out.append(("E = 120, 50 rows", env.render(width=70, height=50), expected_frames(env, [0, 1], 70, 50)))
    env.close()
    return out


def test_frames_equal_the_numpy_rasteriser(pack):
    cases = render_cases(pack, "cpu", load_emu())
    for what, got, exp in cases:
        got = got.cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == exp.shape, what
        assert np.array_equal(got, exp), (what, int((got != exp).any(axis=-1).sum()))
    # the cases show what they are meant to: markers, grey, several job colours
    by = {w: e for w, _, e in cases}
    assert (by["c1 finished"] == (255, 0, 0)).all(-1).any() and (by["overflow"] == (128, 128, 128)).all(-1).any()
    assert len(np.unique(by["c1 400x300"].reshape(-1, 3), axis=0)) > 4
    assert len(np.unique(by["T = 0 right after reset"].reshape(-1, 3), axis=0)) == 1


def test_facade_history_and_rgb_array(pack):
    tg = TimelineGolden("c1_fair")
    lib = load_emu()
    with pytest.raises(ValueError, match="rendering is not available"):
        SparkSchedSimEnv(dict(tg.cfg, render_mode="human"), device="cpu", _lib=lib)
    assert SparkSchedSimEnv.metadata["render_modes"] == ["rgb_array"]
    env = SparkSchedSimEnv(dict(tg.cfg, render_mode="rgb_array"), device="cpu", _lib=lib)
    env.reset(seed=0)
    assert [e.id_ for e in env.executors] == list(range(10)) and all(e.history == [[None, -1]] for e in env.executors)
    st, ne = tg.actions(0)
    for i in range(tg.steps(0)):
        _, _, terminated, _, _ = env.step({"stage_idx": int(st[i]), "num_exec": int(ne[i])})
    assert terminated
    assert [e.history for e in env.executors] == tg.history(0)
    frame = env.render()
    assert isinstance(frame, np.ndarray) and frame.shape == (300, 400, 3) and frame.dtype == np.uint8
    assert np.array_equal(frame, expected_frames(env._vec, [0], 400, 300)[0])
    env.close()
    plain = SparkSchedSimEnv(tg.cfg, device="cpu", _lib=lib)   # no render mode: histories are kept all the same, render() gives None
    plain.reset(seed=0)
    assert plain.render() is None and plain.executors[3].history == [[None, -1]]
    # one fetch from the device per step, however many executors are asked
    calls, fetch = [], plain._vec.timeline
    plain._vec.timeline = lambda i: (calls.append(i), fetch(i))[1]
    plain.step({"stage_idx": 0, "num_exec": 1})
    assert [e.history for e in plain.executors] == fetch(0) and [e.history for e in plain.executors] == fetch(0) and calls == [0]
    plain.step({"stage_idx": -1, "num_exec": 1})
    assert plain.executors[0].history == fetch(0)[0] and calls == [0, 0]
    plain.close()
    # opting out: plain kernels, no rows, no histories
    off = SparkSchedSimEnv(tg.cfg, device="cpu", _lib=lib, record_history=False)
    off.reset(seed=0)
    with pytest.raises(RuntimeError, match="no timeline"):
        off.executors[0].history
    off.close()
    with pytest.raises(ValueError, match="record_history"):
        SparkSchedSimEnv(dict(tg.cfg, render_mode="rgb_array"), device="cpu", _lib=lib, record_history=False)


def test_timeline_raises_on_overflow_in_the_facade_shape(pack):
    tg = TimelineGolden("c1_hash")
    env = tg.make_env([100], pack, "cpu", load_emu(), cap=2)
    env.rollout("hash", 200, HASH_NONE_PERMILLE)
    with pytest.raises(RuntimeError, match="overflowed"):
        env.timeline(0)
    env.close()


def sanitized_checks(lib, pack):
    """what the sanitized child process runs: recording on every path in both instantiations, an overflowing capacity, frames"""
    for name, seeds, bounded in (("tiny_fair_tlimit", [0, 1, 2, 3], None), ("stall", [2002], 7), ("e120_hash", [0], None), ("c1_fifo", [6], None)):
        tg = TimelineGolden(name)
        env, bad = replay(tg, seeds, pack, "cpu", lib, bounded=bounded, cap=256 if name != "c1_fifo" else 3)
        assert not bad, bad[:5]
        got, exp = env.render(width=130, height=37).numpy(), expected_frames(env, list(range(len(seeds))), 130, 37)
        assert np.array_equal(got, exp), name
        env.close()
    tg = TimelineGolden("c1_fair")
    env = tg.make_env([0], pack, "cpu", lib)
    env.rollout("fair", 600)
    assert not check_final(tg, env, 0, 0)
    env.close()


def test_recording_and_rendering_under_asan_ubsan():
    """the same kernel source under AddressSanitizer + UBSan (the emulator's sanitized build, in a child process so that the ASan
    runtime can be preloaded)"""
    subprocess.run(["make", "-s", "-C", osp.join(HERE, "emu"), "../_build/libsss_emu_asan.so"], check=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    assert osp.isabs(libasan) and glob.glob(libasan + "*"), "libasan not found: the sanitized run is required, not optional"
    code = textwrap.dedent("""
        import sys, ctypes
        sys.path[:0] = [%r, %r]
        from spark_sched_sim_amd import workload
        import test_emu_timeline as T
        T.sanitized_checks(ctypes.CDLL(%r), workload.default_pack())
        print("SANITIZED-OK")
    """) % (ROOT, HERE, osp.join(HERE, "_build", "libsss_emu_asan.so"))
    preload = os.environ.get("LD_PRELOAD")
    env = dict(os.environ, LD_PRELOAD=libasan + (":" + preload if preload else ""), ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500)
    assert "SANITIZED-OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
