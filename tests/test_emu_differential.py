"""Differential (average-reward) returns on the device, without a GPU: include/sss.h sss_reward_window_update /
sss_differential_returns through the emulator library (the per-row / per-env functions of csrc/sss_returns.h in plain loops)
against the reference's recorded numbers and against training.DifferentialReturns - bit for bit, there is no tolerance: nothing in
the chain may round differently."""
import ctypes as C
import glob
import os
import os.path as osp
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from differential_util import bits, check_random_records, check_reference_fixture, fixture_rollouts
from emu_util import load_emu

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(HERE)


def _binding():
    from spark_sched_sim_amd.binding import Binding

    return Binding(load_emu())


def test_reference_fixture_is_reproduced_exactly():
    check_reference_fixture(_binding(), "cpu")


def test_host_class_reproduces_the_reference_fixture():
    """(what the device form is compared with elsewhere is itself exact on the reference's numbers)"""
    from spark_sched_sim_amd.training import DifferentialReturns

    ro, d, lens = fixture_rollouts("cpu")
    diff = DifferentialReturns(700)
    for call in range(2):
        out = diff(ro)
        assert bits(diff.avg_num_jobs) == bits(d[f"diff_avg_num_jobs{call}"])
        for b, n in enumerate(lens):
            assert np.array_equal(bits(out[:n, b]), bits(d[f"diffret{call}_r{b}"]))


def test_random_records_match_the_host_class_bit_for_bit():
    check_random_records(_binding(), "cpu")


def test_ordered_sum_is_numpys_axis_sum():
    """the window's sums are 0.0 + row[0] + ... + row[cap - 1] in row order - what numpy's axis-0 sum of the (cap, 2) array gives -
    at window sizes around and far above numpy's pairwise-summation block"""
    from spark_sched_sim_amd.binding import SssRewardWindowArgs

    b = _binding()
    rng = np.random.default_rng(5)
    for cap in (1, 7, 129, 700, 8193, 50_000):
        win = np.stack([rng.random(cap) * 5e4, -rng.random(cap) * 1e4], 1)
        w = torch.from_numpy(np.stack([win, np.zeros_like(win)]))
        sums = torch.full((2,), 7.0, dtype=torch.float64)
        # (T == 0: the window stays where it is and is summed)
        a = SssRewardWindowArgs(0, 4, None, None, None, None, cap, (C.c_void_p * 2)(w[0].data_ptr(), w[1].data_ptr()), 0, 0, None, sums.data_ptr())
        b.check(b.lib.sss_reward_window_update(C.byref(a), 0))
        assert np.array_equal(bits(sums), bits(win.sum(0))), cap
        assert np.array_equal(w[0].numpy(), win) and not w[1].any()
        seq = [0.0, 0.0]
        for row in win:
            seq = [seq[0] + row[0], seq[1] + row[1]]
        assert np.array_equal(bits(sums), bits(np.array(seq))), cap


def test_entry_points_reject_bad_arguments():
    from spark_sched_sim_amd.binding import SssDiffretArgs, SssRewardWindowArgs, reward_window_scratch

    b = _binding()
    T, B, cap = 5, 3, 4
    act = torch.ones((T, B), dtype=torch.uint8)
    x = torch.zeros((T, B), dtype=torch.float64)
    w = torch.zeros((2, cap, 2), dtype=torch.float64)
    sums, avg, out = torch.zeros(2, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), torch.zeros((T, B), dtype=torch.float64)
    scratch = torch.zeros(reward_window_scratch(T, B), dtype=torch.int64)

    def window(**kw):
        f = dict(T=T, B=B, active_dev=act.data_ptr(), t_before_dev=x.data_ptr(), t_after_dev=x.data_ptr(), rewards_dev=x.data_ptr(), cap=cap,
                 window_dev=(C.c_void_p * 2)(w[0].data_ptr(), w[1].data_ptr()), current=0, pad_=0, scratch_dev=scratch.data_ptr(), sums_dev=sums.data_ptr())
        f.update(kw)
        return SssRewardWindowArgs(**f)

    def diffret(**kw):
        f = dict(T=T, B=B, active_dev=act.data_ptr(), t_before_dev=x.data_ptr(), t_after_dev=x.data_ptr(), rewards_dev=x.data_ptr(), sums_dev=sums.data_ptr(),
                 out_dev=out.data_ptr(), avg_dev=avg.data_ptr())
        f.update(kw)
        return SssDiffretArgs(**f)

    lib = b.lib
    assert lib.sss_reward_window_update(C.byref(window()), 0) == 0 and lib.sss_differential_returns(C.byref(diffret()), 0) == 0
    for args, code, msg in ((None, -1, "NULL argument"), (window(sums_dev=None), -1, "NULL argument"), (window(active_dev=None), -1, "NULL argument"),
                            (window(scratch_dev=None), -1, "NULL argument"), (window(window_dev=(C.c_void_p * 2)(w[0].data_ptr(), None)), -1, "NULL argument"),
                            (window(T=-1), -39, "sss_reward_window_update: negative size"), (window(B=-2), -39, "sss_reward_window_update: negative size"),
                            (window(cap=0), -39, "sss_reward_window_update: cap must be >= 1"), (window(cap=-5), -39, "cap must be >= 1"),
                            (window(current=2), -39, "current must be 0 or 1"),
                            (window(window_dev=(C.c_void_p * 2)(w[0].data_ptr(), w[0].data_ptr())), -39, "the two window buffers must differ"),
                            (window(window_dev=(C.c_void_p * 2)(w[0].data_ptr(), w[1].data_ptr() + 8)), -39, "the window buffers must be 16-byte aligned")):
        assert lib.sss_reward_window_update(C.byref(args) if args is not None else None, 0) == code, msg
        assert msg in lib.sss_last_error().decode()
        with pytest.raises(ValueError, match=re.escape(msg)):
            b.check(code)
    for args, code, msg in ((None, -1, "NULL argument"), (diffret(sums_dev=None), -1, "NULL argument"), (diffret(out_dev=None), -1, "NULL argument"),
                            (diffret(rewards_dev=None), -1, "NULL argument"), (diffret(T=-1), -39, "sss_differential_returns: negative size"),
                            (diffret(B=-1), -39, "sss_differential_returns: negative size")):
        assert lib.sss_differential_returns(C.byref(args) if args is not None else None, 0) == code, msg
        assert msg in lib.sss_last_error().decode()


def test_empty_record_leaves_the_window_and_still_writes_the_sums():
    from spark_sched_sim_amd.binding import SssDiffretArgs, SssRewardWindowArgs

    b = _binding()
    cap = 6
    w = torch.zeros((2, cap, 2), dtype=torch.float64)
    w[1] = torch.arange(12, dtype=torch.float64).reshape(6, 2) + 1.0
    w[1, :, 1] *= -1.0
    keep = w.clone()
    for T, B in ((0, 5), (5, 0), (0, 0)):
        sums, avg = torch.zeros(2, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
        a = SssRewardWindowArgs(T, B, None, None, None, None, cap, (C.c_void_p * 2)(w[0].data_ptr(), w[1].data_ptr()), 1, 0, None, sums.data_ptr())
        b.check(b.lib.sss_reward_window_update(C.byref(a), 0))
        assert torch.equal(w, keep)
        assert np.array_equal(bits(sums), bits(keep[1].numpy().sum(0)))
        d = SssDiffretArgs(T, B, None, None, None, None, sums.data_ptr(), None, avg.data_ptr())
        b.check(b.lib.sss_differential_returns(C.byref(d), 0))
        assert bits(avg)[0] == bits(-sums[1].item() / sums[0].item())


def test_abi_of_the_two_entry_points(tmp_path):
    """both symbols are in the emulator library and in EXPORTS, `sss_abi_sizeof` knows both structures and agrees with the ctypes
    mirrors, and every field of a mirror sits where the header compiled with gcc puts it"""
    from spark_sched_sim_amd import binding as B

    lib = load_emu()
    for sym in ("sss_reward_window_update", "sss_differential_returns"):
        assert sym in B.EXPORTS and hasattr(lib, sym)
    assert set(B.ABI_TAGGED_STRUCTS) == {"sss_reward_window_args", "sss_diffret_args"} and not set(B.ABI_TAGGED_STRUCTS) & set(B.ABI_STRUCTS)
    header = open(osp.join(ROOT, "include", "sss.h")).read()
    assert set(re.findall(r"^typedef struct (sss_[a-z_]+) \1;", header, re.M)) - {"sss_handle"} == set(B.ABI_TAGGED_STRUCTS)  # (sss_handle: opaque)
    lib.sss_abi_sizeof.argtypes = [C.c_char_p]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{osp.join(ROOT, "include", "sss.h")}"', "int main(void) {"]
    for cname, cls in B.ABI_TAGGED_STRUCTS.items():
        assert lib.sss_abi_sizeof(cname.encode()) == C.sizeof(cls), cname
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, *_ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append(f'  printf("scratch %d\\n", (int)SSS_REWARD_WINDOW_SCRATCH(130, 7));')
    lines += ["  return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")], check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in B.ABI_TAGGED_STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, *_ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert int(got["scratch"]) == B.reward_window_scratch(130, 7) == 4 * 7 + 1

    class Stale(C.Structure):  # a mirror one field short is refused when the library is loaded
        _fields_ = B.SssDiffretArgs._fields_[:-1]

    keep = B.ABI_TAGGED_STRUCTS["sss_diffret_args"]
    B.ABI_TAGGED_STRUCTS["sss_diffret_args"] = Stale
    try:
        with pytest.raises(RuntimeError, match="binding / library mismatch"):
            B.Binding(lib)
    finally:
        B.ABI_TAGGED_STRUCTS["sss_diffret_args"] = keep


def test_ppo_picks_the_host_class_without_a_gpu_and_the_device_class_needs_kernels():
    from spark_sched_sim_amd.training import PPO, DeviceDifferentialReturns, DifferentialReturns

    cfg = dict(num_sequences=1, num_rollouts=4, reward_buff_cap=700)
    ppo = PPO(torch.nn.Linear(2, 2), cfg)
    assert type(ppo.diff) is DifferentialReturns and ppo.beta is None
    ro, _, _ = fixture_rollouts("cpu")
    out = ppo.returns(ro)  # a record on the CPU: the host form stays
    assert type(ppo.diff) is DifferentialReturns and np.array_equal(bits(out), bits(DifferentialReturns(700)(ro)))
    with pytest.raises(RuntimeError, match="no binding"):  # a missing kernel is an error, not a quiet host path
        DeviceDifferentialReturns(700)(ro)
    with pytest.raises(ValueError, match="reward_buff_cap"):
        DeviceDifferentialReturns(0)


def test_window_update_under_asan_ubsan():
    """the window kernels' source under AddressSanitizer + UBSan (the emulator's sanitized build, in a child process so that the
    ASan runtime can be preloaded): the reference fixture and the random records, overflow and cap = 1 included"""
    subprocess.run(["make", "-s", "-C", osp.join(HERE, "emu"), "../_build/libsss_emu_asan.so"], check=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not osp.isabs(libasan) or not glob.glob(libasan + "*"):
        pytest.skip("libasan not found")
    code = textwrap.dedent("""
        import sys, ctypes
        sys.path[:0] = [%r, %r]
        from differential_util import check_random_records, check_reference_fixture
        from spark_sched_sim_amd.binding import Binding
        b = Binding(ctypes.CDLL(%r))
        check_reference_fixture(b, "cpu")
        check_random_records(b, "cpu")
        print("SANITIZED-OK")
    """) % (ROOT, HERE, osp.join(HERE, "_build", "libsss_emu_asan.so"))
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900)
    assert "SANITIZED-OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]
