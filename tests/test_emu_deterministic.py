"""The deterministic mode's row operation (include/sss.h SSS_ROWS_ORDERED_ADD, csrc/sss_rows.h) through the emulator library's
host implementation and its AddressSanitizer build, and the sort plans the autograd functions build for it"""
import glob
import os
import subprocess
import sys
import textwrap

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_ordered_add_matches_an_in_order_host_sum():
    from deterministic_util import check_ordered_add, check_rejected_ops

    from emu_util import load_emu
    from spark_sched_sim_amd.binding import Binding

    b = Binding(load_emu())
    check_ordered_add(b, "cpu", n=6000)
    check_rejected_ops(b, "cpu")


def test_sort_plans_are_sorted_and_stable():
    from deterministic_util import check_plans

    check_plans("cpu")


def test_ordered_add_under_asan_ubsan():
    """the element statement reads no key past the end of idx, no row outside a / b / perm"""
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu"), "../_build/libsss_emu_asan.so"], check=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not glob.glob(libasan + "*"):
        pytest.skip("libasan not found")
    code = textwrap.dedent("""
        import sys, ctypes
        sys.path[:0] = [%r, %r]
        from deterministic_util import check_ordered_add
        from spark_sched_sim_amd.binding import Binding
        check_ordered_add(Binding(ctypes.CDLL(%r)), "cpu", n=6000)
        print("SANITIZED-OK")
    """) % (os.path.dirname(HERE), HERE, os.path.join(HERE, "_build", "libsss_emu_asan.so"))
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900)
    assert "SANITIZED-OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-4000:]


def test_deterministic_scope_restores_the_callers_settings():
    import torch
    import torch.utils.deterministic as tud

    from spark_sched_sim_amd.train_kernels import deterministic_enabled
    from spark_sched_sim_amd.training import deterministic_scope

    state = lambda: (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(), tud.fill_uninitialized_memory)  # noqa: E731
    before = state()
    assert not deterministic_enabled()
    try:
        for caller in ((False, False), (True, True)):
            torch.use_deterministic_algorithms(caller[0], warn_only=caller[1])
            outer = state()
            with deterministic_scope():
                assert state() == (True, False, False) and deterministic_enabled()
            assert state() == outer
            with pytest.raises(RuntimeError):
                with deterministic_scope(fill_uninitialized_memory=True):
                    assert state() == (True, False, True)
                    raise RuntimeError("escapes")
            assert state() == outer
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert deterministic_enabled()  # (warn-only counts; read at every call)
        torch.use_deterministic_algorithms(False)
        assert not deterministic_enabled()
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
        tud.fill_uninitialized_memory = before[2]


def test_trainer_refuses_combinations_that_are_not_reproducible(tmp_path):
    from decima_util import AGENT
    from training_util import reference_smoke_test_config

    from spark_sched_sim_amd.training import Trainer, make_trainer

    cfg = reference_smoke_test_config(str(tmp_path))
    for extra in (dict(rollout_duration=1.0e5), dict(collector_groups=2)):
        with pytest.raises(ValueError, match="deterministic"):
            make_trainer({**cfg, "trainer": {**cfg["trainer"], "deterministic": True, **extra}}, device="cpu")
        with pytest.raises(ValueError, match="deterministic"):
            Trainer(dict(AGENT, agent_cls="DecimaScheduler"), cfg["env"], {**cfg["trainer"], **extra}, device="cpu", deterministic=True)
