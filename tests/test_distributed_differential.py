"""Differential returns across ranks, on CPU: two gloo ranks hold different records; between the window update and the returns one
all-reduce adds up the ranks' (total time, reward sum), so that both use the same avg_num_jobs = -sum(rew) / sum(time) over both
ranks' windows - for the device form (emulator library) and for the host class alike. Ranks are fresh child processes."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
CAP, CALLS = 400, 3


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _records(rank: int):
    """the rank's records, call after call (different on the two ranks; the third one overflows the window)"""
    from differential_util import random_record

    gen = torch.Generator().manual_seed(100 + rank)
    return [random_record(gen, T, B) for T, B in (((40, 5), (70, 3), (120, 6)) if rank == 0 else ((55, 4), (30, 9), (90, 7)))]


def _worker(rank: int, world: int, port: int, out_dir: str):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    from differential_util import make_rollouts
    from emu_util import load_emu
    from spark_sched_sim_amd.binding import Binding
    from spark_sched_sim_amd.training import DeviceDifferentialReturns, DifferentialReturns

    devc, host = DeviceDifferentialReturns(CAP, binding=Binding(load_emu())), DifferentialReturns(CAP)
    res = []
    for rec in _records(rank):
        ro = make_rollouts(*rec)
        out_d = devc(ro)
        out_h = host(ro)
        res.append({"dev_out": out_d, "host_out": out_h, "dev_avg": devc.avg_num_jobs, "host_avg": float(host.avg_num_jobs), "dev_window": devc.data.copy(),
                    "host_window": host.data.copy()})
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_pool_their_window_sums(tmp_path):
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    from differential_util import bits, make_rollouts
    from emu_util import load_emu
    from spark_sched_sim_amd.training import DifferentialReturns

    load_emu()  # build once, before the ranks start
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ranks = [torch.load(str(tmp_path / f"r{r}.pt"), weights_only=False) for r in range(2)]
    # by hand: each rank's window as a single process keeps it (the window does not depend on the pooling), then the pooled estimate
    alone = [DifferentialReturns(CAP) for _ in range(2)]
    separate = []
    for call in range(CALLS):
        sums = []
        for r in range(2):
            alone[r](make_rollouts(*_records(r)[call]))
            sums.append(alone[r].data.sum(0))
        separate.append([float(a.avg_num_jobs) for a in alone])
        total_time, rew_sum = sums[0][0] + sums[1][0], sums[0][1] + sums[1][1]
        avg = float(-rew_sum / total_time)
        for r in range(2):
            got = ranks[r][call]
            assert np.array_equal(bits(got["dev_window"]), bits(alone[r].data)) and np.array_equal(bits(got["host_window"]), bits(alone[r].data))
            assert bits(got["dev_avg"]) == bits(avg) and bits(got["host_avg"]) == bits(avg), (call, r, got["dev_avg"], got["host_avg"], avg)
            # the single-process formula with that avg (training.DifferentialReturns' loop)
            a, tb, ta, rw = _records(r)[call]
            dt = ta - tb
            R = torch.zeros(a.shape[1], dtype=torch.float64)
            want = torch.zeros_like(rw)
            for k in range(a.shape[0] - 1, -1, -1):
                R = torch.where(a[k], -(-rw[k] - dt[k] * avg) + R, R)
                want[k] = R
            want = want * a
            assert np.array_equal(bits(got["dev_out"]), bits(want)) and np.array_equal(bits(got["host_out"]), bits(want)), (call, r)
    # ... and the ranks' own estimates do differ: without the pooling each would have used another avg_num_jobs
    assert all(s[0] != s[1] for s in separate)
    assert all(ranks[0][c]["dev_avg"] == ranks[1][c]["dev_avg"] != separate[c][0] for c in range(CALLS))
