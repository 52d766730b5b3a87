"""The observation writer beyond one pass of its loops, on the CPU wave-emulator build of the kernel source: more than 64
active jobs (a second chunk of jobs), more than 256 stage slots and more than 256 template edges in a chunk (a second iteration
of the node and of the edge pass), every array of every step bit for bit against the C oracle under the counter-based test
policy. The oracle's own sizes are counted first, so that the comparison cannot pass without having crossed those boundaries."""
import pytest

from boundary_util import lockstep_vs_oracle
from emu_util import load_emu
from oracle_binding import OracleEnv
from spark_sched_sim_amd import workload
from spark_sched_sim_amd.digest import splitmix64

# 6 executors under 80 jobs arriving five times as fast as in the C2 sizing: the jobs pile up (80 active jobs, 724 node rows and
# 975 edges at the most over seeds 1 and 2)
CFG = dict(num_executors=6, job_arrival_cap=80, job_arrival_rate=2.0e-4, moving_delay=2000.0, warmup_delay=1000.0)
# the C2 sizing of the benchmark: about 25 active jobs, some of their records in the LDS cache and some in HBM, and steps
# that leave the graph as it was (the edge rows are not written again)
C2 = dict(num_executors=10, job_arrival_cap=50, job_arrival_rate=4.0e-5, moving_delay=2000.0, warmup_delay=1000.0)


def oracle_sizes(pack: bytes, cfg: dict, seed: int, n_steps: int, p_none_permille: int = 30):
    """the oracle alone under the policy of `lockstep_vs_oracle`: (n_jobs, n_nodes, n_edges) of the observation before each step
    taken, and the step at which the reference's own "[step]" stall (error 5) ended the episode (None: it did not)"""
    o = OracleEnv(pack, cfg)
    assert o.reset(seed) == 0
    sizes, stalled_at = [], None
    for t in range(n_steps):
        info = o.info()
        sizes.append((info.n_jobs, info.n_nodes, info.n_edges))
        h = splitmix64((seed << 32) ^ t)
        h2 = splitmix64(h)
        none = info.n_schedulable == 0 or splitmix64(h2) % 1000 < p_none_permille
        e, _, term = o.step(-1 if none else h % info.n_schedulable, 1 + h2 % max(1, info.num_committable_execs))
        if e == 5:
            stalled_at = t
        assert e in (0, 5), (seed, t, e)
        if e or term:
            break
    o.close()
    return sizes, stalled_at


def steps_past_every_boundary(sizes) -> int:
    return sum(1 for nj, nn, ne in sizes if nj > 64 and nn > 256 and ne > 256)


N_STEPS = 300


@pytest.mark.parametrize("seed", [1, 2])
def test_many_jobs_nodes_and_edges_match_the_oracle_on_the_emulator(seed):
    pack = workload.default_pack()
    sizes, stalled_at = oracle_sizes(pack, CFG, seed, N_STEPS)
    assert stalled_at is None and len(sizes) == N_STEPS
    assert steps_past_every_boundary(sizes) >= 200, steps_past_every_boundary(sizes)
    bad = lockstep_vs_oracle(pack, CFG, [seed], N_STEPS, device="cpu", lib=load_emu())
    assert not bad, "\n".join(bad[:8])


def test_c2_sizing_matches_the_oracle_on_the_emulator():
    bad = lockstep_vs_oracle(workload.default_pack(), C2, [1, 2, 3], 400, device="cpu", lib=load_emu())
    assert not bad, "\n".join(bad[:8])
