"""-m gpu: the observation writer beyond one pass of its loops on the HIP path (tests/test_emu_observation_rows.py has the shape
and the counting of what it covers): more than 64 active jobs, more than 256 node rows and more than 256 edges, and the C2
sizing of the benchmark, every array of every step bit for bit against the C oracle."""
import pytest

from boundary_util import lockstep_vs_oracle
from spark_sched_sim_amd import workload
from test_emu_observation_rows import C2, CFG, oracle_sizes, steps_past_every_boundary

pytestmark = pytest.mark.gpu


def test_many_jobs_nodes_and_edges_match_the_oracle():
    pack = workload.default_pack()
    seeds = list(range(1, 33))
    early_stalls = 0
    for s in seeds:
        sizes, stalled_at = oracle_sizes(pack, CFG, s, 300)
        early_stalls += stalled_at is not None and stalled_at < 100
        if s in (1, 2):
            assert stalled_at is None and len(sizes) == 300, (s, stalled_at, len(sizes))
            assert steps_past_every_boundary(sizes) >= 200, (s, steps_past_every_boundary(sizes))
    assert early_stalls <= len(seeds) // 4, early_stalls
    bad = lockstep_vs_oracle(pack, CFG, seeds, 300, device="cuda:0")
    assert not bad, "\n".join(bad[:8])


def test_c2_sizing_matches_the_oracle():
    bad = lockstep_vs_oracle(workload.default_pack(), C2, list(range(1, 9)), 400, device="cuda:0")
    assert not bad, "\n".join(bad[:8])
