"""The host plugins WeightedFairScheduler / SJFCPScheduler (spark_sched_sim_amd/schedulers.py) on the reference's observation dict:
they reproduce the action streams recorded when they drove the reference env (tests/golden/make_heuristic_golden.py), weighted
fair with alpha = 0 is the reference's fair scheduler, and the edge cases of the definitions hold."""
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLDEN_DIR, Golden
from spark_sched_sim_amd.schedulers import (RoundRobinScheduler, SJFCPScheduler, WeightedFairScheduler, job_work, make_scheduler,
                                            node_work)
from spark_sched_sim_amd.spaces import GraphInstance

HEURISTIC_SETS = ["c1_wfair_m1", "c1_wfair_p1", "c1_sjfcp", "c3_wfair_m1", "c3_sjfcp", "e100_wfair_m1", "e100_sjfcp", "deep_c1_sjfcp",
                  "tiny_wfair_p2_tlimit"]


def make_obs(nodes, edges, ptr, sup, ncommit, src):
    nodes = np.asarray(nodes, dtype=np.float32).reshape(-1, 3)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return {"dag_batch": GraphInstance(nodes, np.zeros(len(edges), dtype=np.int64), edges), "dag_ptr": list(ptr),
            "num_committable_execs": int(ncommit), "source_job_idx": int(src), "exec_supplies": list(sup)}


def recorded_obs(g: Golden, s: int):
    """(step, observation) for the observations a fixture stores in full; the action taken on it is entry step + 1"""
    for i in range(int(g.ep(s, "n_full"))):
        yield i, make_obs(g.ep(s, f"full{i}_nodes"), g.ep(s, f"full{i}_edges"), g.ep(s, f"full{i}_ptr"), g.ep(s, f"full{i}_sup"),
                          g.ep(s, "ncommit")[i], g.ep(s, "src_idx")[i])


def plugin_for(g: Golden):
    E = g.cfg["num_executors"]
    if g.policy == "wfair":
        return WeightedFairScheduler(E, alpha=int(g.z["param"]))
    assert g.policy == "sjfcp"
    return SJFCPScheduler(E)


@pytest.mark.parametrize("name", HEURISTIC_SETS)
def test_host_plugin_reproduces_recorded_actions(name):
    g = Golden(name)
    sched = plugin_for(g)
    n = 0
    for s in g.seeds:
        for i, obs in recorded_obs(g, s):
            if i + 1 >= len(g.ep(s, "stage_idx")):
                break
            act, _ = sched.schedule(obs)
            assert (int(act["stage_idx"]), int(act["num_exec"])) == (int(g.ep(s, "stage_idx")[i + 1]), int(g.ep(s, "num_exec")[i + 1])), (s, i)
            n += 1
    assert n > 0


@pytest.mark.parametrize("name", ["c1_fair", "c3_fair", "e100_fair", "testyaml_fair"])
def test_wfair_alpha_zero_is_round_robin(name):
    g = Golden(name)
    E = g.cfg["num_executors"]
    wf, rr = WeightedFairScheduler(E, alpha=0), RoundRobinScheduler(E)
    for s in g.seeds:
        for i, obs in recorded_obs(g, s):
            if i + 1 >= len(g.ep(s, "stage_idx")):
                break
            a, _ = wf.schedule(dict(obs))
            b, _ = rr.schedule(dict(obs))
            assert a == b, (s, i)
            assert (a["stage_idx"], a["num_exec"]) == (int(g.ep(s, "stage_idx")[i + 1]), int(g.ep(s, "num_exec")[i + 1])), (s, i)


def test_make_scheduler_builds_the_new_plugins():
    a = make_scheduler({"agent_cls": "WeightedFairScheduler", "num_executors": 10, "alpha": -1})
    b = make_scheduler({"agent_cls": "SJFCPScheduler", "num_executors": 10})
    assert isinstance(a, WeightedFairScheduler) and a.alpha == -1 and a.num_executors == 10
    assert isinstance(b, SJFCPScheduler)


@pytest.mark.parametrize("alpha", [5, -5, 100, 0.5])
def test_wfair_rejects_alpha_out_of_range(alpha):
    with pytest.raises(ValueError, match="alpha"):
        WeightedFairScheduler(10, alpha=alpha)


def test_work_is_one_f64_product_summed_left_to_right():
    # 0.1f and 3 * 0.1f: the products are exact in f64; the sum's order decides the last bit
    vals = [(1.0, 0.1), (3.0, 0.1), (7.0, 1e8), (1.0, 0.3)]
    obs = make_obs([(r, d, 1.0) for r, d in vals], [], [0, 4], [0], 1, 1)
    w = node_work(obs)
    assert all(w[k] == np.float64(np.float32(r)) * np.float64(np.float32(d)) for k, (r, d) in enumerate(vals))
    expect = 0.0
    for x in w.tolist():
        expect += x
    assert job_work(obs) == [expect]


def test_no_jobs():
    obs = make_obs(np.zeros((0, 3)), [], [0], [], 4, 0)
    assert WeightedFairScheduler(5, -2).schedule(obs)[0] == {"stage_idx": -1, "num_exec": 4}
    assert SJFCPScheduler(5).schedule(make_obs(np.zeros((0, 3)), [], [0], [], 4, 0))[0] == {"stage_idx": -1, "num_exec": 4}


def test_zero_work_jobs_weigh_like_work_one():
    # W = 0 (no task has run yet: duration 0) and W = 1 both give x = 1, so equal caps ceil(E / 2) for every alpha
    obs = make_obs([(5, 0.0, 1), (1, 1.0, 1)], [], [0, 1, 2], [0, 0], 10, 2)
    for alpha in range(-4, 5):
        assert WeightedFairScheduler(10, alpha).caps(dict(obs)) == [5, 5]
    # SJF-CP: W = 0 is the shortest job
    assert SJFCPScheduler(10).schedule(dict(obs))[0] == {"stage_idx": 0, "num_exec": 10}


def test_wfair_caps_follow_work():
    # W = (1, 9): alpha = 1 gives shares 1/10 and 9/10, alpha = -1 the reverse; the cap is at least 1
    obs = make_obs([(1, 1.0, 1), (9, 1.0, 1)], [], [0, 1, 2], [0, 0], 10, 2)
    assert WeightedFairScheduler(10, 1).caps(dict(obs)) == [1, 9]
    assert WeightedFairScheduler(10, -1).caps(dict(obs)) == [9, 1]
    assert WeightedFairScheduler(10, 2).caps(dict(obs)) == [1, 10]  # ceil(10 * 81 / 82)
    # a single job gets every executor whatever alpha is
    one = make_obs([(3, 2.0, 1)], [], [0, 1], [0], 10, 1)
    for alpha in range(-4, 5):
        assert WeightedFairScheduler(10, alpha).caps(dict(one)) == [10]
        assert WeightedFairScheduler(10, alpha).schedule(dict(one))[0] == {"stage_idx": 0, "num_exec": 10}


def test_wfair_source_job_first_then_capped_jobs():
    # job 0 has 2 executors, cap 1 (alpha = 1, W = (1, 9)) -> skipped; job 1 gets min(ncommit, 9 - 0)
    obs = make_obs([(1, 1.0, 1), (9, 1.0, 1)], [], [0, 1, 2], [2, 0], 4, 2)
    assert WeightedFairScheduler(10, 1).schedule(dict(obs))[0] == {"stage_idx": 1, "num_exec": 4}
    # the source job (index 0) takes every committable executor regardless of its cap
    src = make_obs([(1, 1.0, 1), (9, 1.0, 1)], [], [0, 1, 2], [2, 0], 4, 0)
    assert WeightedFairScheduler(10, 1).schedule(dict(src))[0] == {"stage_idx": 0, "num_exec": 4}


def test_sjfcp_picks_critical_path_head_and_breaks_ties_low():
    # one job, nodes 0..3: 0 -> 2, 1 -> 3; work 0 = 1, 1 = 2, 2 = 5, 3 = 4: CP(0) = 6, CP(1) = 6 (tie -> node 0)
    nodes = [(1, 1.0, 1), (2, 1.0, 1), (5, 1.0, 0), (4, 1.0, 0)]
    obs = make_obs(nodes, [(0, 2), (1, 3)], [0, 4], [0], 3, 1)
    assert SJFCPScheduler(5).schedule(dict(obs))[0] == {"stage_idx": 0, "num_exec": 3}
    # make node 3 heavier: CP(1) = 7 wins
    nodes[3] = (5, 1.0, 0)
    obs = make_obs(nodes, [(0, 2), (1, 3)], [0, 4], [0], 3, 1)
    assert SJFCPScheduler(5).schedule(dict(obs))[0] == {"stage_idx": 1, "num_exec": 3}


def test_sjfcp_shortest_schedulable_job_ties_to_earliest():
    # job 0: W = 2 but nothing schedulable; jobs 1 and 2: W = 4 each (tie -> job 1); stage_idx ranks among schedulable nodes
    nodes = [(2, 1.0, 0), (4, 1.0, 1), (2, 2.0, 1), (0, 1.0, 1)]
    obs = make_obs(nodes, [], [0, 1, 2, 4], [0, 0, 0], 2, 3)
    # schedulable nodes in order: 1, 2, 3 -> job 1's node 1 has rank 0
    assert SJFCPScheduler(5).schedule(dict(obs))[0] == {"stage_idx": 0, "num_exec": 2}
    # none schedulable
    obs = make_obs([(2, 1.0, 0)], [], [0, 1], [0], 2, 1)
    assert SJFCPScheduler(5).schedule(dict(obs))[0] == {"stage_idx": -1, "num_exec": 2}


def test_fixtures_regenerate_from_the_live_reference(tmp_path):
    """the committed fixtures come out of tests/golden/make_heuristic_golden.py array for array (where the reference and its
    gymnasium stand-in are available; skipped elsewhere, like tests/test_oracle_vs_live_reference.py's sources)"""
    here = osp.join(GOLDEN_DIR, "make_heuristic_golden.py")
    probe = subprocess.run([sys.executable, "-c", "import make_golden, os.path as p, sys; sys.exit(0 if p.isdir(p.join(make_golden.REF, 'spark_sched_sim')) else 3)"],
                           cwd=GOLDEN_DIR, capture_output=True)
    if probe.returncode != 0 or not osp.isdir(osp.join(osp.dirname(GOLDEN_DIR), "refharness")):
        pytest.skip("the reference env is not available here")
    names = ["c1_wfair_p1", "tiny_wfair_p2_tlimit", "e100_sjfcp"]
    subprocess.run([sys.executable, here, "--out", str(tmp_path)] + names, check=True, capture_output=True)
    for name in names:
        a, b = np.load(osp.join(GOLDEN_DIR, f"{name}.npz")), np.load(tmp_path / f"{name}.npz")
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (name, k)
