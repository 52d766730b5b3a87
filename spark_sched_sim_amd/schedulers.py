"""Scheduler plugin surface, mirroring the reference's `schedulers/` package for the heuristics
(reference schedulers/scheduler.py:10-18, schedulers/heuristics/{round_robin,random_scheduler,utils}.py).

A plugin written for the reference - anything with `.schedule(obs) -> (action_dict, info_dict)` -
runs unchanged against `SparkSchedSimEnv` (env.py) or `VecSparkSchedSimEnv.obs_view(i)`: those
produce the reference's observation dict. The classes below are this repo's own implementations
of the reference's two heuristic plugins on that dict (host side, one env at a time), plus the Decima paper's two stronger
baselines, weighted fair and SJF-CP (defined here on the observation dict); their batched on-device counterparts are
`VecSparkSchedSimEnv.policy_actions("fair" | "fifo" | "hash" | "wfair" | "sjfcp")`.
"""
from __future__ import annotations

import math
from abc import ABC, abstractmethod
from typing import Any

import numpy as np


class Scheduler(ABC):
    """Interface for all schedulers (reference schedulers/scheduler.py:10-18)"""

    name: str
    env_wrapper_cls: Any | None

    @abstractmethod
    def schedule(self, obs: dict) -> tuple[dict, dict]:
        ...


def preprocess_obs(obs: dict[str, Any]) -> None:
    """adds `frontier_stages` (nodes without an incoming edge in the active subgraph) and
    `schedulable_stages` (node index -> position among schedulable nodes) to the observation;
    same keys as the reference helper (schedulers/heuristics/utils.py:5-14)."""
    nodes = obs["dag_batch"].nodes
    has_parent = np.zeros(nodes.shape[0], dtype=bool)
    has_parent[obs["dag_batch"].edge_links[:, 1]] = True
    sched_nodes = np.flatnonzero(nodes[:, 2] != 0)
    obs["frontier_stages"] = set(np.flatnonzero(~has_parent).tolist())
    obs["schedulable_stages"] = {int(n): i for i, n in enumerate(sched_nodes)}


def find_stage(obs: dict[str, Any], job_idx: int) -> int:
    """first schedulable frontier stage of the job, else its first schedulable stage, else -1
    (reference schedulers/heuristics/utils.py:17-37)"""
    lo, hi = obs["dag_ptr"][job_idx], obs["dag_ptr"][job_idx + 1]
    fallback = -1
    for node in range(lo, hi):
        i = obs["schedulable_stages"].get(node)
        if i is None:
            continue
        if node in obs["frontier_stages"]:
            return i
        if fallback == -1:
            fallback = i
    return fallback


class RoundRobinScheduler(Scheduler):
    """Spark's fair ("Fair", dynamic_partition=True) / FIFO scheduler as in the reference
    (schedulers/heuristics/round_robin.py:7-49)"""

    def __init__(self, num_executors: int, dynamic_partition: bool = True):
        self.name = "Fair" if dynamic_partition else "FIFO"
        self.num_executors = num_executors
        self.dynamic_partition = dynamic_partition
        self.env_wrapper_cls = None

    def schedule(self, obs: dict) -> tuple[dict, dict]:
        preprocess_obs(obs)
        n_jobs = len(obs["exec_supplies"])
        cap = int(np.ceil(self.num_executors / max(1, n_jobs))) if self.dynamic_partition else self.num_executors
        committable = obs["num_committable_execs"]
        src = obs["source_job_idx"]
        # the job that is releasing executors goes first
        if src < n_jobs:
            idx = find_stage(obs, src)
            if idx != -1:
                return {"stage_idx": idx, "num_exec": committable}, {}
        # then jobs in arrival order that are below their share
        for j in range(n_jobs):
            if j == src or obs["exec_supplies"][j] >= cap:
                continue
            idx = find_stage(obs, j)
            if idx != -1:
                return {"stage_idx": idx, "num_exec": min(committable, cap - obs["exec_supplies"][j])}, {}
        return {"stage_idx": -1, "num_exec": committable}, {}


def node_work(obs: dict[str, Any]) -> np.ndarray:
    """work(n) = f64(nodes[n, 0]) * f64(nodes[n, 1]): remaining tasks times the most recent task duration, the reference's
    Stage.approx_remaining_work (components/stage.py:50-51) as the observation shows it. One exact f64 product of two f32
    values, so any implementation gets the same bits."""
    nodes = obs["dag_batch"].nodes
    return nodes[:, 0].astype(np.float64) * nodes[:, 1].astype(np.float64)


def job_work(obs: dict[str, Any], work: np.ndarray | None = None) -> list[float]:
    """W_j: the work of job j's active nodes dag_ptr[j] .. dag_ptr[j+1]-1, schedulable or not, summed in f64 from 0.0 left to
    right in node order. f64 addition is not associative; fixing the order (the node rows' order, i.e. ascending stage id
    within the job) is what lets the on-device policies reproduce these sums bit for bit."""
    if work is None:
        work = node_work(obs)
    ptr = obs["dag_ptr"]
    out = []
    for j in range(len(obs["exec_supplies"])):
        w = 0.0
        for n in range(int(ptr[j]), int(ptr[j + 1])):
            w += float(work[n])
        out.append(w)
    return out


class WeightedFairScheduler(Scheduler):
    """Weighted fair, the Decima paper's tuned fair baseline (Mao et al., SIGCOMM 2019, 7.2): each job's executor share is
    in proportion to its work^alpha. On-device counterpart: `VecSparkSchedSimEnv.policy_actions("wfair", alpha)`, which must
    match this plugin bit for bit, so every float operation below is spelled out in a fixed order:

    - weight: x = max(W_j, 1.0), p = x multiplied by x another |alpha| - 1 times; w_j = 1.0 (alpha = 0), p (alpha > 0) or
      1.0 / p (alpha < 0). Repeated multiplication, not pow: host and device pow differ in the last ulp.
    - S = sum of w_j over the active jobs, f64, left to right in active order.
    - cap_j = min(E, max(1, ceil((f64(E) * w_j) / S))).
    - decision: RoundRobinScheduler's, with cap_j in place of the common cap: the source job first (find_stage, every
      committable executor); else the first job in active order, not the source, with exec_supplies[j] < cap_j and a stage
      from find_stage, which gets min(committable, cap_j - exec_supplies[j]); else stage_idx = -1.

    alpha = 0 gives every job weight 1, S = A exactly and ceil(E / A): RoundRobinScheduler(dynamic_partition=True)."""

    def __init__(self, num_executors: int, alpha: int = -1):
        if int(alpha) != alpha or not -4 <= int(alpha) <= 4:
            raise ValueError(f"WeightedFairScheduler: alpha must be an integer in [-4, 4], got {alpha}")
        self.name = f"WeightedFair(alpha={int(alpha)})"
        self.num_executors = num_executors
        self.alpha = int(alpha)
        self.env_wrapper_cls = None

    def weight(self, W: float) -> float:
        if self.alpha == 0:
            return 1.0
        x = W if W > 1.0 else 1.0
        p = x
        for _ in range(abs(self.alpha) - 1):
            p *= x
        return p if self.alpha > 0 else 1.0 / p

    def caps(self, obs: dict) -> list[int]:
        w = [self.weight(W) for W in job_work(obs)]
        S = 0.0
        for x in w:
            S += x
        E = self.num_executors
        return [min(E, max(1, math.ceil((float(E) * x) / S))) for x in w]

    def schedule(self, obs: dict) -> tuple[dict, dict]:
        preprocess_obs(obs)
        n_jobs = len(obs["exec_supplies"])
        caps = self.caps(obs)
        committable = obs["num_committable_execs"]
        src = obs["source_job_idx"]
        if src < n_jobs:
            idx = find_stage(obs, src)
            if idx != -1:
                return {"stage_idx": idx, "num_exec": committable}, {}
        for j in range(n_jobs):
            if j == src or obs["exec_supplies"][j] >= caps[j]:
                continue
            idx = find_stage(obs, j)
            if idx != -1:
                return {"stage_idx": idx, "num_exec": min(committable, caps[j] - obs["exec_supplies"][j])}, {}
        return {"stage_idx": -1, "num_exec": committable}, {}


class SJFCPScheduler(Scheduler):
    """Shortest job first with critical-path stage choice (SJF-CP, Mao et al., SIGCOMM 2019, 7.2). On-device counterpart:
    `VecSparkSchedSimEnv.policy_actions("sjfcp")`, bit for bit.

    - job: j* = argmin W_j (job_work) over the jobs with at least one schedulable node; ties go to the earliest position.
    - critical path inside j*, over the active subgraph (the observation's edge_links): CP(n) = work(n) + max(CP(c) for the
      children c of n), or work(n) without children. One add to an exact max, so any evaluation order that reaches the
      fixed point gives the same bits.
    - stage: the schedulable node of j* with the largest CP, the lowest node index on ties; stage_idx is its rank among all
      schedulable nodes. num_exec = every committable executor; there is no source-job rule.
    - no job with a schedulable node: stage_idx = -1."""

    name = "SJF-CP"
    env_wrapper_cls = None

    def __init__(self, num_executors: int | None = None):
        self.num_executors = num_executors

    def schedule(self, obs: dict) -> tuple[dict, dict]:
        preprocess_obs(obs)
        nodes = obs["dag_batch"].nodes
        ptr = obs["dag_ptr"]
        committable = obs["num_committable_execs"]
        work = node_work(obs)
        W = job_work(obs, work)
        best = -1
        for j in range(len(W)):
            if np.any(nodes[int(ptr[j]):int(ptr[j + 1]), 2] != 0) and (best < 0 or W[j] < W[best]):
                best = j
        if best < 0:
            return {"stage_idx": -1, "num_exec": committable}, {}
        lo, hi = int(ptr[best]), int(ptr[best + 1])
        children: dict[int, list[int]] = {n: [] for n in range(lo, hi)}
        for u, v in np.asarray(obs["dag_batch"].edge_links).reshape(-1, 2).tolist():
            if lo <= u < hi:
                children[u].append(v)
        cp: dict[int, float] = {}

        def crit(n: int) -> float:
            if n not in cp:
                kids = children[n]
                cp[n] = float(work[n]) + max(crit(c) for c in kids) if kids else float(work[n])
            return cp[n]

        pick = -1
        for n in range(lo, hi):
            if nodes[n, 2] != 0 and (pick < 0 or crit(n) > crit(pick)):
                pick = n
        return {"stage_idx": obs["schedulable_stages"][pick], "num_exec": committable}, {}


class RandomScheduler(Scheduler):
    """The reference's random heuristic (schedulers/heuristics/random_scheduler.py:7-32): jobs are
    tried in a random order until one has a stage to offer, then a random executor count.

    What is pinned by tests/golden/c1_random.npz is the stream, not the text: the draws come from a
    legacy MT19937 `numpy.random.RandomState(seed)`; each job pick is one `choice` over the jobs not
    yet rejected in this call (in active order), and the executor count is one `randint` over
    [1, num_committable_execs] made after the job search, whether or not a stage was found."""

    name = "Random"
    env_wrapper_cls = None

    def __init__(self, seed: int = 42):
        self.set_seed(seed)

    def set_seed(self, seed: int) -> None:
        self.np_random = np.random.RandomState(seed)

    def _pick_stage(self, obs: dict) -> int:
        remaining = list(range(len(obs["exec_supplies"])))
        while remaining:
            job = self.np_random.choice(remaining)
            found = find_stage(obs, job)
            if found != -1:
                return found
            remaining.remove(job)
        return -1

    def schedule(self, obs: dict) -> tuple[dict, dict]:
        preprocess_obs(obs)
        stage = self._pick_stage(obs)
        count = self.np_random.randint(1, obs["num_committable_execs"] + 1)
        return {"stage_idx": stage, "num_exec": count}, {}


def make_scheduler(agent_cfg: dict) -> Scheduler:
    """by-name factory like the reference's (schedulers/__init__.py:17-21)"""
    cfg = dict(agent_cfg)
    cls = cfg.pop("agent_cls")
    table = {"RoundRobinScheduler": RoundRobinScheduler, "RandomScheduler": RandomScheduler,
             "WeightedFairScheduler": WeightedFairScheduler, "SJFCPScheduler": SJFCPScheduler}
    if cls == "DecimaScheduler":  # needs torch.nn; imported on demand like the reference's optional agents
        from .decima import DecimaScheduler
        table["DecimaScheduler"] = DecimaScheduler
    assert cls in table, f"'{cls}' is not a valid scheduler."
    return table[cls](**cfg)
