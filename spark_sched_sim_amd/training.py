"""Rollout collection and PPO over the batched env.

The reference trains with one OS process per env: a `RolloutWorker` loop per process
(reference trainers/rollout_worker.py:118-206), a Pipe gather, then returns / baselines / the CLIP
loss on the learner (trainers/trainer.py:171-216, trainers/utils/returns_calculator.py:45-76,
trainers/utils/baselines.py:12-37, trainers/ppo.py:51-138). Here every "worker" is one env of a
`VecSparkSchedSimEnv`, all envs advance together on the GPU, the recorded observations stay on the
device as one compact graph (`decima.compact_graph`), and the per-rollout post-processing is a set
of padded tensor ops. The arithmetic per element follows the reference's; tolerances are in the tests.

Layout of a `Rollouts` record (T = longest rollout of the batch, B = envs): every per-step quantity
is a [T, B] tensor and `active[t, b]` says whether env b recorded a step at position t (a rollout's
steps are always a prefix). Observation (t, b) is observation id t*B + b of `graph`.
"""
from __future__ import annotations

import contextlib
import ctypes
from dataclasses import dataclass, field
from typing import Any, Callable, Sequence

import numpy as np
import torch

from .binding import ERROR_NAMES, SssCollectArgs, device_of
from .decima import concat_graphs, select_observations
from .wrappers import VecStochasticTimeLimit

SKIP_ENV = -(2 ** 31)  # include/sss.h SSS_SKIP_ENV
EPS = 1e-8             # trainers/ppo.py:12


@dataclass
class Rollouts:
    graph: dict[str, Any]
    active: torch.Tensor        # bool[T,B]
    t_before: torch.Tensor      # f64[T,B]  wall time (sync) / elapsed time (async) when the action was taken
    t_after: torch.Tensor       # f64[T,B]  the same clock after the step
    rewards: torch.Tensor       # f64[T,B]
    stage_sel: torch.Tensor     # i64[T,B]
    job_idx: torch.Tensor       # i64[T,B]
    exec_sel: torch.Tensor      # i64[T,B]
    lgprobs: torch.Tensor       # f32[T,B]
    resets: torch.Tensor        # bool[T,B] (async: the env was reset right after this step)
    stats: dict[str, np.ndarray] = field(default_factory=dict)
    obs_index: torch.Tensor | None = None  # i64[T,B]: which observation of `graph` belongs to (t, b); None: t * B + b

    @property
    def lengths(self) -> torch.Tensor:
        return self.active.sum(0)

    def rollout(self, b: int) -> dict[str, np.ndarray]:
        """env b's record in the shape of the reference's `RolloutBuffer` (rollout_worker.py:18-45)"""
        n = int(self.active[:, b].sum())
        tb, ta = self.t_before[:n, b].cpu().numpy(), self.t_after[:n, b].cpu().numpy()
        return {"wall_times": np.concatenate([tb, ta[-1:]]) if n else np.zeros(1),
                "rewards": self.rewards[:n, b].cpu().numpy(),
                "actions": torch.stack([self.stage_sel[:n, b], self.job_idx[:n, b], self.exec_sel[:n, b]], 1).cpu().numpy(),
                "lgprobs": self.lgprobs[:n, b].cpu().numpy(),
                "resets": self.resets[:n, b].nonzero(as_tuple=True)[0].cpu().numpy()}

    def sample_ids(self) -> torch.Tensor:
        """observation ids of all recorded steps in the reference's order (rollout-major:
        `chain(*obsns_list)`, ppo.py:58-62)"""
        T, B = self.active.shape
        ids = self.obs_index if self.obs_index is not None else (
            torch.arange(T, device=self.active.device)[:, None] * B + torch.arange(B, device=self.active.device)[None, :])
        return ids.t()[self.active.t()]

    def flat(self, x: torch.Tensor) -> torch.Tensor:
        """a [T,B] quantity as the flat per-sample vector matching `sample_ids`"""
        return x.t()[self.active.t()]


ActFn = Callable[[dict[str, Any], torch.Tensor], dict[str, torch.Tensor]]


class GraphArena:
    """The record of a collection's observations as ONE compact graph (what `concat_graphs` of the per-step graphs gives), built
    on the device while collecting: `append` copies the step's graph out of the env's capacity buffers (`decima_graph_on_device`)
    behind what is there, at cursors that stay on the device, shifting its ids to arena ids (include/sss.h sss_arena_append).
    The host never learns a step's sizes; it keeps `headroom` steps' worth of the env's capacities free beyond the last cursor
    it has seen (`ensure`), growing the arrays geometrically when that is not the case."""

    NODES, EDGES, JOBS, OBS = 0, 1, 2, 3
    # (name, dtype, elements per row, what it has one row per, what its ids name: 0 nothing, 1 nodes, 2 jobs, 3 observations)
    ARRAYS = (("x", torch.float32, 5, 0, 0), ("node_obs", torch.int64, 1, 0, 3), ("node_loc", torch.int64, 1, 0, 0), ("node_job", torch.int64, 1, 0, 2),
              ("gen", torch.int32, 1, 0, 0), ("stage_mask", torch.bool, 1, 0, 0), ("sched_rank", torch.int64, 1, 0, 0), ("node_recv", torch.int32, 1, 0, 0),
              ("src", torch.int64, 1, 1, 1), ("dst", torch.int64, 1, 1, 1), ("edge_obs", torch.int64, 1, 1, 3), ("edge_layers", torch.int32, 1, 1, 0),
              ("job_obs", torch.int64, 1, 2, 3), ("job_cap", torch.int64, 1, 2, 0), ("job_first", torch.int64, 1, 2, 1),
              ("obs_nodes", torch.int64, 1, 3, 0), ("obs_jobs", torch.int64, 1, 3, 0), ("obs_depth", torch.int32, 1, 3, 0))

    def __init__(self, env, capacity: Sequence[int] | None = None):
        self.env, self.dev, self.B = env, env.device, env.num_envs
        d = env.dims
        self.step_max = (self.B * d.node_cap, self.B * d.edge_cap, self.B * d.job_cap, self.B)  # what one step can add at most
        self.capacity = [max(int(c), 16 * m) for c, m in zip(capacity or (0, 0, 0, 0), self.step_max)]
        self.capacity[3] = max(self.capacity[3], 1024 * self.B)
        self.cursor = torch.zeros(8, dtype=torch.int64, device=self.dev)
        self.seen = [0, 0, 0, 0]   # the last cursors the host has seen
        self.seen_steps = 0        # ... and how many steps they cover
        self.steps = 0             # steps appended (enqueued)
        self.buf = {name: torch.empty((self.capacity[kind], per) if per > 1 else (self.capacity[kind],), dtype=dt, device=self.dev)
                    for name, dt, per, kind, _ in self.ARRAYS}
        self._args = None

    def _build_args(self, g):
        from .binding import SssArenaArgs, SssArenaArray
        a = SssArenaArgs()
        a.n_arrays, a.n_obs = len(self.ARRAYS), self.B
        a.totals_dev, a.cursor_dev = g["totals_dev"].data_ptr(), self.cursor.data_ptr()
        for k in range(4):
            a.capacity[k] = self.capacity[k]
        a.rows_hint = 0
        for i, (name, dt, per, kind, shift) in enumerate(self.ARRAYS):
            src = g[name]
            assert src.dtype == dt and src.is_contiguous(), name
            a.arrays[i] = SssArenaArray(src.data_ptr(), self.buf[name].data_ptr(), src.element_size(), per, kind, shift)
        self._args = (a, tuple(g[name].data_ptr() for name, *_ in self.ARRAYS) + (g["totals_dev"].data_ptr(),))

    def note(self, cursors: Sequence[int], steps: int) -> None:
        """the host has seen the cursors as they were after `steps` appended steps"""
        self.seen, self.seen_steps = [int(c) for c in cursors[:4]], int(steps)

    def ensure(self, sync) -> None:
        """room for the next step whatever its size: the steps the host has not seen the cursors of may each have added a
        step's maximum. Grows (after `sync()`, which must leave `note` up to date) when that bound does not fit."""
        def short():
            ahead = self.steps - self.seen_steps + 1
            return [k for k in range(4) if self.seen[k] + ahead * self.step_max[k] > self.capacity[k]]
        if not short():
            return
        sync()
        for k in short():
            # (x 1.3, not x 2: at BASELINE config 5 the record is ~21 GB per rank and a doubled arena can hold twice that during a first
            # collection; a growth step is one device copy of the arrays of that kind, ~10 ms)
            new_cap = max(int(1.3 * self.capacity[k]), self.seen[k] + 8 * self.step_max[k])
            for name, dt, per, kind, _ in self.ARRAYS:
                if kind == k:
                    old = self.buf[name]
                    self.buf[name] = torch.empty((new_cap, *old.shape[1:]), dtype=dt, device=self.dev)
                    self.buf[name][: self.seen[k]] = old[: self.seen[k]]
            self.capacity[k] = new_cap
        self._args = None

    def append(self, g: dict[str, Any], rows_hint: int = 0) -> None:
        key = tuple(g[name].data_ptr() for name, *_ in self.ARRAYS) + (g["totals_dev"].data_ptr(),)
        if self._args is None or self._args[1] != key:
            self._build_args(g)
        a = self._args[0]
        a.rows_hint = int(rows_hint)
        with device_of(self.dev):
            self.env._b.check(self.env._b.lib.sss_arena_append(ctypes.byref(a), self.env._stream()))
        self.steps += 1

    def finish(self, n_steps: int, sizes: Sequence[int] | None = None) -> dict[str, Any]:
        """the graph of the first `n_steps` steps: `sizes` = the cursors (nodes, edges, jobs) as they were after that many steps
        (`note`), default: everything appended - the steps behind them are dropped"""
        cur = [int(c) for c in self.cursor[:6].tolist()]
        if cur[5]:
            raise RuntimeError("the graph arena overflowed (the headroom rule of GraphArena.ensure was violated)")
        if sizes is None:
            sizes = cur[:3]
        assert all(0 <= int(s) <= c for s, c in zip(sizes[:3], cur[:3])) and n_steps <= cur[4]
        sizes = (int(sizes[0]), int(sizes[1]), int(sizes[2]), n_steps * self.B)
        out: dict[str, Any] = {name: self.buf[name][: sizes[kind]] for name, _, _, kind, _ in self.ARRAYS}
        out["gen"] = out["gen"].long()
        out["n_obs"], out["n_pad"] = n_steps * self.B, self.env.dims.node_cap
        out["_by_observation"] = True  # (appended step by step, env by env: decima.select_observations cuts such a record by ranges)
        return out


class _Collection:
    """What one collection keeps between its steps: the envs' state (who takes part, their clocks, who failed), the record -
    [T_cap, B] arrays that grow geometrically, row t written by step t's `sss_collect_step` phase 1 together with row t of the
    [T_cap, 8] flags - and what the host has learnt of the steps so far."""

    SPEC = (("active", torch.uint8), ("t_before", torch.float64), ("t_after", torch.float64), ("rewards", torch.float64), ("stage_sel", torch.int64),
            ("job_idx", torch.int64), ("exec_sel", torch.int64), ("lgprobs", torch.float32), ("resets", torch.uint8))  # (the order of sss_collect_args' rec_*)

    def __init__(self, asynchronous: bool, duration: float, wall: torch.Tensor, cap: int = 1024):
        B, dev = wall.shape[0], wall.device
        self.asynchronous, self.duration, self.wall = asynchronous, duration, wall
        self.elapsed = torch.zeros(B, dtype=torch.float64, device=dev)
        self.active = torch.ones(B, dtype=torch.uint8, device=dev)  # (bool view for the graph kernel and the caller's policy)
        self.pending = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.cap = cap
        self.rows = {name: torch.zeros((cap, B), dtype=dt, device=dev) for name, dt in self.SPEC}
        self.flags = torch.zeros((cap, 8), dtype=torch.int32, device=dev)
        self.alive = B > 0   # somebody takes part in the next step
        self.n_kept = 0      # steps that are part of the record
        self.n_lockstep = 0  # steps a loop that reads every step's flags before issuing the next would have issued (a dropped last step included)
        self.n_failed = 0

    def grow(self) -> None:
        for name, a in self.rows.items():
            self.rows[name] = torch.cat([a, torch.zeros_like(a)])
        self.flags = torch.cat([self.flags, torch.zeros_like(self.flags)])
        self.cap *= 2

    def row_pointers(self, t: int) -> tuple[int, ...]:
        """the tail of `sss_collect_args` for step t: the record's arrays, then the step's flags"""
        return (*(a.data_ptr() for a in self.rows.values()), self.flags[t].data_ptr())

    def fields(self) -> dict[str, torch.Tensor]:
        """the kept rows as `Rollouts` fields"""
        out = {name: a[: self.n_kept] for name, a in self.rows.items()}
        out["active"], out["resets"] = out["active"].view(torch.bool), out["resets"].view(torch.bool)
        return out


class RolloutCollector:
    """the reference's `RolloutWorkerSync` / `RolloutWorkerAsync` loops for all envs at once.

    Env b plays worker rank b: seed of its k-th episode = base_seeds[b] + seed_step * k
    (rollout_worker.py:118-120, trainer.py:264-269), time limit from `StochasticTimeLimit`'s rule.
    `act_fn(g, step_counts)` (g = compact graph of the active envs' observations) returns
    `DecimaPolicy.act`'s dict; the default samples from `policy`. `step_counts` is an int64 tensor ON THE ENV'S DEVICE (the
    collection kernels update it in place): an `act_fn` that mixes it with CPU tensors has to move it (`.cpu()` is one sync
    per step). Envs that are done (sync) or have filled their duration (async) are frozen with
    SSS_SKIP_ENV until the others catch up."""

    def __init__(self, env, mean_time_limit: float, base_seeds: Sequence[int], seed_step: int, num_executors: int,
                 policy=None, act_fn: ActFn | None = None, generator: torch.Generator | None = None, on_env_error: str = "raise",
                 record_on_device: bool = True):
        """record_on_device: synchronous collection with the default policy sampling keeps the host out of the loop - the step's
        graph stays in the env's capacity buffers with its sizes on the device, `GraphArena` appends it to the record there, and
        the flags of a step are read a few steps late (the steps enqueued in between find every env frozen when the collection
        turns out to be over). The record is the same; False reads the sizes and the flags every step (two waits per step).
        on_env_error: what to do when an env reports an error from `step` - in practice the
        reference's `[step]` assertion (spark_sched_sim.py:212-215), which valid Decima actions can
        trigger (tests/golden/stall_case.json). "raise" = the reference's behaviour (the worker
        aborts, the trainer stops, rollout_worker.py:110-112 / trainer.py:117-124); "truncate" = the
        rollout ends before the failing step and training goes on (`env_errors` counts them).
        (All envs take their steps together on one stream. Alternating groups of envs on streams of their own were measured
        slower on one MI355X - 1.84 ms per row of the record with two groups against 0.88 ms, profiles/r03_ppo.md - and removed.)"""
        assert on_env_error in ("raise", "truncate")
        self.record_on_device = bool(record_on_device)
        self._arena_sizes = None  # the previous collection's graph sizes: the next arena's starting capacity
        self.on_env_error = on_env_error
        self.env_errors = 0
        self.env = env
        self.tl_env = VecStochasticTimeLimit(env, mean_time_limit)
        self.base_seeds = np.asarray(base_seeds, dtype=np.int64)
        assert self.base_seeds.shape == (env.num_envs,)
        self.seed_step = int(seed_step)
        self.reset_count = np.zeros(env.num_envs, dtype=np.int64)
        self.step_counts = torch.zeros(env.num_envs, dtype=torch.long, device=env.device)
        self.E = num_executors
        self.policy = policy
        self.generator = generator
        if policy is not None:
            policy.bind_kernels(env._b)  # inference on the fused GNN kernels; training stays on autograd
        self.act_fn = act_fn
        self._in_episodes = False  # the envs are inside their episodes (async: the next collection goes on from there)
        self._wall = None
        self._pending_reset = None

    @property
    def seeds(self) -> np.ndarray:
        return self.base_seeds + self.seed_step * self.reset_count

    def _reset(self, mask: torch.Tensor | None = None) -> None:
        self.tl_env.reset(seed=[int(s) for s in self.seeds], mask=mask)
        self.reset_count += 1 if mask is None else mask.cpu().numpy().astype(np.int64)

    def _stats(self) -> dict[str, np.ndarray]:
        """rollout_worker.py:122-130 for every env"""
        return {k: v.cpu().numpy() for k, v in self.env.rollout_stats().items()}

    def _issue(self, col: _Collection, t: int, stage_idx: torch.Tensor, num_exec: torch.Tensor, arena: GraphArena | None = None) -> dict[str, Any]:
        """Enqueues step t: the compact graph of the active envs' observations (recorded: returned, or appended to `arena` with
        its sizes left on the device), the policy's sample, `sss_collect_step` phase 0 (the env's actions, into `stage_idx` /
        `num_exec`), `sss_step`, `sss_collect_step` phase 1 (time limit, who failed / finished / goes on, row t of the record
        and of the flags, the envs' clocks). Waits for nothing but what the graph and the policy wait for."""
        env, dev = self.env, self.env.device
        if t == col.cap:
            col.grow()
        act_b = col.active.view(torch.bool)
        g = env.decima_graph(act_b) if arena is None else env.decima_graph_on_device(act_b)
        a = self.act_fn(g, self.step_counts) if self.act_fn is not None else self.policy.act(g, self.generator)
        if arena is not None:
            hint = g["totals_hint"].tolist()
            arena.append(g, rows_hint=max(5 * hint[0], hint[1], hint[2], env.num_envs) if hint[0] >= 0 else 0)
        sel = [a[n] if a[n].dtype == torch.int64 and a[n].is_contiguous() else a[n].to(torch.int64).contiguous() for n in ("stage_sel", "job_idx", "exec_sel")]
        lg = a["lgprob"] if a["lgprob"].dtype == torch.float32 and a["lgprob"].is_contiguous() else a["lgprob"].float().contiguous()
        c = SssCollectArgs(env.num_envs, int(col.asynchronous), t, float(col.duration), env.obs_f64.data_ptr(), env.obs_i32.data_ptr(), env.obs_i32.stride(0),
                           self.tl_env.time_limit.data_ptr(), col.active.data_ptr(), col.wall.data_ptr(), col.elapsed.data_ptr(), self.step_counts.data_ptr(),
                           col.pending.data_ptr(), sel[0].data_ptr(), sel[1].data_ptr(), sel[2].data_ptr(), lg.data_ptr(), stage_idx.data_ptr(), num_exec.data_ptr(),
                           *col.row_pointers(t))
        stream = env._stream()
        with device_of(dev):
            env._b.check(env._b.lib.sss_collect_step(ctypes.byref(c), 0, stream))
        env.step_async(stage_idx, num_exec)
        with device_of(dev):
            env._b.check(env._b.lib.sss_collect_step(ctypes.byref(c), 1, stream))
        return g

    def _outcome(self, col: _Collection, t: int, flags: Sequence[int], stage_idx: torch.Tensor, num_exec: torch.Tensor) -> None:
        """what became of step t, from the first five of its flags (the step has finished): an env's error raises or truncates,
        the step is counted as kept unless it failed for every env left, async resets, whether anybody is left (`col.alive`)"""
        any_bad, any_done, any_left, bad_env, any_recorded = flags
        col.n_lockstep = t + 1
        if any_bad:
            n_bad = int(col.pending.sum()) - col.n_failed
            col.n_failed += n_bad
            self.env_errors += n_bad
            if self.on_env_error == "raise":
                b = bad_env - 1
                code = int(self.env.obs_i32[b, 7])
                err = RuntimeError(f"env {b} (seed {int(self.seeds[b] - self.seed_step)}), rollout step {t}: "
                                   f"{ERROR_NAMES.get(code, code)}; action stage_idx={int(stage_idx[b])} num_exec={int(num_exec[b])}")
                # what a bug report needs: the env's seed, time limit and action history
                err.case = {"seed": int(self.seeds[b] - self.seed_step), "time_limit": float(self.tl_env.time_limit[b]), "code": code,
                            "stage_idx": [int(x) for x in col.rows["stage_sel"][:t, b]] + [int(stage_idx[b])],
                            "num_exec": [int(x) + 1 for x in col.rows["exec_sel"][:t, b]] + [int(num_exec[b])]}
                raise err
            # truncate: the failing step is not recorded and the env sits out the rest of this
            # collection (async: it starts its next episode at the next collection)
            if not any_recorded:
                col.alive = False
                return
        col.n_kept = t + 1
        if col.asynchronous and any_done:
            self._reset(mask=col.rows["resets"][t].view(torch.bool))
        col.alive = bool(any_left)

    def _collect_waiting(self, col: _Collection) -> dict[str, Any]:
        """The loop that waits: the graph's sizes and the flags are read after every step (two device->host reads per step),
        the kept steps' graphs are concatenated at the end."""
        B, dev = self.env.num_envs, self.env.device
        acts = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        graphs = []
        t = 0
        while col.alive:
            g = self._issue(col, t, *acts)
            self._outcome(col, t, col.flags[t, :5].tolist(), *acts)
            if col.n_kept == t + 1:
                graphs.append(g)
            t += 1
        return concat_graphs(graphs)

    def _collect_ahead(self, col: _Collection) -> dict[str, Any]:
        """The loop that runs ahead (see __init__, record_on_device): the graphs go to a `GraphArena` on the device, what the
        host wants of a step - its flags and the arena's cursors after it - lands in pinned rings of R slots, and the host looks
        at a step when it has finished or when LAG steps have been enqueued behind it (one pinned-ring read per step)."""
        env, dev, B = self.env, self.env.device, self.env.num_envs
        LAG, R = 4, 8
        cuda = dev.type == "cuda"
        pin = (lambda x: x.pin_memory()) if cuda else (lambda x: x)
        cap0 = None
        if self._arena_sizes:
            d = env.dims
            step_max = (B * d.node_cap, B * d.edge_cap, B * d.job_cap, B)
            cap0 = [int(1.1 * c) + (LAG + 4) * m for c, m in zip(self._arena_sizes, step_max)]
        arena = GraphArena(env, cap0)
        ring_flags, ring_cur = pin(torch.zeros((R, 8), dtype=torch.int32)), pin(torch.zeros((R, 8), dtype=torch.int64))
        ring_acts = [(torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)) for _ in range(R)]
        ring_ev = [torch.cuda.Event() for _ in range(R)] if cuda else None
        calls0 = getattr(self.policy, "_calls", 0)
        late: list[int] = []  # steps enqueued whose flags have not been looked at, oldest first

        def take_late() -> None:
            """the oldest enqueued step's flags (waits for that step if it has not finished)"""
            t = late.pop(0)
            if ring_ev is not None:
                ring_ev[t % R].synchronize()
            cursors = ring_cur[t % R].tolist()  # (ring_cur[.., 4] = steps appended: which step the cursors are of)
            self._outcome(col, t, ring_flags[t % R, :5].tolist(), *ring_acts[t % R])
            if col.n_kept == t + 1:  # (a last step that failed for every env left is dropped: the arena's record ends before it)
                arena.note(cursors, t + 1)

        def drain_all() -> None:
            while late and col.alive:
                take_late()

        t = 0
        while col.alive:
            # look at the steps that have finished, and never run more than LAG steps ahead of the flags
            while late and col.alive and (len(late) >= LAG or ring_ev is None or ring_ev[late[0] % R].query()):
                take_late()
            if col.alive:
                arena.ensure(drain_all)
                self._issue(col, t, *ring_acts[t % R], arena=arena)
                ring_flags[t % R].copy_(col.flags[t], non_blocking=True)
                ring_cur[t % R].copy_(arena.cursor, non_blocking=True)
                if ring_ev is not None:
                    ring_ev[t % R].record(torch.cuda.current_stream(dev))
                late.append(t)
                t += 1
                if ring_ev is None:
                    take_late()
        if cuda:
            torch.cuda.current_stream(dev).synchronize()
        graph = arena.finish(col.n_kept, arena.seen)  # (the steps enqueued behind the last kept one are dropped)
        # the steps enqueued behind the last one found every env frozen, but each took a draw counter of the policy's sampling
        # stream (decima._sample_kernels): hand them back, so that the next collection draws what it would have drawn - the loop
        # that waits for every step's flags has issued n_lockstep steps (a last step that failed for every env left took its
        # counter too, although it is not part of the record)
        if hasattr(self.policy, "_calls"):
            self.policy._calls = calls0 + col.n_lockstep
        self._arena_sizes = [int(graph["x"].shape[0]), int(graph["src"].numel()), int(graph["job_obs"].numel()), col.n_kept * B]
        return graph

    def _loop(self, asynchronous: bool, duration: float, with_stats: bool) -> Rollouts:
        """Both worker loops: the collection's set-up (sync: every env starts an episode; async: the envs go on where the last
        collection left them, those that failed in it start a new episode), one of the two drivers, the record as `Rollouts`."""
        env, dev, B = self.env, self.env.device, self.env.num_envs
        if not asynchronous or not self._in_episodes:
            self._reset()
            self._in_episodes = True
            self._wall = torch.zeros(B, dtype=torch.float64, device=dev)
        wall = self._wall
        if asynchronous and self._pending_reset is not None:
            self._reset(mask=self._pending_reset)
            wall = torch.where(self._pending_reset, torch.zeros_like(wall), wall)
        self._pending_reset = None
        col = _Collection(asynchronous, duration, wall.clone())
        # the loop without waits (see __init__, record_on_device)
        fast = (self.record_on_device and not asynchronous and self.act_fn is None and self.policy is not None and B > 0
                and self.policy._use_kernels() and env.graph_kernel_fits)
        graph = self._collect_ahead(col) if fast else self._collect_waiting(col)
        if col.n_failed:
            self._pending_reset = col.pending.view(torch.bool)
        self._wall = col.wall
        return Rollouts(graph=graph, stats=self._stats() if with_stats else {}, **col.fields())

    def collect_sync(self, with_stats: bool = True) -> Rollouts:
        """one full episode per env (rollout_worker.py:133-159)"""
        return self._loop(False, 0.0, with_stats)

    def collect_async(self, rollout_duration: float, with_stats: bool = True) -> Rollouts:
        """`rollout_duration` ms of simulated time per env, episodes restarting in place
        (rollout_worker.py:162-206)"""
        return self._loop(True, float(rollout_duration), with_stats)


# ---- returns (trainers/utils/returns_calculator.py) -----------------------------------------------

def _record_kernels(ro: Rollouts, binding=None):
    """the binding to run the [T, B] record kernels with (include/sss.h sss_discounted_returns / sss_sequence_baselines): the
    library when the record is on a GPU - no fallback there - or the one a caller passes (tests: the emulator's host backend)"""
    if binding is not None:
        return binding
    if ro.active.is_cuda:
        from .train_kernels import _binding
        return _binding()
    return None


def _dist_world() -> int:
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _c64(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous() if t.dtype == torch.float64 else t.double().contiguous()


def discounted_returns(ro: Rollouts, beta: float, binding=None) -> torch.Tensor:
    """R_k = r_k + exp(-beta * 1e-3 * dt_k) * R_{k+1} per rollout (returns_calculator.py:67-76); f64[T,B]"""
    T, B = ro.active.shape
    b = _record_kernels(ro, binding)
    if b is not None and T > 0 and B > 0:  # one kernel, a thread per env (the loop below: T x 5 launches, 0.30 s at BASELINE config 5)
        from .binding import SssReturnsArgs
        dev = ro.active.device
        act, tb, ta, rw = ro.active.contiguous().view(torch.uint8), _c64(ro.t_before), _c64(ro.t_after), _c64(ro.rewards)
        out = torch.empty((T, B), dtype=torch.float64, device=dev)
        a = SssReturnsArgs(T, B, act.data_ptr(), tb.data_ptr(), ta.data_ptr(), rw.data_ptr(), float(beta), out.data_ptr())
        with device_of(dev):
            b.check(b.lib.sss_discounted_returns(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0))
        return out
    dt = ro.t_after - ro.t_before
    out = torch.zeros_like(ro.rewards)
    R = torch.zeros(B, dtype=torch.float64, device=ro.rewards.device)
    for k in range(T - 1, -1, -1):
        R = torch.where(ro.active[k], ro.rewards[k] + torch.exp(-beta * 1e-3 * dt[k]) * R, R)
        out[k] = R
    return out * ro.active


def _pool_window_sums(sums: torch.Tensor) -> torch.Tensor:
    """several ranks: the ranks' (total time, reward sum) added up, in place - every rank then uses the same
    avg_num_jobs = -sum(rew) / sum(time) over all ranks' windows (the reference's one learner keeps ONE window over every worker's
    rows; here each rank keeps `cap` rows of its own envs and the estimate is pooled: DESIGN section 7). One process: untouched."""
    import torch.distributed as dist
    if _dist_world() > 1:
        dist.all_reduce(sums)
    return sums


class DifferentialReturns:
    """average-reward ("differential") returns with the moving estimate of the mean number of
    concurrent jobs kept in a circular buffer of (dt, reward) rows (returns_calculator.py:6-65, 78-89).
    The host form: the rows go to the host and the window is a numpy array (`DeviceDifferentialReturns`: the kernels)"""

    def __init__(self, buff_cap: int):
        self.cap = int(buff_cap)
        self.data = np.zeros((self.cap, 2))
        self.avg_num_jobs: float | None = None

    def _extend(self, new: np.ndarray) -> None:
        if new.shape[0] > self.cap:
            new = new[-self.cap:]
        keep = self.cap - new.shape[0]
        if keep > 0:
            self.data[:keep] = self.data[-keep:]
        self.data[keep:] = new

    def __call__(self, ro: Rollouts) -> torch.Tensor:
        dt = ro.t_after - ro.t_before
        rows = np.stack([ro.flat(dt).cpu().numpy(), ro.flat(ro.rewards).cpu().numpy()], 1)
        self._extend(rows[rows[:, 0] > 0])
        total_time, rew_sum = self.data.sum(0)
        if _dist_world() > 1:
            total_time, rew_sum = _pool_window_sums(torch.tensor([total_time, rew_sum], dtype=torch.float64, device=ro.rewards.device)).tolist()
            total_time, rew_sum = np.float64(total_time), np.float64(rew_sum)  # (numpy's division: 0 / 0 is nan, not an exception)
        self.avg_num_jobs = -rew_sum / total_time
        T, B = ro.active.shape
        out = torch.zeros_like(ro.rewards)
        R = torch.zeros(B, dtype=torch.float64, device=ro.rewards.device)
        for k in range(T - 1, -1, -1):
            # R = -(job_time - expected_job_time) + R with job_time = -r (returns_calculator.py:57-60)
            R = torch.where(ro.active[k], -(-ro.rewards[k] - dt[k] * self.avg_num_jobs) + R, R)
            out[k] = R
        return out * ro.active


class DeviceDifferentialReturns:
    """`DifferentialReturns` on the record's device (include/sss.h sss_reward_window_update / sss_differential_returns; csrc/
    sss_returns.h): the window is a pair of f64[cap][2] device buffers used in turn, its sums are taken in row order (the bits of
    the host class's numpy sum), and the call makes no device->host transfer and no synchronisation. `avg_num_jobs` reads the
    device scalar when asked. `binding`: as for `discounted_returns` (tests: the emulator's host backend)."""

    def __init__(self, buff_cap: int, binding=None):
        self.cap = int(buff_cap)
        if self.cap < 1:
            raise ValueError("reward_buff_cap must be >= 1")
        self.binding = binding
        self._win: torch.Tensor | None = None   # f64[2, cap, 2]: the window is _win[_cur]
        self._cur = 0
        self._sums: torch.Tensor | None = None  # f64[2] total time, reward sum (pooled over the ranks)
        self._avg: torch.Tensor | None = None   # f64[1]

    @property
    def avg_num_jobs(self) -> float | None:
        return None if self._avg is None else float(self._avg)

    @property
    def data(self) -> np.ndarray:
        """the window's rows (a host copy)"""
        return np.zeros((self.cap, 2)) if self._win is None else self._win[self._cur].cpu().numpy()

    def __call__(self, ro: Rollouts) -> torch.Tensor:
        from .binding import SssDiffretArgs, SssRewardWindowArgs, reward_window_scratch
        b = _record_kernels(ro, self.binding)
        if b is None:
            raise RuntimeError("DeviceDifferentialReturns: the record is not on a GPU and no binding was given (DifferentialReturns is the host form)")
        T, B = ro.active.shape
        dev = ro.active.device
        if self._win is None:
            self._win = torch.zeros((2, self.cap, 2), dtype=torch.float64, device=dev)
            self._sums = torch.empty(2, dtype=torch.float64, device=dev)
            self._avg = torch.empty(1, dtype=torch.float64, device=dev)
        act, tb, ta, rw = ro.active.contiguous().view(torch.uint8), _c64(ro.t_before), _c64(ro.t_after), _c64(ro.rewards)
        scratch = torch.empty(reward_window_scratch(T, B), dtype=torch.int64, device=dev)
        out = torch.empty((T, B), dtype=torch.float64, device=dev)
        w = SssRewardWindowArgs(T, B, act.data_ptr(), tb.data_ptr(), ta.data_ptr(), rw.data_ptr(), self.cap,
                                (ctypes.c_void_p * 2)(self._win[0].data_ptr(), self._win[1].data_ptr()), self._cur, 0, scratch.data_ptr(), self._sums.data_ptr())
        d = SssDiffretArgs(T, B, act.data_ptr(), tb.data_ptr(), ta.data_ptr(), rw.data_ptr(), self._sums.data_ptr(), out.data_ptr(), self._avg.data_ptr())
        with device_of(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
            b.check(b.lib.sss_reward_window_update(ctypes.byref(w), stream))
            if T > 0 and B > 0:
                self._cur = 1 - self._cur  # (the update wrote the other buffer)
            _pool_window_sums(self._sums)
            b.check(b.lib.sss_differential_returns(ctypes.byref(d), stream))
        return out


# ---- baselines (trainers/utils/baselines.py) --------------------------------------------------------

def _interp(x: torch.Tensor, xp: torch.Tensor, fp: torch.Tensor, n: torch.Tensor) -> torch.Tensor:
    """numpy.interp along the last axis for batches: xp rows are non-decreasing with `n` valid
    entries (the rest padding). Same case analysis as numpy's compiled_interp: clamp outside the
    range, the LAST knot j with xp[j] <= x, exact hit -> fp[j], else slope * (x - xp[j]) + fp[j]."""
    Tm = xp.shape[-1]
    ar = torch.arange(Tm, device=xp.device)
    xp_s = torch.where(ar < n[..., None], xp, torch.full_like(xp, float("inf")))
    j = (torch.searchsorted(xp_s, x.contiguous(), right=True) - 1).clamp(min=0)
    last = (n[..., None] - 1).clamp(min=0).expand_as(j)
    j = torch.minimum(j, last)
    j1 = torch.minimum(j + 1, last)
    x0, x1, y0, y1 = xp.gather(-1, j), xp.gather(-1, j1), fp.gather(-1, j), fp.gather(-1, j1)
    slope = (y1 - y0) / (x1 - x0)
    v = slope * (x - x0) + y0
    exact = (x == x0) | (j == last) | (x < x0)
    return torch.where(exact, y0, v)


def numpy_sum_order(terms: list) -> Any:
    """the sum of `terms` (tensors, or floats) in the order numpy's `add.reduce` takes over a float64 axis - what `y_hat.mean()`
    does in baselines.py:33 (numpy's DOUBLE_pairwise_sum): fewer than 8 terms one after the other from 0.0; up to 128 terms eight
    strided partial sums combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail; above that the range is halved (the
    first half rounded down to a multiple of 8). tests/test_emu_training.py checks it against numpy itself."""
    n = len(terms)
    if n < 8:
        res = torch.zeros_like(terms[0]) if n and torch.is_tensor(terms[0]) else 0.0
        for t in terms:
            res = res + t
        return res
    if n <= 128:
        r = list(terms[:8])
        i = 8
        while i < n - (n % 8):
            for k in range(8):
                r[k] = r[k] + terms[i + k]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for t in terms[i:]:
            res = res + t
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return numpy_sum_order(terms[:n2]) + numpy_sum_order(terms[n2:])


def sequence_baselines(ro: Rollouts, values: torch.Tensor, num_sequences: int, num_rollouts: int, binding=None) -> torch.Tensor:
    """for each group of `num_rollouts` consecutive envs (the rollouts of one job sequence) the mean
    over the group's rollouts of their piecewise-linear value curves, evaluated at each rollout's own
    step times (baselines.py:12-37; times = `wall_times[:-1]`, trainer.py:206-207). f64[T,B]"""
    T, B = ro.active.shape
    assert B == num_sequences * num_rollouts
    G, R = num_sequences, num_rollouts
    b = _record_kernels(ro, binding)
    if b is not None and T > 0 and B > 0:  # one kernel, a thread per (step, env) query (below: ~20 operations on [G, R, R, T] tensors)
        from .binding import SssBaselineArgs
        dev = ro.active.device
        act, ts, ys = ro.active.contiguous().view(torch.uint8), _c64(ro.t_before), _c64(values)
        n = ro.active.sum(0).to(torch.int64).contiguous()
        out = torch.empty((T, B), dtype=torch.float64, device=dev)
        # (skip_empty always: with every rollout non-empty it multiplies by 1.0 and divides by R, the same bits - and asking the
        # device whether some rollout is empty would make the host wait for it)
        a = SssBaselineArgs(T, B, R, 1, act.data_ptr(), ts.data_ptr(), ys.data_ptr(), n.data_ptr(), out.data_ptr())
        with device_of(dev):
            b.check(b.lib.sss_sequence_baselines(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0))
        return out
    ts = ro.t_before.t().reshape(G, R, T)
    ys = values.t().reshape(G, R, T)
    n = ro.active.sum(0).reshape(G, R)
    x = ts[:, :, None, :].expand(G, R, R, T)          # query: rollout i's times ...
    xp = ts[:, None, :, :].expand(G, R, R, T)         # ... on rollout j's curve
    fp = ys[:, None, :, :].expand(G, R, R, T)
    nn = n[:, None, :].expand(G, R, R)
    y_hat = _interp(x.contiguous(), xp.contiguous(), fp.contiguous(), nn.contiguous())
    if bool((n > 0).all()):  # (the mean over the sequence's rollouts in numpy's summation order)
        return (numpy_sum_order([y_hat[:, :, j, :] for j in range(R)]) / R).reshape(B, T).t() * ro.active
    # some rollout recorded nothing (its env failed on its first step, on_env_error="truncate"):
    # it has no curve and is left out of its group's mean
    has = (n > 0).to(torch.float64)
    acc = numpy_sum_order([y_hat[:, :, j, :] * has[:, None, j, None] for j in range(R)])
    return (acc / has.sum(1).clamp(min=1)[:, None, None]).reshape(B, T).t() * ro.active


# ---- PPO (trainers/ppo.py) ----------------------------------------------------------------------------

def ppo_loss(policy, g: dict[str, Any], stage_sel, job_idx, exec_sel, advantages: torch.Tensor, old_lgprobs: torch.Tensor,
             clip_range: float, entropy_coeff: float, adv_stats: tuple[float, float] | None = None, weight: float = 1.0):
    """the CLIP loss of ppo.py:104-138 on one minibatch (a compact graph + per-observation vectors).
    Several ranks, each holding a part of the minibatch: `adv_stats` = (mean, std) of the WHOLE minibatch's advantages (ppo.py:113-116
    normalises over the minibatch - the reference has one learner and every sample in it) and `weight` = this rank's share of the
    minibatch x number of ranks, so that the ranks' AVERAGED gradients are the gradient of the whole minibatch's mean loss."""
    res = policy.evaluate_actions(g, stage_sel, job_idx, exec_sel)
    advgs = advantages.float()
    mean, std = (advgs.mean(), advgs.std()) if adv_stats is None else adv_stats
    advgs = (advgs - mean) / (std + EPS)
    log_ratio = res["lgprobs"] - old_lgprobs
    ratio = log_ratio.exp()
    policy_loss = -torch.min(advgs * ratio, advgs * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    entropy_loss = -res["entropies"].mean()
    loss = policy_loss + entropy_coeff * entropy_loss
    if weight != 1.0:
        loss = loss * weight
    with torch.no_grad():
        approx_kl = ((ratio - 1) - log_ratio).mean()
    return loss, {"policy_loss": policy_loss.detach(), "entropy_loss": entropy_loss.detach(), "approx_kl_div": approx_kl}


class PPO:
    """the reference's PPO trainer (trainers/ppo.py + the parts of trainers/trainer.py it uses) on
    the batched env. With `torch.distributed` initialised every rank trains on its own env shard and
    gradients are averaged across ranks before each optimiser step; the KL early-stop test uses the
    all-rank mean so that every rank takes the same number of steps."""

    def __init__(self, policy, train_cfg: dict[str, Any], generator: torch.Generator | None = None):
        self.policy = policy
        self.entropy_coeff = train_cfg.get("entropy_coeff", 0.0)
        self.clip_range = train_cfg.get("clip_range", 0.2)
        self.target_kl = train_cfg.get("target_kl", 0.01)
        self.num_epochs = train_cfg.get("num_epochs", 10)
        self.num_batches = train_cfg.get("num_batches", 3)
        self.num_sequences = int(train_cfg["num_sequences"])
        self.num_rollouts = int(train_cfg["num_rollouts"])
        assert ("reward_buff_cap" in train_cfg) ^ ("beta_discount" in train_cfg), \
            "must provide exactly one of `reward_buff_cap` and `beta_discount` in config"  # trainer.py:63-65
        self.beta = train_cfg.get("beta_discount")
        # differential returns: `diff` starts as the host form; the first record decides (`returns`): on a GPU the kernels take over
        self.diff = DifferentialReturns(train_cfg["reward_buff_cap"]) if "reward_buff_cap" in train_cfg else None
        self.device_returns = True  # (False: the host form also for a record on a GPU - A/B timing, tools/bench_ppo.py --host-returns)
        self.generator = generator

    def returns(self, ro: Rollouts) -> torch.Tensor:
        if self.diff is None:
            return discounted_returns(ro, self.beta)
        if type(self.diff) is DifferentialReturns and self.diff.avg_num_jobs is None and ro.active.is_cuda and self.device_returns:
            self.diff = DeviceDifferentialReturns(self.diff.cap)  # (the first record is on a GPU: the kernels, no fallback from here on)
        return self.diff(ro)

    def preprocess(self, ro: Rollouts):
        returns = self.returns(ro)
        baselines = sequence_baselines(ro, returns, self.num_sequences, self.num_rollouts)
        return returns, baselines

    def _dist(self):
        import torch.distributed as dist
        return dist if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 else None

    def train_on_rollouts(self, ro: Rollouts) -> dict[str, float]:
        returns, baselines = self.preprocess(ro)
        ids = ro.sample_ids()
        advgs = ro.flat(returns - baselines)
        acts = [ro.flat(ro.stage_sel), ro.flat(ro.job_idx), ro.flat(ro.exec_sel)]
        old_lg = ro.flat(ro.lgprobs)
        n = ids.numel()
        bs = n // self.num_batches + 1
        dist = self._dist()
        pol, ent, kls = [], [], []
        go = True
        for _ in range(self.num_epochs):
            if not go:
                break
            perm = torch.randperm(n, generator=self.generator, device=ids.device if self.generator is None or self.generator.device.type != "cpu" else "cpu").to(ids.device)
            # single process: the reference's DataLoader batches (size n // num_batches + 1, ppo.py:66-71).
            # several ranks: exactly num_batches chunks everywhere, so that the collectives line up
            chunks = torch.tensor_split(perm, self.num_batches) if dist else [perm[s: s + bs] for s in range(0, n, bs)]
            whole = None
            if dist:
                # A minibatch is the ranks' chunks TOGETHER, as if one learner held every sample (the reference's does: the workers'
                # rollouts are gathered into one process, trainer.py:113-121, ppo.py:51-138): its advantages are normalised with the
                # mean / std over all ranks' chunks and every rank's loss counts by its share of the samples. One all-reduce per
                # epoch carries the sums of all its minibatches: (count, sum, sum of squares) each, f64.
                a64 = advgs.double()
                whole = torch.stack([torch.stack([torch.tensor(float(mb.numel()), dtype=torch.float64, device=ids.device), a64[mb].sum(), (a64[mb] ** 2).sum()])
                                     for mb in chunks])
                dist.all_reduce(whole)
                whole = whole.cpu()
            for ci, mb in enumerate(chunks):
                stats, weight = None, 1.0
                if dist:
                    N, S1, S2 = (float(v) for v in whole[ci])
                    usable = mb.numel() >= 1 and N >= 2  # (a single sample in the whole minibatch has no advantage std)
                    if usable:
                        mean = S1 / N
                        stats = (mean, max(0.0, (S2 - N * mean * mean) / (N - 1)) ** 0.5)  # (torch.std: the unbiased estimate)
                        weight = mb.numel() * dist.get_world_size() / N
                else:
                    usable = mb.numel() >= 2  # a single sample has no advantage std (the reference would fail on it)
                if usable:
                    g = select_observations(ro.graph, ids[mb])
                    loss, info = ppo_loss(self.policy, g, acts[0][mb], acts[1][mb], acts[2][mb], advgs[mb], old_lg[mb],
                                          self.clip_range, self.entropy_coeff, stats, weight)
                    kl = info["approx_kl_div"]
                else:
                    loss, info, kl = None, None, torch.zeros((), device=ids.device)
                if dist:  # the early-stop test looks at the whole minibatch's mean KL (ppo.py:89-93)
                    stat = torch.stack([kl.float() * (mb.numel() if usable else 0), torch.ones_like(kl.float()) * (mb.numel() if usable else 0)])
                    dist.all_reduce(stat)
                    kl = stat[0] / stat[1].clamp(min=1)
                elif not usable:
                    continue
                kl = float(kl)
                if usable:
                    pol.append(float(info["policy_loss"]))
                    ent.append(float(info["entropy_loss"]))
                kls.append(kl)
                if self.target_kl is not None and kl > 1.5 * self.target_kl:
                    go = False
                    break
                if usable:
                    loss.backward()
                if dist:
                    # ONE all-reduce per optimiser step: the whole gradient (20.8 k floats = 83 KB for the
                    # published architecture) as a single bucket - latency-bound on xGMI, so fewer, larger
                    # messages is all there is to tune
                    params = list(self.policy.parameters())
                    for p in params:
                        if p.grad is None:
                            p.grad = torch.zeros_like(p)
                    flat = torch.cat([p.grad.reshape(-1) for p in params])
                    dist.all_reduce(flat)
                    flat /= dist.get_world_size()
                    off = 0
                    for p in params:
                        k = p.numel()  # not `n`: that is the number of samples the epochs permute
                        p.grad.copy_(flat[off: off + k].view_as(p))
                        off += k
                self.policy.update_parameters(None)
        # (`minibatches`: optimiser steps taken - fewer than epochs x batches when the KL test stopped the epochs, ppo.py:89-93)
        return {"policy loss": abs(float(np.mean(pol))), "entropy": abs(float(np.mean(ent))), "approx kl div": abs(float(np.mean(kls))), "minibatches": len(pol)}


@contextlib.contextmanager
def deterministic_scope(fill_uninitialized_memory: bool = False):
    """`torch.use_deterministic_algorithms(True)` for the duration of the block, with torch's
    `torch.utils.deterministic.fill_uninitialized_memory` set as given (False by default: its fills would write every `empty`
    buffer of a multi-GB update, and no result here depends on that memory). Both are restored on exit, also when an exception
    escapes. The row kernels of the update read the flag at every call (train_kernels.deterministic_enabled)."""
    import torch.utils.deterministic as tud

    prev, prev_warn, prev_fill = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(), tud.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True)
    tud.fill_uninitialized_memory = fill_uninitialized_memory
    try:
        yield
    finally:
        tud.fill_uninitialized_memory = prev_fill
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


class Trainer:
    """the reference's training loop (trainers/trainer.py:27-168) with the rollout workers replaced
    by the batched env: per iteration collect `num_sequences x num_rollouts` rollouts (per rank),
    update the policy, track / checkpoint the best parameters.

    With torch.distributed initialised (one process per GPU) every rank owns `num_sequences` job
    sequences of its own (base seeds are a function of the global sequence id, so the union over
    ranks does not depend on the placement), rollouts of one sequence stay on one rank (their
    baseline needs no traffic), gradients are averaged across ranks and ONE all-gather per
    iteration moves the per-rollout statistics (trainer.py:113-121's Pipe gather).

    Deterministic mode (`deterministic=True`, or the `deterministic` key of the trainer section): `train()` runs inside
    `deterministic_scope()`, so that the same config, seed and record give the same parameters bit for bit on the same software
    and hardware. Not verified across several ranks (the collective's reduction order is the library's)."""

    def __init__(self, agent_cfg: dict[str, Any], env_cfg: dict[str, Any], train_cfg: dict[str, Any],
                 device: str | torch.device | None = None, _lib=None, pack: bytes | None = None, deterministic: bool | None = None):
        """`pack`: the workload pack the envs run on (None: the frozen default trace set); `deterministic`: None reads
        train_cfg["deterministic"] (default False)"""
        import torch.distributed as dist

        from .decima import DecimaPolicy
        from .vec_env import VecSparkSchedSimEnv

        self.rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.seed = int(train_cfg["seed"])
        torch.manual_seed(self.seed)
        self.num_iterations = int(train_cfg["num_iterations"])
        self.num_sequences = int(train_cfg["num_sequences"])
        self.num_rollouts = int(train_cfg["num_rollouts"])
        self.rollout_duration = train_cfg.get("rollout_duration")
        self.deterministic = bool(train_cfg.get("deterministic", False) if deterministic is None else deterministic)
        if self.deterministic and self.rollout_duration:
            raise ValueError("trainer: `deterministic: true` cannot be combined with `rollout_duration` (asynchronous collection is paced by the wall clock)")
        if int(train_cfg.get("collector_groups", 1)) != 1:
            raise ValueError("trainer: `collector_groups` other than 1 is no longer supported (alternating groups of envs on their own streams were measured "
                             "slower on one MI355X, profiles/r03_ppo.md, never verified with `deterministic: true`, and removed): drop the key")
        self.checkpointing_freq = int(train_cfg.get("checkpointing_freq", 50))
        self.artifacts_dir = train_cfg.get("artifacts_dir", "artifacts")
        self.env_cfg = dict(env_cfg)
        if "beta_discount" in train_cfg:
            self.env_cfg["beta"] = train_cfg["beta_discount"]  # trainer.py:70-72
        assert agent_cfg.get("agent_cls", "DecimaScheduler") == "DecimaScheduler"
        dev = torch.device(device if device is not None else train_cfg.get("device", "cuda:0"))
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", 0)
        self.device = dev
        if dev.type == "cuda" and train_cfg.get("allocator_rounding", True):
            # The sizes of a minibatch's tensors (GBs at BASELINE config 5) differ by a percent from one minibatch to the next; the
            # caching allocator then keeps asking the driver for slightly larger blocks (0.1 s per hipMalloc, 0.9 s of a 3.4 s
            # update: profiles/r04_ppo.md). Rounding request sizes up to eighths of a power of two makes the blocks reusable.
            try:
                (getattr(torch._C, "_accelerator_setAllocatorSettings", None) or torch.cuda.memory._set_allocator_settings)("roundup_power2_divisions:8")
            except Exception:  # (an allocator backend without the option)
                pass
        E = int(self.env_cfg["num_executors"])
        kw = {k: v for k, v in agent_cfg.items() if k != "agent_cls"}
        self.policy = DecimaPolicy(num_executors=E, opt_cls=train_cfg["opt_cls"], opt_kwargs=train_cfg.get("opt_kwargs"),
                                   max_grad_norm=train_cfg.get("max_grad_norm"), **kw).to(dev)
        B = self.num_sequences * self.num_rollouts
        sim_cfg = {k: v for k, v in self.env_cfg.items() if k not in ("mean_time_limit", "dataset")}
        self.env = VecSparkSchedSimEnv(sim_cfg, B, device=dev, _lib=_lib, pack=pack)
        total_sequences = self.num_sequences * self.world
        seq_ids = self.rank * self.num_sequences + np.arange(self.num_sequences)
        base_seeds = np.repeat(self.seed + seq_ids, self.num_rollouts)  # trainer.py:264-266
        gen = torch.Generator(device=dev if dev.type == "cuda" else "cpu")
        gen.manual_seed(self.seed * 1000003 + self.rank)
        self.collector = RolloutCollector(self.env, self.env_cfg["mean_time_limit"], base_seeds, total_sequences, E,
                                          policy=self.policy, generator=gen, on_env_error=train_cfg.get("on_env_error", "raise"))
        self.ppo = PPO(self.policy, train_cfg, generator=gen)
        self.history: list[dict[str, float]] = []
        # evaluation on held-out job sequences while training (off by default): every `eval_every` iterations `eval_envs` whole
        # episodes from `eval_seed` on an env of its own, under the policy (`eval_greedy`: arg-max actions) and under fair
        self.eval_every = int(train_cfg.get("eval_every", 0) or 0)
        self.eval_envs = int(train_cfg.get("eval_envs", 64))
        self.eval_seed = int(train_cfg.get("eval_seed", 10_000_000))
        self.eval_greedy = bool(train_cfg.get("eval_greedy", True))
        self.eval_history: list[dict[str, Any]] = []
        self._eval = None
        self._eval_env_args = dict(env_cfg=sim_cfg, device=dev, _lib=_lib, pack=pack)

    def evaluate(self, tag: int | None = None) -> dict[str, Any]:
        """`eval_envs` held-out job sequences (seeds from `eval_seed`) played to their end under the current policy and under the fair
        scheduler on the trainer's evaluation env (created at the first call, fair's episodes played once): the paired summary of
        `evaluation.compare` over each episode's own mean job duration. Leaves the training run as it found it: the policy's draw
        counter, its training mode and the collector's generator are not touched (sampled evaluation draws from a generator of its own)."""
        from .evaluation import compare, run_episodes
        from .vec_env import VecSparkSchedSimEnv

        if self._eval is None:
            a = self._eval_env_args
            env = VecSparkSchedSimEnv(a["env_cfg"], self.eval_envs, device=a["device"], _lib=a["_lib"], pack=a["pack"])
            gen = torch.Generator(device=self.device if self.device.type == "cuda" else "cpu")
            gen.manual_seed(self.eval_seed)
            self._eval = {"env": env, "gen": gen, "fair": run_episodes(env, "fair", self.eval_seed)}
        ev = self._eval
        was_training, calls = self.policy.training, getattr(self.policy, "_calls", 0)
        self.policy.eval()
        try:
            res = {"fair": ev["fair"], "decima": run_episodes(ev["env"], self.policy, self.eval_seed, greedy=self.eval_greedy, generator=ev["gen"])}
        finally:
            self.policy._calls = calls
            self.policy.train(was_training)
        row = compare(res, metric="episode_avg_job_duration_s")
        row["after_iterations"], row["greedy"] = tag, self.eval_greedy
        return row

    def _gather_stats(self, stats: dict[str, np.ndarray]) -> dict[str, np.ndarray]:
        import torch.distributed as dist
        keys = sorted(stats)
        local = torch.from_numpy(np.stack([stats[k] for k in keys], 1)).to(self.device)
        if self.world > 1:
            out = [torch.empty_like(local) for _ in range(self.world)]
            dist.all_gather(out, local)
            local = torch.cat(out, 0)
        arr = local.cpu().numpy()
        return {k: arr[:, i] for i, k in enumerate(keys)}

    def train(self, verbose: bool = True) -> list[dict[str, float]]:
        if self.deterministic:
            with deterministic_scope():
                return self._train(verbose)
        return self._train(verbose)

    def _train(self, verbose: bool) -> list[dict[str, float]]:
        import json
        import os
        import os.path as osp
        from copy import deepcopy

        ckpt_dir = osp.join(self.artifacts_dir, "checkpoints")
        if self.rank == 0:
            os.makedirs(ckpt_dir, exist_ok=True)
        best = None
        for i in range(self.num_iterations):
            state_dict = deepcopy(self.policy.state_dict())
            self.policy.eval()
            ro = (self.collector.collect_async(self.rollout_duration) if self.rollout_duration else self.collector.collect_sync())
            self.policy.train()
            learn = self.ppo.train_on_rollouts(ro)
            stats = self._gather_stats(ro.stats)
            with np.errstate(all="ignore"):
                avg_num_jobs = (self.ppo.diff.avg_num_jobs if self.ppo.diff is not None else None) or float(np.mean(stats["avg_num_jobs"]))
            if not best or avg_num_jobs < best["avg_num_jobs"]:  # trainer.py:138-142
                best = {"iteration": i, "avg_num_jobs": float(np.round(avg_num_jobs, 3)), "state_dict": state_dict,
                        "completed_job_count": int(np.mean(stats["num_completed_jobs"]))}
            if (i + 1) % self.checkpointing_freq == 0 and self.rank == 0:
                d = osp.join(ckpt_dir, f"{i + 1}")
                os.makedirs(d, exist_ok=True)
                torch.save(best.pop("state_dict"), osp.join(d, "model.pt"))
                with open(osp.join(d, "state.json"), "w") as fp:
                    json.dump(best, fp)
                best = None
            elif (i + 1) % self.checkpointing_freq == 0:
                best = None
            rec = dict(learn, iteration=i, avg_num_jobs=float(avg_num_jobs), samples=int(ro.active.sum()), env_errors=self.collector.env_errors,
                       episode_length=float(ro.lengths.float().mean()))
            self.history.append(rec)
            if self.eval_every and (i + 1) % self.eval_every == 0 and self.rank == 0:
                self.eval_history.append(self.evaluate(i + 1))
            if verbose and self.rank == 0:
                print(f"Iteration {i + 1} complete. Avg. # jobs: {avg_num_jobs:.3f}", flush=True)
        return self.history

    def close(self) -> None:
        self.env.close()
        if self._eval is not None:
            self._eval["env"].close()


def make_trainer(cfg: dict[str, Any], device: str | torch.device | None = None, _lib=None) -> Trainer:
    """by-name factory like the reference's (trainers/__init__.py:7-13): `cfg` is the parsed YAML
    with its `trainer` / `agent` / `env` sections"""
    trainer_cls = cfg["trainer"]["trainer_cls"]
    assert trainer_cls == "PPO", f"'{trainer_cls}' is not a valid trainer."  # PPO is the trainer of BASELINE config 5
    return Trainer(agent_cfg=cfg["agent"], env_cfg=cfg["env"], train_cfg=cfg["trainer"], device=device, _lib=_lib)
