"""Batched Spark-scheduling environment: the host-side mirror of the reference's
`SparkSchedSimEnv` (reference spark_sched_sim/spark_sched_sim.py:29-245) over `num_envs`
independent simulations that live in HBM and are stepped by the HIP kernels behind include/sss.h.

PyTorch only provides device memory and streams here: every buffer is a torch tensor whose raw
pointer is handed to the C ABI, so observations come back as device tensors without a copy.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Sequence

import numpy as np
import torch

from . import workload
from .binding import (ERROR_NAMES, POLICY_IDS, WFAIR_ALPHA_RANGE, Binding, SssBuffers, SssCfg, SssDecimaGraph, SssDecimaLists, SssTimeline,
                      SssTimelineRenderArgs, device_of)

OBS_FIELDS = ("n_nodes", "n_edges", "n_jobs", "n_schedulable", "num_committable_execs", "source_job_idx",
              "terminated", "err")
NUM_NODE_FEATURES = 3  # reference spark_sched_sim.py:25


class BatchedObs(dict):
    """dict of device tensors; rows beyond n_nodes[i] / n_edges[i] / n_jobs[i] of env i are padding.

    keys: nodes f32[B, node_cap, 3], edge_links i32[B, edge_cap, 2], dag_ptr i32[B, job_cap+1],
    exec_supplies i32[B, job_cap], plus one i32[B] tensor per OBS_FIELDS entry.
    """


def _mask_u8(mask: torch.Tensor | None) -> torch.Tensor | None:
    """an env mask as the u8 array the kernels read: a view when it already is one byte per env (bool / uint8, contiguous)"""
    if mask is None:
        return None
    if mask.is_contiguous() and mask.dtype in (torch.bool, torch.uint8):
        return mask.view(torch.uint8)
    return mask.to(torch.uint8).contiguous()


class LateHint:
    """A few device integers read back WITHOUT waiting for them: `post(t)` enqueues a copy of `t` to pinned host memory on the current
    stream, `read()` returns the most recent copy that has COMPLETED (all `fill` until one has) - two host buffers taken in turn,
    each with an event recorded behind its copy, so that a buffer is never read while a copy into it may be in flight (a plain
    pinned tensor read while the previous call's non_blocking copy was still running gave torn / half-old values). The values only
    size grids and work buffers: late ones are fine, undefined ones are not. CPU tensors: the copy is synchronous."""

    def __init__(self, n: int, device: torch.device, fill: int = -1):
        self.cuda = device.type == "cuda"
        self.fill = torch.full((n,), fill, dtype=torch.int64)
        bufs = [torch.full((n,), fill, dtype=torch.int64) for _ in range(2)]
        self.bufs = [b.pin_memory() for b in bufs] if self.cuda else bufs
        self.events = [torch.cuda.Event() for _ in range(2)] if self.cuda else None
        self.posted = [False, False]
        self.tags = [None, None]
        self.last = 1

    def read(self) -> torch.Tensor:
        return self.read_tagged()[0]

    def read_tagged(self):
        """(values, the `tag` their `post` was given); (fill, None) until a copy has completed. With the host several steps ahead of
        the device BOTH buffers can be waiting for their copies: the values of the last completed one are kept and returned again
        (returning the fill value then sized every grid by its capacity for as long as the host stayed ahead)"""
        for k in (self.last, 1 - self.last):
            if self.posted[k] and (not self.cuda or self.events[k].query()):
                self.kept = (self.bufs[k].clone(), self.tags[k])
                break
        kept = getattr(self, "kept", None)
        return (kept[0].clone(), kept[1]) if kept is not None else (self.fill.clone(), None)

    def post(self, t: torch.Tensor, tag=None) -> None:
        k = 1 - self.last
        if self.cuda and self.posted[k] and not self.events[k].query():
            return  # (the copy before last has not even finished: the host is far ahead - skip this one rather than wait)
        self.bufs[k].copy_(t, non_blocking=True)
        if self.cuda:
            self.events[k].record(torch.cuda.current_stream(t.device))
        self.posted[k], self.last, self.tags[k] = True, k, tag


class VecSparkSchedSimEnv:
    """`num_envs` reference environments in one object.

    env_cfg keys are the reference's (`num_executors`, `job_arrival_cap`, `job_arrival_rate`,
    `moving_delay`, `warmup_delay`, optional `beta`; `data_sampler_cls` must be "TPCHDataSampler"
    if present) plus optional `max_jobs` (arena capacity when `job_arrival_cap` is None).
    """

    def __init__(self, env_cfg: dict[str, Any], num_envs: int, device: str | torch.device = "cuda:0",
                 pack: bytes | None = None, auto_reset: bool = False, seed_stride: int | None = None,
                 _lib: C.CDLL | None = None) -> None:
        self.device = torch.device(device)
        if self.device.type != "cuda" and _lib is None:
            raise RuntimeError("VecSparkSchedSimEnv runs on an AMD GPU (device='cuda:N'); there is no CPU path")
        sampler = env_cfg.get("data_sampler_cls", "TPCHDataSampler")
        if sampler != "TPCHDataSampler":
            raise ValueError(f"'{sampler}' is not a valid data sampler.")  # data_samplers/__init__.py:12-14
        self.num_envs = int(num_envs)
        self.num_executors = int(env_cfg["num_executors"])
        self.env_cfg = dict(env_cfg)
        self.auto_reset = bool(auto_reset)
        self.seed_stride = int(seed_stride if seed_stride is not None else num_envs)
        self._b = Binding(_lib)
        self._pack = pack if pack is not None else workload.default_pack()
        cap = env_cfg.get("job_arrival_cap")
        self._cfg = SssCfg(self.num_executors, int(cap) if cap else 0, int(env_cfg.get("max_jobs") or 0), 0,
                           float(env_cfg["job_arrival_rate"]), float(env_cfg["moving_delay"]),
                           float(env_cfg["warmup_delay"]), float(env_cfg.get("beta", 0.0)))
        self.dims = self._b.query_dims(self._cfg, self._pack, self.num_envs)
        dev_index = self.device.index or 0
        self._h = self._b.create(self._cfg, self._pack, self.num_envs, dev_index if self.device.type == "cuda" else -1)
        d, B, dev = self.dims, self.num_envs, self.device
        # the arena must start zeroed (lifetime counters) and 256-byte aligned
        self._state_raw = torch.zeros(d.state_bytes + 256, dtype=torch.uint8, device=dev)
        off = (-self._state_raw.data_ptr()) % 256
        self.state = self._state_raw[off: off + d.state_bytes]
        self.nodes = torch.zeros((B, d.node_cap, NUM_NODE_FEATURES), dtype=torch.float32, device=dev)
        self.edge_links = torch.zeros((B, d.edge_cap, 2), dtype=torch.int32, device=dev)
        self.dag_ptr = torch.zeros((B, d.job_cap + 1), dtype=torch.int32, device=dev)
        self.exec_supplies = torch.zeros((B, d.job_cap), dtype=torch.int32, device=dev)
        self.obs_i32 = torch.zeros((B, d.obs_i32), dtype=torch.int32, device=dev)
        self.obs_f64 = torch.zeros((B, d.obs_f64), dtype=torch.float64, device=dev)
        self.rebind_buffers()
        self._seeds = torch.zeros(B, dtype=torch.int64, device=dev)
        self._tl = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
        self._mask = torch.ones(B, dtype=torch.uint8, device=dev)
        self._env_view = self.state.view(B, d.env_stride)
        self._act_stage = torch.zeros(B, dtype=torch.int32, device=dev)
        self._act_nexec = torch.ones(B, dtype=torch.int32, device=dev)
        self._closed = False
        self._dg_pool: dict[int, torch.Tensor] = {}
        self._layer_scratch: dict = {}
        self._never = None
        from .workload import pack_max_depth
        self.max_dag_depth = pack_max_depth(self._pack)  # bound of an observation's DAG layers: sizes sss_gnn_encode's layer launches
        # gymnasium.vector.VectorEnv attributes; the per-env action space is the reference's at
        # construction (its stage_idx bound follows each observation: valid range is [-1, n_nodes[i]))
        from .spaces import make_action_space, make_observation_space
        self.single_action_space = make_action_space(self.num_executors)
        self.action_space = self.single_action_space
        # per-env observation space of the reference (its two episode-dependent bounds are those of the env at
        # construction here; the per-env views of the facade keep them current, env.py)
        self.single_observation_space = make_observation_space(self.num_executors, NUM_NODE_FEATURES)
        self.observation_space = self.single_observation_space

    # ---- plumbing ---------------------------------------------------------------------

    def rebind_buffers(self) -> None:
        """(re)registers the observation / state tensors with the library (include/sss.h sss_bind_buffers). Every
        call starts a new buffer generation: rows the env skips while nothing changed (the edge rows of an
        unchanged active subgraph) are written again at the next step. The supported way to hand over new
        buffers - or buffers whose contents were changed behind the env's back: assign the tensors, then call this."""
        bufs = SssBuffers(self.state.data_ptr(), self.nodes.data_ptr(), self.edge_links.data_ptr(),
                          self.dag_ptr.data_ptr(), self.exec_supplies.data_ptr(), self.obs_i32.data_ptr(),
                          self.obs_f64.data_ptr())
        self._b.check(self._b.lib.sss_bind_buffers(self._h, C.byref(bufs)))
        self._bind_timeline()  # (a recording that is on stays on)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0

    def _obs(self) -> BatchedObs:
        o = BatchedObs(nodes=self.nodes, edge_links=self.edge_links, dag_ptr=self.dag_ptr,
                       exec_supplies=self.exec_supplies)
        for k, name in enumerate(OBS_FIELDS):
            o[name] = self.obs_i32[:, k]
        return o

    def close(self) -> None:
        if not self._closed:
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self._b.lib.sss_destroy(self._h)
            self._closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- Gymnasium-style API ----------------------------------------------------------

    def reset(self, *, seed: int | Sequence[int] | None = None, options: dict[str, Any] | None = None,
              mask: torch.Tensor | None = None):
        """reference `reset(seed, options)` (spark_sched_sim.py:127-186) for every env (or the
        envs selected by `mask`). `seed`: int -> env i gets seed + i; sequence -> per env;
        None -> fresh entropy, as `gymnasium.Env.reset(seed=None)` does."""
        B = self.num_envs
        if seed is None:
            seeds = np.random.SeedSequence().generate_state(B, np.uint64) >> np.uint64(1)
        elif isinstance(seed, (int, np.integer)):
            seeds = np.arange(B, dtype=np.uint64) + np.uint64(int(seed))
        else:
            seeds = np.asarray(list(seed), dtype=np.uint64)
            if seeds.shape != (B,):
                raise ValueError("need one seed per env")
        self._seeds.copy_(torch.from_numpy(seeds.view(np.int64)))
        tl = (options or {}).get("time_limit", np.inf)
        tl_arr = np.broadcast_to(np.asarray(tl, dtype=np.float64), (B,)).copy()
        self._tl.copy_(torch.from_numpy(tl_arr))
        mask_ptr = None
        if mask is not None:
            self._mask.copy_(mask.to(torch.uint8))
            mask_ptr = self._mask.data_ptr()
        self._b.check(self._b.lib.sss_reset(self._h, self._seeds.data_ptr(), self._tl.data_ptr(), mask_ptr, self._stream()))
        return self._obs(), {"wall_time": self.obs_f64[:, 1]}

    def step_async(self, stage_idx: torch.Tensor, num_exec: torch.Tensor) -> None:
        """launches one `step(action)` per env on the current stream and returns immediately"""
        assert stage_idx.dtype == torch.int32 and num_exec.dtype == torch.int32
        assert stage_idx.device == self.device and stage_idx.is_contiguous() and num_exec.is_contiguous()
        self._b.check(self._b.lib.sss_step(self._h, stage_idx.data_ptr(), num_exec.data_ptr(), int(self.auto_reset),
                                           self.seed_stride, self._stream()))

    def step_bounded_async(self, stage_idx: torch.Tensor, num_exec: torch.Tensor, max_events: int, ready: torch.Tensor | None = None) -> torch.Tensor:
        """`step_async` with an event budget per launch (include/sss.h sss_step_bounded): an env whose step needs more than
        `max_events` events is cut between two events and goes on in the next call (its action entries are then ignored).
        Returns `ready` u8[B] (the env's buffer unless one is given): 1 = the env's step is complete and its outputs are
        current, 0 = it continues - its observation / reward / flags are still the previous ones. Envs run at their own
        pace, as the reference's envs do in their worker processes; each env's trajectory is the one `step` gives."""
        assert stage_idx.dtype == torch.int32 and num_exec.dtype == torch.int32
        assert stage_idx.device == self.device and stage_idx.is_contiguous() and num_exec.is_contiguous()
        if ready is None:
            if getattr(self, "_ready", None) is None:
                self._ready = torch.ones(self.num_envs, dtype=torch.uint8, device=self.device)
            ready = self._ready
        assert ready.dtype == torch.uint8 and ready.is_contiguous() and ready.numel() == self.num_envs
        self._b.check(self._b.lib.sss_step_bounded(self._h, stage_idx.data_ptr(), num_exec.data_ptr(), int(self.auto_reset), self.seed_stride, int(max_events),
                                                   ready.data_ptr(), self._stream()))
        return ready

    def step(self, actions):
        """reference `step(action)` (spark_sched_sim.py:188-221), batched.
        `actions`: {"stage_idx": i32[B], "num_exec": i32[B]} (tensors on the env's device).
        Returns (obs, reward f64[B], terminated bool[B], truncated bool[B], info).

        Aliasing contract: `obs` holds VIEWS of the env's observation buffers - the next step / reset
        overwrites them in place (zero-copy hand-off to a policy on the device). The small per-env
        vectors a loop typically keeps across steps - reward, terminated, info["wall_time"],
        info["err"] - are copies. `step_async` + the buffers themselves is the copy-free path."""
        if set(actions.keys()) != {"stage_idx", "num_exec"}:
            raise ValueError("invalid action: does not belong to the action space")  # Dict.contains
        self.step_async(actions["stage_idx"], actions["num_exec"])
        obs = self._obs()
        # the small per-env vectors are COPIES (two copy launches + one compare): reward / wall_time, terminated / err
        f64 = self.obs_f64.clone()
        i32 = self.obs_i32[:, 6:8].clone()
        terminated = i32[:, 0] != 0
        if self._never is None or self._never.shape != terminated.shape:
            self._never = torch.zeros_like(terminated)  # (truncation is the time-limit wrapper's business: always False here; shared, read-only)
        return obs, f64[:, 0], terminated, self._never, {"wall_time": f64[:, 1], "err": i32[:, 1]}

    # ---- executor timelines (the reference's Executor.history) and Gantt frames -----------------

    def _bind_timeline(self) -> None:
        tl = getattr(self, "_timeline", None)
        if tl is None:
            self._b.check(self._b.lib.sss_bind_timeline(self._h, None))
            return
        t, job, count = tl
        a = SssTimeline(t.data_ptr(), job.data_ptr(), count.data_ptr(), t.shape[2], 0)
        self._b.check(self._b.lib.sss_bind_timeline(self._h, C.byref(a)))

    def enable_timeline(self, cap: int = 256) -> None:
        """starts recording every executor's history on the device (include/sss.h sss_bind_timeline; the reference's
        `Executor.history`, components/executor.py:21-44): `cap` entries are stored per executor, further ones are only counted.
        The rows start as after a reset - one open entry [None, -1] - so a recording describes an episode when it is enabled
        before the episode's `reset`; every reset (also an auto-reset inside a launch) restarts the env's rows."""
        cap = int(cap)
        if cap < 1:
            raise ValueError(f"enable_timeline: cap must be >= 1, got {cap}")
        B, E, dev = self.num_envs, self.num_executors, self.device
        t = torch.full((B, E, cap), float("nan"), dtype=torch.float64, device=dev)
        job = torch.full((B, E, cap), -1, dtype=torch.int32, device=dev)
        count = torch.ones((B, E), dtype=torch.int32, device=dev)
        self._timeline = (t, job, count)
        self._bind_timeline()

    def disable_timeline(self) -> None:
        self._timeline = None
        self._bind_timeline()

    def timeline_arrays(self) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(t f64[B, E, cap], job i32[B, E, cap], count i32[B, E]) - the device tensors the kernels write. Entry k < count - 1 holds
        its release time, the open entry NaN; count is the true number of entries and may exceed cap (the rest is not stored)"""
        if getattr(self, "_timeline", None) is None:
            raise RuntimeError("no timeline is being recorded: call enable_timeline() first")
        return self._timeline

    def timeline(self, i: int) -> list[list[list]]:
        """env i's histories in the reference's shape: per executor the list of [t, job_id] pairs, None in the open entry's t
        (one device->host copy). Raises when an executor has more entries than the capacity holds."""
        t, job, count = self.timeline_arrays()
        cap = t.shape[2]
        cnt = count[i].cpu().numpy()
        if int(cnt.max()) > cap:
            raise RuntimeError(f"timeline of env {i} overflowed: executor {int(cnt.argmax())} has {int(cnt.max())} entries, the capacity is {cap}; "
                               f"enable_timeline(cap={int(cnt.max())}) would have held the episode")
        tt, jj = t[i].cpu().numpy(), job[i].cpu().numpy()
        return [[[None if k == n - 1 else float(tt[e, k]), int(jj[e, k])] for k in range(n)] for e, n in enumerate(cnt.tolist())]

    def render(self, env_ids=None, width: int = 400, height: int = 300) -> torch.Tensor:
        """Gantt frames of the recorded timelines, uint8 [n, height, width, 3] on the device, written by one kernel (include/sss.h
        sss_timeline_render, where the frame is defined): one band of rows per executor coloured by the job it belongs to over
        [0, wall_time), black = the common pool, red columns = job completions, grey = beyond the recording's capacity.
        `env_ids`: the envs to draw (any sequence / tensor of indices), None = all."""
        self.timeline_arrays()
        dev = self.device
        if env_ids is None:
            ids, n = None, self.num_envs
        else:
            ids = torch.as_tensor(env_ids, dtype=torch.int32).reshape(-1).to(dev).contiguous()
            n = int(ids.numel())
            if n and (int(ids.min()) < 0 or int(ids.max()) >= self.num_envs):
                raise IndexError("render: env id out of range")
        rgb = torch.empty((n, int(height), int(width), 3), dtype=torch.uint8, device=dev)
        a = SssTimelineRenderArgs(ids.data_ptr() if ids is not None and n else None, n, int(width), int(height), 0, rgb.data_ptr() if n else None)
        self._b.check(self._b.lib.sss_timeline_render(self._h, C.byref(a), self._stream()))
        return rgb

    # ---- on-device policies and fused rollouts ---------------------------------------------

    @staticmethod
    def _policy_id(policy: str, param: int) -> int:
        pid = POLICY_IDS[policy]
        lo, hi = WFAIR_ALPHA_RANGE
        if policy == "wfair" and not lo <= int(param) <= hi:
            raise ValueError(f"wfair: alpha (param) must be an integer in [{lo}, {hi}], got {param}")
        return pid

    def policy_actions(self, policy: str = "fair", param: int = 0):
        """one action per env from an on-device heuristic; returns {"stage_idx", "num_exec"} device tensors (re-used buffers).

        "fair" / "fifo": the reference's RoundRobinScheduler with / without dynamic partitioning; "hash": the build's counter-based
        uniform-random policy (param = per-mille probability of stage_idx = -1); "wfair": weighted fair, executor caps in proportion
        to job work^alpha (param = alpha, an integer in [-4, 4]; ValueError otherwise); "sjfcp": shortest job first, inside it the
        stage at the head of the critical path (param unused). "wfair" / "sjfcp" equal the host plugins WeightedFairScheduler /
        SJFCPScheduler (schedulers.py) on `obs_view(i)` bit for bit."""
        pid = self._policy_id(policy, param)
        self._b.check(self._b.lib.sss_policy(self._h, pid, int(param), self._act_stage.data_ptr(),
                                             self._act_nexec.data_ptr(), self._stream()))
        return {"stage_idx": self._act_stage, "num_exec": self._act_nexec}

    def rollout(self, policy: str, n_steps: int, param: int = 0) -> None:
        """n_steps x (policy -> step) per env inside one kernel launch (asynchronous); `policy` / `param` as for
        `policy_actions`"""
        pid = self._policy_id(policy, param)
        self._b.check(self._b.lib.sss_rollout(self._h, pid, int(param), int(n_steps), int(self.auto_reset),
                                              self.seed_stride, self._stream()))

    def _i32_per_env(self, t: torch.Tensor, what: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or t.numel() != self.num_envs:
            raise ValueError(f"{what}: need a contiguous int32 tensor of {self.num_envs} entries on {self.device}")
        return t

    def rollout_each(self, policy: torch.Tensor, param: torch.Tensor, n_steps: int, first_policy: torch.Tensor | None = None,
                     first_param: torch.Tensor | None = None, out: dict[str, torch.Tensor] | None = None) -> dict[str, torch.Tensor]:
        """the fused rollout with a policy per env (include/sss.h sss_rollout_each), one asynchronous launch and no host sync: env i
        takes up to `n_steps` steps under policy id `policy[i]` with `param[i]` (`binding.POLICY_IDS`; int32 device tensors [B]) and
        stops at the end of its episode or at an env error - there is no auto-reset here, whatever the env's `auto_reset` says.
        `policy[i] == -1` leaves env i untouched byte for byte. `first_policy` / `first_param` (both or neither): the policy of
        the env's first step in this launch where the entry is >= 0. The tensors' values are not read back: an id outside the table
        or a weighted-fair alpha outside [-4, 4] makes the kernel skip that env and report `steps[i] == -1`.
        Returns {"steps", "first_stage_idx", "first_num_exec"} (int32 [B], on the device): the steps env i took and the action of
        its first one. They are fresh tensors (0 / -1 / 0 for envs that took no part) unless `out` - such a dict from an earlier
        call - is given: then those are written again, and entries of envs that take no part keep what they held.
        Not available while a timeline is recorded (ValueError)."""
        B, dev = self.num_envs, self.device
        pol, par = self._i32_per_env(policy, "rollout_each: policy"), self._i32_per_env(param, "rollout_each: param")
        if (first_policy is None) != (first_param is None):
            raise ValueError("rollout_each: first_policy and first_param come together or not at all")
        fpol = self._i32_per_env(first_policy, "rollout_each: first_policy") if first_policy is not None else None
        fpar = self._i32_per_env(first_param, "rollout_each: first_param") if first_param is not None else None
        if out is None:
            out = {"steps": torch.zeros(B, dtype=torch.int32, device=dev), "first_stage_idx": torch.full((B,), -1, dtype=torch.int32, device=dev),
                   "first_num_exec": torch.zeros(B, dtype=torch.int32, device=dev)}
        o = [self._i32_per_env(out[k], f"rollout_each: out[{k!r}]") for k in ("steps", "first_stage_idx", "first_num_exec")]
        self._b.check(self._b.lib.sss_rollout_each(self._h, pol.data_ptr(), par.data_ptr(), fpol.data_ptr() if fpol is not None else None,
                                                   fpar.data_ptr() if fpar is not None else None, int(n_steps), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                   self._stream()))
        return out

    def rollout_action(self, policy: torch.Tensor, param: torch.Tensor, n_steps: int, first_stage: torch.Tensor, first_exec: torch.Tensor,
                       out: dict[str, torch.Tensor] | None = None) -> dict[str, torch.Tensor]:
        """`rollout_each` whose first step is a given ACTION (include/sss.h sss_rollout_action without policy arguments), one
        asynchronous launch and no host sync: where `first_exec[i] >= 1` env i first takes `(first_stage[i], first_exec[i])` verbatim,
        as `step` would, and then up to `n_steps - 1` steps under `policy[i]` / `param[i]`; `first_exec[i] == 0` forces nothing (the
        policy decides every step); `first_exec[i] < 0` leaves env i untouched byte for byte, like `policy[i] == -1`. An action the env
        refuses leaves the env's error as `step` does, ends the env's part and is not counted in `steps`. All four are int32 device
        tensors [B]; nothing is read back. Returns `rollout_each`'s dict (`out`: such a dict to write again). The heuristics' ids only:
        `DecimaPolicy.rollout_action_env` is the form with a Decima follower. Not available while a timeline is recorded (ValueError)."""
        B, dev = self.num_envs, self.device
        t = [self._i32_per_env(x, f"rollout_action: {what}") for x, what in ((policy, "policy"), (param, "param"), (first_stage, "first_stage"), (first_exec, "first_exec"))]
        if out is None:
            out = {"steps": torch.zeros(B, dtype=torch.int32, device=dev), "first_stage_idx": torch.full((B,), -1, dtype=torch.int32, device=dev),
                   "first_num_exec": torch.zeros(B, dtype=torch.int32, device=dev)}
        o = [self._i32_per_env(out[k], f"rollout_action: out[{k!r}]") for k in ("steps", "first_stage_idx", "first_num_exec")]
        self._b.check(self._b.lib.sss_rollout_action(self._h, None, 0, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), int(n_steps),
                                                     o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), self._stream()))
        return out

    def lookahead_pick(self, parents: torch.Tensor, children: torch.Tensor, cand: dict[str, torch.Tensor], best: torch.Tensor, scores: torch.Tensor,
                       env_policy: dict[str, torch.Tensor]) -> None:
        """the decision of a lookahead from its finished children, one asynchronous launch (include/sss.h sss_lookahead_pick, where
        cost, score and winner are defined): `parents` i32[P] env ids, `children` i32[P, K, S] env ids, `cand` the candidates'
        {"first_policy", "first_param", "policy", "param"} i32[K]; writes `best` i32[P] (-1: no valid candidate), `scores` f64[P, K]
        and the winner's four entries into `env_policy` (the same keys, i32[B]) at the parents' ids - the arguments of the
        `rollout_each` that steps the parents. All tensors on the env's device, contiguous; nothing is read back."""
        keys = ("first_policy", "first_param", "policy", "param")
        if children.dim() != 3 or children.shape[0] != parents.numel():
            raise ValueError(f"lookahead_pick: children must be [P, K, S] with P = {parents.numel()}, got {tuple(children.shape)}")
        P, K, S = (int(x) for x in children.shape)
        for name, t, dt, n in [("parents", parents, torch.int32, P), ("children", children, torch.int32, P * K * S), ("best", best, torch.int32, P),
                               ("scores", scores, torch.float64, P * K)] + [(f"cand[{k!r}]", cand[k], torch.int32, K) for k in keys]:
            if t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() != n:
                raise ValueError(f"lookahead_pick: {name} must be a contiguous {dt} tensor of {n} entries on {self.device}")
        e = [self._i32_per_env(env_policy[k], f"lookahead_pick: env_policy[{k!r}]") for k in keys]
        self._b.check(self._b.lib.sss_lookahead_pick(self._h, P, K, S, parents.data_ptr(), children.data_ptr(), *(cand[k].data_ptr() for k in keys),
                                                     best.data_ptr(), scores.data_ptr(), *(t.data_ptr() for t in e), self._stream()))

    def rollout_until(self, policy: torch.Tensor, param: torch.Tensor, horizon: float, max_steps: int, first_policy: torch.Tensor | None = None,
                      first_param: torch.Tensor | None = None, out: dict[str, torch.Tensor] | None = None) -> dict[str, torch.Tensor]:
        """`rollout_each` with a stop time (include/sss.h sss_rollout_until), one asynchronous launch and no host sync: env i takes
        steps under `policy[i]` / `param[i]` until its wall time has reached T = its wall time at entry + `horizon` (simulated time,
        > 0, `float("inf")` allowed; ValueError otherwise), its episode is over, or it has taken `max_steps` steps. Everything else
        is `rollout_each`'s: -1 sits out untouched, `first_policy` / `first_param`, `steps == -1` for a bad policy.
        Returns `rollout_each`'s dict plus `t_stop` (f64[B]: T, for every env that took part) and `rem_work` (f64[B, job_cap]: the
        work every active job of the state the env stopped in still holds - `schedulers.job_work` of its observation, bit for bit
        - and 0.0 for every other job). Fresh tensors (zeros) unless `out` - such a dict from an earlier call - is given."""
        B, dev = self.num_envs, self.device
        pol, par = self._i32_per_env(policy, "rollout_until: policy"), self._i32_per_env(param, "rollout_until: param")
        if (first_policy is None) != (first_param is None):
            raise ValueError("rollout_until: first_policy and first_param come together or not at all")
        fpol = self._i32_per_env(first_policy, "rollout_until: first_policy") if first_policy is not None else None
        fpar = self._i32_per_env(first_param, "rollout_until: first_param") if first_param is not None else None
        if out is None:
            out = {"steps": torch.zeros(B, dtype=torch.int32, device=dev), "first_stage_idx": torch.full((B,), -1, dtype=torch.int32, device=dev),
                   "first_num_exec": torch.zeros(B, dtype=torch.int32, device=dev), "t_stop": torch.zeros(B, dtype=torch.float64, device=dev),
                   "rem_work": torch.zeros((B, self.dims.job_cap), dtype=torch.float64, device=dev)}
        o = [self._i32_per_env(out[k], f"rollout_until: out[{k!r}]") for k in ("steps", "first_stage_idx", "first_num_exec")]
        for k, n in (("t_stop", B), ("rem_work", B * self.dims.job_cap)):
            t = out[k]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != dev or not t.is_contiguous() or t.numel() != n:
                raise ValueError(f"rollout_until: out[{k!r}] must be a contiguous float64 tensor of {n} entries on {dev}")
        self._b.check(self._b.lib.sss_rollout_until(self._h, pol.data_ptr(), par.data_ptr(), fpol.data_ptr() if fpol is not None else None,
                                                    fpar.data_ptr() if fpar is not None else None, float(horizon), int(max_steps), o[0].data_ptr(), o[1].data_ptr(),
                                                    o[2].data_ptr(), out["t_stop"].data_ptr(), out["rem_work"].data_ptr(), self._stream()))
        return out

    def lookahead_pick_horizon(self, parents: torch.Tensor, children: torch.Tensor, cand: dict[str, torch.Tensor], t_stop: torch.Tensor, rem_work: torch.Tensor,
                               tail: str, best: torch.Tensor, scores: torch.Tensor, env_policy: dict[str, torch.Tensor]) -> None:
        """`lookahead_pick` for children that stopped at a time horizon (include/sss.h sss_lookahead_pick_horizon, where validity
        and cost are defined; `evaluation.horizon_cost` restates the cost in Python floats): `t_stop` f64[B] and `rem_work`
        f64[B, job_cap] as `rollout_until` wrote them for the children, `tail` "none" or "srpt" (`binding.LOOKAHEAD_TAILS`);
        everything else as `lookahead_pick`. One asynchronous launch, nothing is read back."""
        from .binding import LOOKAHEAD_TAILS

        if tail not in LOOKAHEAD_TAILS:
            raise ValueError(f"lookahead_pick_horizon: tail must be one of {sorted(LOOKAHEAD_TAILS)}, got {tail!r}")
        keys = ("first_policy", "first_param", "policy", "param")
        if children.dim() != 3 or children.shape[0] != parents.numel():
            raise ValueError(f"lookahead_pick_horizon: children must be [P, K, S] with P = {parents.numel()}, got {tuple(children.shape)}")
        P, K, S = (int(x) for x in children.shape)
        for name, t, dt, n in [("parents", parents, torch.int32, P), ("children", children, torch.int32, P * K * S), ("best", best, torch.int32, P),
                               ("scores", scores, torch.float64, P * K), ("t_stop", t_stop, torch.float64, self.num_envs),
                               ("rem_work", rem_work, torch.float64, self.num_envs * self.dims.job_cap)] + [(f"cand[{k!r}]", cand[k], torch.int32, K) for k in keys]:
            if t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() != n:
                raise ValueError(f"lookahead_pick_horizon: {name} must be a contiguous {dt} tensor of {n} entries on {self.device}")
        e = [self._i32_per_env(env_policy[k], f"lookahead_pick_horizon: env_policy[{k!r}]") for k in keys]
        self._b.check(self._b.lib.sss_lookahead_pick_horizon(self._h, P, K, S, parents.data_ptr(), children.data_ptr(), *(cand[k].data_ptr() for k in keys),
                                                             t_stop.data_ptr(), rem_work.data_ptr(), LOOKAHEAD_TAILS[tail], best.data_ptr(), scores.data_ptr(),
                                                             *(t.data_ptr() for t in e), self._stream()))

    def decima_graph_on_device(self, active: torch.Tensor | None = None, num_tasks_scale: float = 200.0, work_scale: float = 1e5) -> dict[str, Any]:
        """`decima_graph` without the device->host round trip: the graph's totals (nodes, edges, jobs, schedulable nodes) stay on
        the device (`g["totals_dev"]`, i64[4]); every array is a buffer of the env at its CAPACITY (num_envs x node_cap nodes, ...),
        only its leading `totals_dev[k]` rows are meaningful, and the kernels downstream read the counts themselves
        (sss_gnn_args::n_rows_dev, sss_gnn_encode_args::n_nodes_dev). `g["totals_hint"]`: the previous call's totals, copied back
        without waiting (pinned memory) - grid sizes only. For act-and-forget inference (`DecimaPolicy.schedule_env`): the buffers are
        overwritten by the next call; graphs that are kept (rollout recording, training) use `decima_graph`."""
        B, dev, d = self.num_envs, self.device, self.dims
        assert self.graph_kernel_fits, "the graph kernel's LDS working set does not fit this node capacity"
        D = self.max_dag_depth
        ws = getattr(self, "_dg_dev", None)
        if ws is None:
            Mc, Ec, Jc = B * d.node_cap, B * d.edge_cap, B * d.job_cap
            # (zeros, not uninitialised memory: for an env without a schedulable stage the executor-score launch reads the row of job 0 -
            # `job_first`, `job_obs`, `job_cap` - and that row is not written when the very first graph built here has no job at all)
            e = lambda n, dt, *tail: torch.zeros((max(n, 1), *tail), dtype=dt, device=dev)  # noqa: E731
            ws = self._dg_dev = {
                "x": e(Mc, torch.float32, 5), "node_obs": e(Mc, torch.int64), "node_loc": e(Mc, torch.int64), "node_job": e(Mc, torch.int64),
                "sched_rank": e(Mc, torch.int64), "gen": e(Mc, torch.int32), "node_recv": e(Mc, torch.int32), "stage_mask": e(Mc, torch.bool),
                "src": e(Ec, torch.int64), "dst": e(Ec, torch.int64), "edge_obs": e(Ec, torch.int64), "edge_layers": e(Ec, torch.int32),
                "job_obs": e(Jc, torch.int64), "job_cap": e(Jc, torch.int64), "job_first": e(Jc, torch.int64), "obs_depth": e(B, torch.int32),
                "job_nodes": e(Jc, torch.int64), "out_start": e(Mc, torch.int64), "out_deg": e(Mc, torch.int32),
                "layer_cnt": e(32, torch.int32, B), "sched_list": e(Mc, torch.int64),
                "scan": e(2, torch.int64, 4, B),
                # two sets of list counters (i64[33][32] each: a counter per layer and block of envs + the blocks' largest observation) used in turn - a launch reserves on
                # one and clears the other - with the graph's four totals between them: [set 0 | totals | set 1], so that the totals and
                # the current set are one contiguous piece for the read-back of the grid-size hints
                "pp": torch.zeros(1056 + 4 + 1056, dtype=torch.int64, device=dev),
                "recv": e(Mc * max(D, 1), torch.int64), "hint": LateHint(1060, dev), "epoch": 0}
            ws["tot"] = ws["pp"][1056:1060]
        act8 = _mask_u8(active)
        scan, tot = ws["scan"], ws["tot"]
        stream = self._stream()
        mask_ptr = act8.data_ptr() if act8 is not None else None
        kept = ws.get("args")
        if kept is None or kept[0] != (num_tasks_scale, work_scale, self.obs_i32.data_ptr()):
            # the buffers are the env's own, the same at every call: the argument structure and the dict of views are made once
            # (building them cost more host time per step than the two launches), the mask pointer is written per call
            off, cnt_t = scan[0], scan[1]
            stride = ws["recv"].numel() // max(D, 1)
            a = SssDecimaGraph(mask_ptr, off[0].data_ptr(), off[2].data_ptr(), off[1].data_ptr(),
                               float(num_tasks_scale), float(work_scale), *(ws[k].data_ptr() for k in (
                                   "x", "node_obs", "node_loc", "node_job", "sched_rank", "gen", "node_recv", "stage_mask", "src", "dst",
                                   "edge_obs", "edge_layers", "job_obs", "job_cap", "job_first", "obs_depth", "job_nodes", "out_start", "out_deg", "layer_cnt")),
                               off[3].data_ptr(), ws["sched_list"].data_ptr(), None, ws["recv"].data_ptr(), stride, None, 33 * 32)
            g0 = {k: ws[k] for k in ("x", "node_obs", "node_loc", "node_job", "sched_rank", "gen", "node_recv", "stage_mask", "src", "dst", "edge_obs",
                                     "edge_layers", "job_obs", "job_cap", "job_first", "obs_depth", "job_nodes", "out_start", "out_deg", "layer_cnt", "sched_list")}
            g0["n_obs"], g0["n_pad"], g0["max_depth"] = B, d.node_cap, D
            g0["obs_nodes"], g0["obs_jobs"], g0["obs_node_off"], g0["obs_job_off"] = cnt_t[0], cnt_t[2], off[0], off[2]
            g0["totals_dev"], g0["_binding"] = tot, self._b
            ptrs = (self.obs_i32.data_ptr(), self.obs_i32.stride(0), scan[0].data_ptr(), scan[1].data_ptr(), tot.data_ptr())
            kept = ws["args"] = ((num_tasks_scale, work_scale, self.obs_i32.data_ptr()), a, g0, stride, off, ptrs)
        _, a, g0, stride, off, ptrs = kept
        a.active_dev = mask_ptr
        with device_of(dev):
            self._b.check(self._b.lib.sss_prefix_rows(ptrs[0], 1, ptrs[1], mask_ptr, 4, B, ptrs[2], ptrs[3], ptrs[4], stream))
            ws["epoch"] += 1
            par, pp = ws["epoch"] & 1, ws["pp"]
            sets = (pp[0:1056], pp[1060:2116])
            a.layer_totals_dev, a.layer_totals_clear_dev = sets[par].data_ptr(), sets[1 - par].data_ptr()
            self._b.check(self._b.lib.sss_decima_graph_build(self._h, C.byref(a), stream))
            g = dict(g0)
            g["layer_totals"] = sets[par]
            g["_layer_lists"] = ({"recv": ws["recv"], "stride": stride, "epoch": ws["epoch"]}, ws["epoch"])
            # the latest earlier call's numbers that have arrived: totals (M, Ed, J, S) and the lists' piece lengths (-1: none yet)
            hv, tag = ws["hint"].read_tagged()
            g["totals_hint"], g["layer_hint"] = (hv[:4], hv[:1056]) if tag is None else (hv[1056:1060], hv[:1056]) if tag == 0 else (hv[:4], hv[4:1060])
            ws["hint"].post(pp[0:1060] if par == 0 else pp[1056:2116], tag=par)
        g["_keepalive"] = (off, act8)
        return g

    @property
    def graph_kernel_fits(self) -> bool:
        """whether include/sss.h sss_decima_graph_build takes this env's capacities (its per-env LDS working set: 8 bytes per node
        slot + 8 per job slot; 16-bit node / edge slots; job templates of at most 24 DAG layers = longest path in edges) - else the
        graph comes from tensor ops"""
        d = self.dims
        return 8 * d.node_cap + 8 * (d.job_cap + 1) <= 65536 and d.node_cap <= 65535 and d.edge_cap <= 65535 and self.max_dag_depth <= 24

    def decima_graph(self, active: torch.Tensor | None = None, num_tasks_scale: float = 200.0, work_scale: float = 1e5,
                     reuse_buffers: bool = False) -> dict[str, Any]:
        """the current observations of all envs (or of those with `active[b]` True) as Decima's
        compact graph - `decima.compact_graph(decima.decima_observation(obs))` produced by ONE kernel
        (include/sss.h sss_decima_graph_build) instead of ~150 tensor ops, plus per-edge / per-node
        DAG-layer bits and each schedulable node's `stage_idx`. One device->host sync (totals).
        `reuse_buffers`: write into buffers kept by the env (views into them are returned and are
        overwritten by the next such call) - for act-and-forget inference loops; graphs that are
        kept (rollout recording) must use the default."""
        B, dev = self.num_envs, self.device
        if not self.graph_kernel_fits:
            # the kernel's per-node LDS working set does not fit: same graph from tensor ops on the device
            from .decima import compact_graph, decima_observation
            if not getattr(self, "_warned_graph_fallback", False):
                import warnings
                self._warned_graph_fallback = True
                warnings.warn(f"Decima graph kernel not usable for this env (node capacity {self.dims.node_cap}, edge capacity {self.dims.edge_cap}, "
                              f"deepest job template {self.max_dag_depth} DAG layers; limits: 8 B x nodes + 8 B x jobs <= 64 KB of LDS, 65535 slots, 24 layers): "
                              "observations are transformed by tensor ops instead (same results, several times slower per step)", RuntimeWarning, stacklevel=2)
            f = decima_observation(self._obs(), self.num_executors, self.dims.stage_stride, int(num_tasks_scale), work_scale)
            if active is not None:
                for k in ("node_valid", "job_valid", "edge_valid", "stage_mask"):
                    f[k] = f[k] & active[:, None]
                f["n_nodes"], f["depth"] = f["n_nodes"] * active, f["depth"] * active
            return compact_graph(f)
        # per-env counts (n_nodes, n_edges, n_jobs; 0 for inactive envs), their exclusive prefix sums and totals:
        # one small kernel over the obs_i32 rows in place (include/sss.h sss_prefix_rows) instead of a handful of
        # tensor ops; the totals are the one device->host sync
        act8 = _mask_u8(active)
        # (rows of the scan: n_nodes, n_edges, n_jobs, n_sched = columns 0..3 of obs_i32)
        scan = torch.empty((2, 4, B), dtype=torch.int64, device=dev)
        tot = torch.empty(4, dtype=torch.int64, device=dev)
        with device_of(dev):  # (sss_prefix_rows takes no handle: it launches on the CURRENT device)
            self._b.check(self._b.lib.sss_prefix_rows(self.obs_i32.data_ptr(), 1, self.obs_i32.stride(0), act8.data_ptr() if act8 is not None else None, 4, B,
                                                     scan[0].data_ptr(), scan[1].data_ptr(), tot.data_ptr(), self._stream()))
        off, cnt_t = scan[0], scan[1]  # [4, B] each
        M, Ed, J, S = (int(v) for v in tot.tolist())
        # buffers hold at least one element so that their pointers are never NULL; `g` gets exact views
        pool = self._dg_pool if reuse_buffers else None

        def mk(n, dt, *tail, _c=[0]):
            if pool is None:
                return torch.empty((max(n, 1), *tail), dtype=dt, device=dev)
            k = _c[0]
            _c[0] += 1
            t = pool.get(k)
            if t is None or t.shape[0] < max(n, 1) or t.dtype != dt:
                t = pool[k] = torch.empty((max(2 * n, 1024), *tail), dtype=dt, device=dev)  # grows geometrically
            return t[: max(n, 1)]
        buf = {"x": mk(M, torch.float32, 5), "node_obs": mk(M, torch.int64), "node_loc": mk(M, torch.int64), "node_job": mk(M, torch.int64),
               "sched_rank": mk(M, torch.int64), "gen": mk(M, torch.int32), "node_recv": mk(M, torch.int32), "stage_mask": mk(M, torch.bool),
               "src": mk(Ed, torch.int64), "dst": mk(Ed, torch.int64), "edge_obs": mk(Ed, torch.int64), "edge_layers": mk(Ed, torch.int32),
               "job_obs": mk(J, torch.int64), "job_cap": mk(J, torch.int64), "job_first": mk(J, torch.int64), "obs_depth": mk(B, torch.int32),
               "job_nodes": mk(J, torch.int64), "out_start": mk(M, torch.int64), "out_deg": mk(M, torch.int32),
               "layer_cnt": torch.empty((32, B), dtype=torch.int32, device=dev), "sched_list": mk(S, torch.int64)}
        size = {"x": M, "node_obs": M, "node_loc": M, "node_job": M, "sched_rank": M, "gen": M, "node_recv": M, "stage_mask": M,
                "src": Ed, "dst": Ed, "edge_obs": Ed, "edge_layers": Ed, "job_obs": J, "job_cap": J, "job_first": J, "obs_depth": B,
                "job_nodes": J, "out_start": M, "out_deg": M, "layer_cnt": 32, "sched_list": S}
        g = {k: v[: size[k]] for k, v in buf.items()}
        # the layers' lists of receiving nodes, written by the graph kernel itself into work space the env keeps per stream
        # (max_dag_depth lists of up to M ids; lengths in `layer_totals`): valid until the next decima_graph on this stream
        D = self.max_dag_depth
        skey = (dev, self._stream())
        ls = self._layer_scratch.get(skey)
        if ls is None or ls["recv"].numel() < max(M, 1) * max(D, 1):
            ls = self._layer_scratch[skey] = {"recv": torch.empty(max(2 * M, 1 << 14) * max(D, 1), dtype=torch.int64, device=dev), "epoch": 0}
        ls["epoch"] += 1
        ls["stride"] = ls["recv"].numel() // max(D, 1)
        layer_totals = torch.zeros(33 * 32, dtype=torch.int64, device=dev)  # (i64[33][32]: a counter per layer and block of envs, the blocks' largest observation)
        a = SssDecimaGraph(act8.data_ptr() if act8 is not None else None, off[0].data_ptr(), off[2].data_ptr(), off[1].data_ptr(),
                           float(num_tasks_scale), float(work_scale), *(buf[k].data_ptr() for k in (
                               "x", "node_obs", "node_loc", "node_job", "sched_rank", "gen", "node_recv", "stage_mask", "src", "dst",
                               "edge_obs", "edge_layers", "job_obs", "job_cap", "job_first", "obs_depth", "job_nodes", "out_start", "out_deg", "layer_cnt")),
                           off[3].data_ptr(), buf["sched_list"].data_ptr(), layer_totals.data_ptr(), ls["recv"].data_ptr(), ls["stride"], None, 33 * 32)
        self._b.check(self._b.lib.sss_decima_graph_build(self._h, C.byref(a), self._stream()))
        g["n_obs"], g["n_pad"] = B, self.dims.node_cap
        g["max_depth"] = self.max_dag_depth
        g["layer_totals"], g["_layer_lists"] = layer_totals, (ls, ls["epoch"])
        g["obs_nodes"], g["obs_jobs"] = cnt_t[0], cnt_t[2]
        g["obs_node_off"], g["obs_job_off"] = off[0], off[2]
        g["_keepalive"] = (off, act8)
        g["_binding"] = self._b
        return g

    @staticmethod
    def decima_layer_lists(g: dict[str, Any]) -> list[torch.Tensor]:
        """for every DAG layer of a graph from `decima_graph` the ids of the nodes it updates (one
        small kernel for all layers; one device->host sync for the list sizes)"""
        if "recv_lists" not in g:
            lc = g["layer_cnt"]  # i32[32, B]
            dev_l = lc.device
            scan = torch.empty((32, lc.shape[1]), dtype=torch.int64, device=dev_l)
            tot = torch.empty(32, dtype=torch.int64, device=dev_l)
            b = g["_binding"]
            stream = torch.cuda.current_stream(dev_l).cuda_stream if dev_l.type == "cuda" else 0
            with device_of(dev_l):
                b.check(b.lib.sss_prefix_rows(lc.data_ptr(), lc.stride(0), 1, None, 32, lc.shape[1], scan.data_ptr(), None, tot.data_ptr(), stream))
            totals = tot.tolist()
            n_layers = max((lvl + 1 for lvl, c in enumerate(totals) if c), default=0)
            base = [0] * 32
            for lvl in range(1, 32):
                base[lvl] = base[lvl - 1] + totals[lvl - 1]
            recv = torch.empty(max(sum(totals), 1), dtype=torch.int64, device=dev_l)
            if n_layers:
                env_off = scan  # exclusive prefix of the per-env receiver counts, per layer
                a = SssDecimaLists(g["obs_node_off"].data_ptr(), g["obs_nodes"].data_ptr(), g["node_recv"].data_ptr(), env_off.data_ptr(),
                                   (C.c_int64 * 32)(*base), recv.data_ptr(), n_layers)
                with device_of(dev_l):
                    b.check(b.lib.sss_decima_layer_lists(g["n_obs"], C.byref(a), stream))
                g["_keepalive_lists"] = env_off
            g["recv_lists"] = [recv[base[lvl]: base[lvl] + totals[lvl]] for lvl in range(n_layers)]
        return g["recv_lists"]

    def raise_on_error(self) -> None:
        """the reference raises from inside step(); the batched env records a per-env code. This
        turns recorded codes into the reference's exception types (one device->host sync)."""
        err = self.obs_i32[:, 7].cpu().numpy()
        bad = np.nonzero(err)[0]
        if bad.size:
            code = int(err[bad[0]])
            msg = f"env(s) {bad.tolist()[:8]}: {ERROR_NAMES.get(code, code)}"
            if code in (5, 7):
                raise AssertionError(msg)
            if code == 2:
                raise KeyError(msg)
            raise ValueError(msg)

    # ---- per-env views (host copies) for unmodified reference-style plugins ---------------

    def obs_view(self, i: int) -> dict[str, Any]:
        """the reference observation dict of env i (spark_sched_sim.py:393-399) as numpy/python
        objects - what `Scheduler.schedule(obs)` plugins written for the reference consume."""
        from .spaces import GraphInstance

        s = self.obs_i32[i].cpu().numpy()
        n, ne, a = int(s[0]), int(s[1]), int(s[2])
        nodes = self.nodes[i, :n].cpu().numpy()
        el = self.edge_links[i, :ne].cpu().numpy().astype(np.int64)
        return {
            "dag_batch": GraphInstance(nodes, np.zeros(ne, dtype=int), el),
            "dag_ptr": self.dag_ptr[i, : a + 1].cpu().tolist(),
            "num_committable_execs": int(s[4]),
            "source_job_idx": int(s[5]),
            "exec_supplies": self.exec_supplies[i, :a].cpu().tolist(),
        }

    def _hdr_i32(self, i: int, byte_off: int) -> int:
        return int(self._env_view[i, byte_off: byte_off + 4].cpu().numpy().view(np.int32)[0])

    def job_times(self, i: int):
        """(t_arrival f64[J], t_completed f64[J], completion_order i16[J], template id i16[J]) of env
        i's current episode (between launches the HBM copy of every record is current)"""
        d = self.dims
        row = self._env_view[i].cpu().numpy()
        hdr = row[: d.hdr_bytes]
        J = int(hdr[HDR_OFF["J"]: HDR_OFF["J"] + 4].view(np.int32)[0])
        ta = row[d.off_t_arrival: d.off_t_arrival + 8 * J].view(np.float64).copy()
        tc = row[d.off_t_completed: d.off_t_completed + 8 * J].view(np.float64).copy()
        jobs = row[d.off_jobs: d.off_jobs + d.job_rec_bytes * J].reshape(J, d.job_rec_bytes)
        order = jobs[:, 56:58].copy().view(np.int16).ravel()
        gs_base = jobs[:, 60:64].copy().view(np.int32).ravel()
        tmpl = np.searchsorted(workload.pack_section(self._pack, "tmpl_stage_off"), gs_base).astype(np.int16)
        return ta, tc, order, tmpl

    def job_duration_buff(self, i: int) -> list[float]:
        """env i's deque of the last 200 completed-job durations, oldest first (spark_sched_sim.py:121, 693-697)"""
        d = self.dims
        h = self.header(i)
        ring = self._env_view[i, d.off_dur_ring: d.off_dur_ring + 8 * 200].cpu().numpy().view(np.float64)
        return [float(ring[(h["dur_head"] + k) % 200]) for k in range(h["dur_n"])]

    def header(self, i: int) -> dict[str, Any]:
        hdr = self._env_view[i, : self.dims.hdr_bytes].cpu().numpy()
        out = {}
        for name, off in HDR_OFF.items():
            w = HDR_W[name]
            out[name] = hdr[off: off + np.dtype(w).itemsize].view(w)[0].item()
        return out

    def header_field(self, name: str) -> torch.Tensor:
        """device tensor [B] of one header scalar (zero-copy view of the arena)"""
        off, w = HDR_OFF[name], HDR_W[name]
        tw = {np.float64: torch.float64, np.uint64: torch.int64, np.int32: torch.int32, np.uint32: torch.int32}[w]
        n = np.dtype(w).itemsize
        return self._env_view[:, off: off + n].view(tw).squeeze(1)

    def rollout_stats(self) -> dict[str, torch.Tensor]:
        """what the reference's rollout workers report per env (rollout_worker.py:122-130:
        `avg_job_duration` [s, over the last <=200 completed jobs, nan if none], `avg_num_jobs`
        (metrics.py:16-18), `num_completed_jobs`, `num_job_arrivals`) for ALL envs as f64[B] device
        tensors - no per-env host round trips"""
        d, B = self.dims, self.num_envs
        J = d.job_cap
        f64 = lambda off, n: self._env_view[:, off: off + 8 * n].view(torch.float64)  # noqa: E731
        ta, tc = f64(d.off_t_arrival, J), f64(d.off_t_completed, J)
        wall = self.header_field("wall_time")
        arrived = torch.arange(J, device=self.device)[None, :] < self.header_field("next_arrival")[:, None]
        dur = torch.where(arrived, torch.minimum(tc, wall[:, None]) - ta, torch.zeros_like(ta))
        n_ring = self.header_field("dur_n").to(torch.float64)
        ring = f64(d.off_dur_ring, 200)
        head = self.header_field("dur_head").long()
        k = (torch.arange(200, device=self.device)[None, :] - head[:, None]) % 200  # position of slot in deque order
        ring_sum = torch.where(k < n_ring[:, None], ring, torch.zeros_like(ring)).sum(1)
        done, act = self.header_field("n_completed").to(torch.float64), self.header_field("n_active").to(torch.float64)
        return {"avg_job_duration": ring_sum / n_ring * 1e-3, "avg_num_jobs": dur.sum(1) / wall, "num_completed_jobs": done,
                "num_job_arrivals": done + act}

    def job_stats(self, q: Sequence[float] = (25, 50, 75, 100), active: torch.Tensor | None = None, want_sorted: bool = False) -> dict[str, torch.Tensor]:
        """the episode metrics of ALL envs from one kernel launch (include/sss.h sss_job_stats, where every column is defined), as
        device tensors and with no device->host transfer: `stats` f64[B, 8] - columns `binding.JOB_STATS_COLUMNS`: the number of
        arrived jobs, the sum and the mean of their durations (metrics.py:4-14), `avg_num_jobs` (:16-18), the mean duration of the
        last <= 200 completed jobs in seconds (spark_sched_sim.py:243-245), completed jobs, active jobs, wall time - `pct` f64[B, len(q)] =
        `numpy.percentile(durations, q)` and, with `want_sorted`, `sorted` f64[B, job_cap] (the sorted durations, NaN behind them).
        Every value carries the bits of the host functions of `metrics` on env i. `active` (bool / u8 [B]): rows of envs with 0 keep
        what they held. The percent tensor and the outputs are kept per `q` and overwritten by the next call with the same `q`."""
        from .binding import JOB_STATS_MAX_Q
        qs = tuple(float(x) for x in q)
        if len(qs) > JOB_STATS_MAX_Q:
            raise ValueError(f"job_stats: at most {JOB_STATS_MAX_Q} percent values, got {len(qs)}")
        if not all(0.0 <= x <= 100.0 for x in qs):  # (also refuses NaN)
            raise ValueError("job_stats: percentiles must be in the range [0, 100]")
        B, dev, nq = self.num_envs, self.device, len(qs)
        cache = self.__dict__.setdefault("_job_stats_ws", {})
        ws = cache.get(qs)
        if ws is None:
            ws = cache[qs] = {"q": torch.tensor(qs, dtype=torch.float64).to(dev) if nq else None,
                              "stats": torch.zeros((B, 8), dtype=torch.float64, device=dev),
                              "pct": torch.zeros((B, nq), dtype=torch.float64, device=dev)}
        if want_sorted and "sorted" not in ws:
            ws["sorted"] = torch.full((B, self.dims.job_cap), float("nan"), dtype=torch.float64, device=dev)
        act8 = _mask_u8(active)
        self._b.check(self._b.lib.sss_job_stats(self._h, nq, ws["q"].data_ptr() if nq else None, ws["stats"].data_ptr(), ws["pct"].data_ptr() if nq else None,
                                                ws["sorted"].data_ptr() if want_sorted else None, act8.data_ptr() if act8 is not None else None, self._stream()))
        out = {"stats": ws["stats"], "pct": ws["pct"]}
        if want_sorted:
            out["sorted"] = ws["sorted"]
        return out

    def counters(self) -> dict[str, int]:
        """lifetime totals over all envs: real step() calls, events popped, SURVEY 8(d) model bytes"""
        hdr = self._env_view[:, : self.dims.hdr_bytes].cpu().numpy()
        tot = {}
        for name in ("n_steps", "n_events", "model_bytes"):
            off = HDR_OFF[name]
            tot[name] = int(np.ascontiguousarray(hdr[:, off: off + 8]).view(np.uint64).sum())
        prof = np.ascontiguousarray(hdr[:, HDR_PROF: HDR_PROF + 40]).view(np.uint64).sum(axis=0)
        for k, name in enumerate(("ticks_slow_events", "ticks_action", "ticks_events", "ticks_reward", "ticks_observe")):
            tot[name] = int(prof[k])
        for name in ("n_fast", "n_batched", "n_rounds"):
            off = HDR_OFF[name]
            tot[name + "_events" if name != "n_rounds" else name] = int(np.ascontiguousarray(hdr[:, off: off + 8]).view(np.uint64).sum())
        return tot

    # ---- copies of running envs: fork, snapshot, restore (include/sss.h sss_env_copy) -----------

    @property
    def layout_id(self) -> int:
        """what two envs must share for an image to pass between them (include/sss.h sss_env_layout_id): every capacity and offset
        of an env's block and the kernel instantiation - not num_envs"""
        return int(self._b.lib.sss_env_layout_id(self._h))

    def _copy_ids(self, ids, what: str, limit: int) -> tuple[torch.Tensor, list[int] | None]:
        """ids for sss_env_copy as (i32 tensor on the device, the host's list or None). An int or a host sequence is checked against
        [0, limit); a tensor is passed through as it is - its values stay on the device, the kernel skips ids outside the store"""
        if isinstance(ids, torch.Tensor):
            return ids.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous(), None
        host = [int(ids)] if isinstance(ids, (int, np.integer)) else [int(x) for x in ids]
        bad = [x for x in host if not 0 <= x < limit]
        if bad:
            raise ValueError(f"{what}: id {bad[0]} is outside [0, {limit})")
        return torch.tensor(host, dtype=torch.int32).to(self.device), host

    @staticmethod
    def _check_pairs(src: list[int] | None, dst: list[int] | None, same_store: bool, what: str) -> None:
        if dst is not None and len(set(dst)) != len(dst):
            raise ValueError(f"{what}: destination ids must be distinct, got {dst}")
        if same_store and src is not None and dst is not None and set(src) & set(dst):
            raise ValueError(f"{what}: destination ids {sorted(set(src) & set(dst))} are also source ids")

    def _own_store(self):
        """this env's buffers as an sss_env_store (for a call on ANOTHER handle; on its own handle a NULL store says the same)"""
        from .binding import SssEnvStore
        tl = getattr(self, "_timeline", None)
        t, job, count = tl if tl is not None else (None, None, None)
        return SssEnvStore(self.state.data_ptr(), self.nodes.data_ptr(), self.edge_links.data_ptr(), self.dag_ptr.data_ptr(), self.exec_supplies.data_ptr(),
                           self.obs_i32.data_ptr(), self.obs_f64.data_ptr(), t.data_ptr() if tl else None, job.data_ptr() if tl else None,
                           count.data_ptr() if tl else None, t.shape[2] if tl else 0, self.num_envs, self.layout_id)

    def _env_copy(self, src_store, dst_store, src_ids: torch.Tensor, dst_ids: torch.Tensor, reseed: torch.Tensor | None) -> None:
        from .binding import SssEnvCopyArgs
        n = int(src_ids.numel())
        if int(dst_ids.numel()) != n or (reseed is not None and int(reseed.numel()) != n):
            raise ValueError(f"env copy: {n} source ids, {int(dst_ids.numel())} destination ids" + (f", {int(reseed.numel())} seeds" if reseed is not None else ""))
        a = SssEnvCopyArgs(C.pointer(src_store) if src_store is not None else None, C.pointer(dst_store) if dst_store is not None else None,
                           src_ids.data_ptr() if n else None, dst_ids.data_ptr() if n else None, reseed.data_ptr() if reseed is not None and n else None, n, 0)
        self._b.check(self._b.lib.sss_env_copy(self._h, C.byref(a), self._stream()))

    def _seed_tensor(self, reseed, n: int) -> torch.Tensor | None:
        """seeds in [0, 2^64) as the u64[n] array the kernel reads (an int64 tensor holding the same bits)"""
        if reseed is None:
            return None
        if isinstance(reseed, torch.Tensor):
            return reseed.reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
        vals = [int(reseed)] * n if isinstance(reseed, (int, np.integer)) else [int(x) for x in reseed]
        if any(not 0 <= v < 2 ** 64 for v in vals):
            raise ValueError("reseed: seeds must be in [0, 2**64)")
        return torch.from_numpy(np.asarray(vals, dtype=np.uint64).view(np.int64).copy()).to(self.device)

    def _mirrors(self):
        """the per-env arrays kept beside the arena: reset seeds, time limits, the bounded-step `ready` flags (None until first used)"""
        return (self._seeds, self._tl, getattr(self, "_ready", None))

    @staticmethod
    def _copy_mirrors(src, n_src: int, src_ids: torch.Tensor, dst, n_dst: int, dst_ids: torch.Tensor) -> None:
        """dst[k][dst_ids] = src[k][src_ids] for the pairs the kernel takes - both ids inside their stores - with device ops only
        (the ids may live on the device: a pair the kernel skips goes to a spare element instead of an index out of range)"""
        if not int(src_ids.numel()):
            return
        s, d = src_ids.long(), dst_ids.long()
        valid = (s >= 0) & (s < n_src) & (d >= 0) & (d < n_dst)
        s, d = s.clamp(0, n_src - 1), torch.where(valid, d, torch.full_like(d, n_dst))
        for a, b in zip(src, dst):
            if a is None or b is None:
                continue
            ext = torch.cat([b[:n_dst], b.new_zeros(1)])
            ext[d] = a.to(b.device)[s]
            b[:n_dst].copy_(ext[:n_dst])

    def fork(self, src, dst, reseed=None) -> None:
        """env dst[k] becomes a copy of env src[k] - the reference's `copy.deepcopy(env)` (everything spark_sched_sim.py:34-125 sets up,
        in whatever state the episode has brought it to, a step cut by `step_bounded_async` included) for every pair in one launch,
        asynchronous on the current stream. The copy continues exactly as the source would; with `reseed` (an int for all, or one
        per pair; numpy's `default_rng(seed)`) it keeps the job sequence - every arrival is drawn at reset - and draws its own task
        durations from there on. The destination keeps its own lifetime counters (`counters()` is unchanged), its observation rows
        and - when a timeline is recorded - its timeline rows become the source's.
        `src`, `dst`: an int, a sequence or a tensor of env ids. Host-side ids are checked - in range, `dst` distinct and disjoint from
        `src` (ValueError, nothing is written) - tensors are passed to the kernel without a sync: the rule is then the caller's duty,
        ids out of range are skipped. A copy's next episode under auto-reset follows the SOURCE's seed schedule (the episode's seed
        is part of the image)."""
        s_t, s_h = self._copy_ids(src, "fork: src", self.num_envs)
        d_t, d_h = self._copy_ids(dst, "fork: dst", self.num_envs)
        self._check_pairs(s_h, d_h, True, "fork")
        seeds = self._seed_tensor(reseed, int(s_t.numel()))
        self._env_copy(None, None, s_t, d_t, seeds)
        self._copy_mirrors(self._mirrors(), self.num_envs, s_t, self._mirrors(), self.num_envs, d_t)

    def snapshot(self, env_ids=None) -> "EnvSnapshot":
        """the images of `env_ids` (default: all envs) in tensors of their own: slot k holds env_ids[k] as it is now (asynchronous).
        `restore` brings them back - into this env or another one of the same layout."""
        ids, host = self._copy_ids(range(self.num_envs) if env_ids is None else env_ids, "snapshot: env_ids", self.num_envs)
        snap = EnvSnapshot(self, int(ids.numel()))
        slots = torch.arange(snap.num_slots, dtype=torch.int32, device=self.device)
        self._env_copy(None, snap._store(), ids, slots, None)
        self._copy_mirrors(self._mirrors(), self.num_envs, ids, (snap.seeds, snap.time_limits, snap.ready), snap.num_slots, slots)
        snap.env_ids = host
        return snap

    def restore(self, snap: "EnvSnapshot", env_ids=None, slots=None) -> None:
        """env env_ids[k] becomes the image in slot slots[k] of `snap` (defaults: every slot, into the envs it was taken from - or
        0 .. m - 1 when those are not known on the host). `snap` may come from another `VecSparkSchedSimEnv` of the same layout
        (`layout_id`: same env_cfg capacities and workload pack, any num_envs); another layout raises ValueError. Lifetime counters stay
        the env's own, as for `fork`. Timeline rows move only when the snapshot holds them AND this env records a timeline: a
        snapshot without them leaves this env's rows untouched (they then describe the env's previous state), and an env without
        a timeline ignores the snapshot's."""
        if snap.layout_id != self.layout_id:
            raise ValueError(f"restore: the snapshot was taken from another env layout (layout id {snap.layout_id}, this env's is {self.layout_id}); "
                             "images pass only between envs of the same capacities, workload pack and executor-count class")
        sl_t, sl_h = self._copy_ids(range(snap.num_slots) if slots is None else slots, "restore: slots", snap.num_slots)
        if env_ids is None:
            env_ids = [snap.env_ids[k] for k in sl_h] if snap.env_ids is not None and sl_h is not None and max(snap.env_ids, default=-1) < self.num_envs else range(int(sl_t.numel()))
        e_t, e_h = self._copy_ids(env_ids, "restore: env_ids", self.num_envs)
        self._check_pairs(None, e_h, False, "restore")
        self._env_copy(snap._store(), None, sl_t, e_t, None)
        self._copy_mirrors((snap.seeds, snap.time_limits, snap.ready), snap.num_slots, sl_t, self._mirrors(), self.num_envs, e_t)


class EnvSnapshot:
    """`num_slots` env images (`VecSparkSchedSimEnv.snapshot`) in tensors laid out as a store of include/sss.h sss_env_copy: blocks of
    a state arena, rows of the six observation buffers and - when the env recorded a timeline - of the three timeline arrays, plus the
    host-side mirrors of the envs (`seeds`, `time_limits`, the bounded-step `ready` flags) and the `layout_id` they belong to."""

    def __init__(self, env: VecSparkSchedSimEnv, m: int) -> None:
        d, dev, n = env.dims, env.device, max(int(m), 1)  # (at least one slot is allocated: no NULL pointers)
        self.num_slots, self.layout_id, self.device = int(m), env.layout_id, dev
        self._state_raw = torch.zeros(n * d.env_stride + 256, dtype=torch.uint8, device=dev)
        off = (-self._state_raw.data_ptr()) % 256
        self.state = self._state_raw[off: off + n * d.env_stride]
        self.nodes = torch.zeros((n, d.node_cap, NUM_NODE_FEATURES), dtype=torch.float32, device=dev)
        self.edge_links = torch.zeros((n, d.edge_cap, 2), dtype=torch.int32, device=dev)
        self.dag_ptr = torch.zeros((n, d.job_cap + 1), dtype=torch.int32, device=dev)
        self.exec_supplies = torch.zeros((n, d.job_cap), dtype=torch.int32, device=dev)
        self.obs_i32 = torch.zeros((n, d.obs_i32), dtype=torch.int32, device=dev)
        self.obs_f64 = torch.zeros((n, d.obs_f64), dtype=torch.float64, device=dev)
        self.timeline = None
        tl = getattr(env, "_timeline", None)
        if tl is not None:
            E, cap = env.num_executors, tl[0].shape[2]
            self.timeline = (torch.full((n, E, cap), float("nan"), dtype=torch.float64, device=dev), torch.full((n, E, cap), -1, dtype=torch.int32, device=dev),
                             torch.ones((n, E), dtype=torch.int32, device=dev))
        self.seeds = torch.zeros(n, dtype=torch.int64, device=dev)[: self.num_slots]
        self.time_limits = torch.full((n,), float("inf"), dtype=torch.float64, device=dev)[: self.num_slots]
        self.ready = torch.ones(n, dtype=torch.uint8, device=dev)[: self.num_slots]
        self.env_ids: list[int] | None = None

    def _store(self):
        from .binding import SssEnvStore
        tl = self.timeline
        return SssEnvStore(self.state.data_ptr(), self.nodes.data_ptr(), self.edge_links.data_ptr(), self.dag_ptr.data_ptr(), self.exec_supplies.data_ptr(),
                           self.obs_i32.data_ptr(), self.obs_f64.data_ptr(), tl[0].data_ptr() if tl else None, tl[1].data_ptr() if tl else None,
                           tl[2].data_ptr() if tl else None, tl[0].shape[2] if tl else 0, max(self.num_slots, 1), self.layout_id)

    @property
    def nbytes(self) -> int:
        """bytes of device memory the snapshot's tensors hold"""
        ts = [self._state_raw, self.nodes, self.edge_links, self.dag_ptr, self.exec_supplies, self.obs_i32, self.obs_f64, *(self.timeline or ())]
        return int(sum(t.numel() * t.element_size() for t in ts))


# byte offset of SssHot::ex_job (i16 per executor) inside an env's arena block, by the kernels' executor capacity (csrc/sss_layout.h:
# 64 up to 64 executors, 128 in the wide instantiation); pinned by tests/test_emu_timeline.py against the header compiled with g++
HOT_EX_JOB_OFF = {64: 320 + 64 * 16 + 64 * 4, 128: 320 + 128 * 16 + 128 * 4}
# byte offsets inside SssHdr (csrc/sss_layout.h); pinned by tests/test_abi.py against the header compiled with gcc
HDR_PROF = 208  # uint64 prof[5]: shader-clock ticks in slow-path handlers, action + fulfil, event loop, reward, observe
HDR_OFF = {"wall_time": 40, "time_limit": 48, "seed": 56, "n_steps": 64, "n_events": 72, "model_bytes": 80,
           "counter": 88, "next_arrival": 92, "J": 96, "n_active": 100, "n_completed": 104, "curr_source": 108,
           "n_sched": 112, "n_commits": 124, "terminated": 136, "err": 140, "need_reset": 144, "dur_head": 148, "dur_n": 152,
           "episodes": 156, "last_reward": 160, "ep_return": 168, "last_ep_return": 176, "last_ep_wall": 184,
           "ep_steps": 192, "last_ep_steps": 196, "next_arrival_t": 200, "n_fast": 248, "n_batched": 256, "n_rounds": 264,
           "err_line": 272}  # source line of the kernel-side check that failed last (diagnostics for bug reports)
HDR_W = {"wall_time": np.float64, "time_limit": np.float64, "seed": np.uint64, "n_steps": np.uint64,
         "n_events": np.uint64, "model_bytes": np.uint64, "counter": np.uint32, "next_arrival": np.int32,
         "J": np.int32, "n_active": np.int32, "n_completed": np.int32, "curr_source": np.uint32,
         "n_sched": np.int32, "n_commits": np.int32, "terminated": np.int32, "err": np.int32, "need_reset": np.int32,
         "dur_head": np.int32, "dur_n": np.int32, "episodes": np.int32, "last_reward": np.float64,
         "ep_return": np.float64, "last_ep_return": np.float64, "last_ep_wall": np.float64,
         "ep_steps": np.int32, "last_ep_steps": np.int32, "next_arrival_t": np.float64, "n_fast": np.uint64,
         "n_batched": np.uint64, "n_rounds": np.uint64, "err_line": np.uint64}
