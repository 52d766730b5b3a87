"""`SparkSchedSimEnv`: the reference's single-environment Gymnasium API (reference
spark_sched_sim/spark_sched_sim.py:29-245) as a facade over a 1-env `VecSparkSchedSimEnv`, i.e.
over the same HIP kernels. `reset`/`step` return the reference's observation dict, rewards and
flags, and raise the reference's exceptions, so harnesses like `examples.run_episode`
(reference examples.py:84-102) and `Scheduler.schedule(obs)` plugins work unchanged.

If gymnasium is importable the class derives from `gymnasium.Env` and is registered under the
reference's id "SparkSchedSimEnv-v0"; gymnasium itself is optional.
"""
from __future__ import annotations

from typing import Any

import numpy as np
import torch

from .binding import ERROR_NAMES
from .vec_env import VecSparkSchedSimEnv

try:  # pragma: no cover
    import gymnasium as _gym

    _Base = _gym.Env
except Exception:  # gymnasium is not installed in the target image
    _gym = None
    _Base = object


class JobView:
    """what reference metrics / trainers read from `env.jobs[j]` (metrics.py:6-9)"""

    def __init__(self, t_arrival: float, t_completed: float):
        self.t_arrival = t_arrival
        self.t_completed = t_completed


class ExecutorView:
    """what the reference's renderer reads from `env.executors[i]` (spark_sched_sim.py:408-411): `id_` and `history`, the list
    of [t, job_id] pairs of components/executor.py:21-44 (read from the device when asked for)"""

    def __init__(self, env: "SparkSchedSimEnv", id_: int):
        self._env = env
        self.id_ = id_

    @property
    def history(self) -> list[list]:
        return self._env._histories()[self.id_]


class SparkSchedSimEnv(_Base):  # type: ignore[misc]
    metadata = {"render_modes": ["rgb_array"], "render_fps": 30}
    RENDER_SIZE = (400, 300)  # width, height of an "rgb_array" frame
    TIMELINE_CAP = 512        # history entries kept per executor (whole episodes of the usual configurations need ~100)

    def __init__(self, env_cfg: dict[str, Any], device: str = "cuda:0", _lib=None, record_history: bool = True, pack: bytes | None = None) -> None:
        """`record_history=False` (not with a render mode): `Executor.history` is not kept - the env then runs the kernels
        without recording and allocates no timeline rows; `executors[i].history` raises. `pack`: a workload pack other than the default"""
        render_mode = env_cfg.get("render_mode")
        if render_mode and render_mode != "rgb_array":
            raise ValueError("rendering is not available in the GPU build")  # the pygame window ("human") is out of scope
        self.num_executors: int = env_cfg["num_executors"]
        self.moving_delay = env_cfg["moving_delay"]
        self.beta: float = env_cfg.get("beta", 0)
        self.job_arrival_cap = env_cfg.get("job_arrival_cap")
        self.render_mode = render_mode or None
        from .spaces import make_action_space, make_observation_space
        self.action_space = make_action_space(self.num_executors)
        self.observation_space = make_observation_space(self.num_executors)
        self._vec = VecSparkSchedSimEnv({k: v for k, v in env_cfg.items() if k != "render_mode"}, 1, device=device, _lib=_lib, pack=pack)
        self._ctor = (dict(env_cfg), _lib, bool(record_history))  # what __deepcopy__ builds the copy from
        if render_mode and not record_history:
            raise ValueError("render_mode needs record_history=True")
        if record_history:  # Executor.history is kept unless the caller opts out, as in the reference
            self._vec.enable_timeline(self.TIMELINE_CAP)
        self._hist_cache = None  # the histories as last fetched; a reset / step drops them
        self.executors = [ExecutorView(self, i) for i in range(self.num_executors)]
        self._act_s = torch.zeros(1, dtype=torch.int32, device=self._vec.device)
        self._act_n = torch.ones(1, dtype=torch.int32, device=self._vec.device)

    # ---- Gymnasium API ------------------------------------------------------------------

    def reset(self, seed: int | None = None, options: dict[str, Any] | None = None):
        time_limit = (options or {}).get("time_limit", np.inf)
        if time_limit is np.inf and not self.job_arrival_cap:
            raise ValueError("must either have a limit on job arrivals or time.")
        self._hist_cache = None
        self._vec.reset(seed=None if seed is None else [seed], options=options)
        self._raise()
        self.job_arrival_cap = self._vec.header(0)["J"]  # reference overwrites it (spark_sched_sim.py:156)
        self.observation_space["source_job_idx"].n = self.job_arrival_cap + 1  # :157
        return self._observe(), self.info

    def step(self, action: dict):
        if not isinstance(action, dict) or set(action.keys()) != {"stage_idx", "num_exec"}:
            raise ValueError("invalid action: does not belong to the action space")
        for v in action.values():
            if not isinstance(v, (int, np.integer)):
                raise ValueError("invalid action: does not belong to the action space")
        self._act_s[0] = int(action["stage_idx"])
        self._act_n[0] = int(action["num_exec"])
        self._hist_cache = None
        self._vec.step_async(self._act_s, self._act_n)
        self._raise()
        o = self._vec.obs_i32[0].cpu().numpy()
        reward = self._vec.obs_f64[0, 0].item()
        return self._observe(), reward, bool(o[6]), False, self.info

    def __deepcopy__(self, memo) -> "SparkSchedSimEnv":
        """the reference's `copy.deepcopy(env)`, also in the middle of an episode: a new env of the same configuration, workload
        pack and device that holds this env's image (VecSparkSchedSimEnv.snapshot / restore: state, observation, executor
        histories) and the Python-side fields this facade keeps current. The two step independently from here on."""
        env_cfg, lib, record_history = self._ctor
        new = type(self)(env_cfg, device=str(self._vec.device), _lib=lib, record_history=record_history, pack=self._vec._pack)
        new._vec.restore(self._vec.snapshot([0]), [0])
        new.job_arrival_cap, new.render_mode = self.job_arrival_cap, self.render_mode
        new.observation_space["source_job_idx"].n = self.observation_space["source_job_idx"].n
        new.action_space["stage_idx"].n = self.action_space["stage_idx"].n
        new.observation_space["dag_ptr"].feature_space.n = self.observation_space["dag_ptr"].feature_space.n
        memo[id(self)] = new
        return new

    def _observe(self) -> dict:
        obs = self._vec.obs_view(0)
        self.action_space["stage_idx"].n = len(obs["dag_batch"].nodes) + 1  # spark_sched_sim.py:403-404
        self.observation_space["dag_ptr"].feature_space.n = len(obs["dag_batch"].nodes) + 1
        return obs

    def _histories(self) -> list[list[list]]:
        """every executor's history, fetched from the device once per step: `[e.history for e in env.executors]`
        (spark_sched_sim.py:411) is one copy, not one per executor"""
        if self._hist_cache is None:
            self._hist_cache = self._vec.timeline(0)
        return self._hist_cache

    def render(self):
        """an H x W x 3 uint8 frame of the executors' Gantt chart (render_mode "rgb_array"; VecSparkSchedSimEnv.render), else None"""
        if self.render_mode != "rgb_array":
            return None
        w, h = self.RENDER_SIZE
        return self._vec.render([0], width=w, height=h)[0].cpu().numpy()

    def close(self) -> None:
        self._vec.close()

    def _raise(self) -> None:
        code = int(self._vec.obs_i32[0, 7].item())
        if code == 0:
            return
        msg = ERROR_NAMES.get(code, str(code))
        if code in (5, 7):
            raise AssertionError(msg)
        if code == 2:
            raise KeyError(msg)
        raise ValueError(msg)

    # ---- attributes the reference's callers read ----------------------------------------------

    @property
    def unwrapped(self):
        return self

    @property
    def wall_time(self) -> float:
        return self._vec.header(0)["wall_time"]

    @property
    def info(self) -> dict:
        return {"wall_time": self.wall_time}

    @property
    def jobs(self) -> dict[int, JobView]:
        ta, tc, _, _ = self._vec.job_times(0)
        return {j: JobView(float(ta[j]), float(tc[j])) for j in range(len(ta))}

    @property
    def active_job_ids(self) -> list[int]:
        d = self._vec.dims
        n = self._vec.header(0)["n_active"]
        row = self._vec._env_view[0, d.off_active: d.off_active + 2 * n].cpu().numpy()
        return row.view(np.uint16).astype(int).tolist()

    @property
    def completed_job_ids(self) -> set[int]:
        _, _, order, _ = self._vec.job_times(0)
        done = [(int(o), j) for j, o in enumerate(order) if o >= 0]
        s: set[int] = set()
        for _, j in sorted(done):  # same insertion order as the reference's set (spark_sched_sim.py:695)
            s.add(j)
        return s

    @property
    def num_completed_jobs(self) -> int:
        return self._vec.header(0)["n_completed"]

    @property
    def num_active_jobs(self) -> int:
        return self._vec.header(0)["n_active"]

    @property
    def all_jobs_complete(self) -> bool:
        h = self._vec.header(0)
        return h["n_completed"] == h["J"]

    @property
    def job_duration_buff(self) -> list[float]:
        return self._vec.job_duration_buff(0)

    @property
    def avg_job_duration(self) -> float:
        return np.mean(self.job_duration_buff).item() * 1e-3  # spark_sched_sim.py:243-245


if _gym is not None:  # pragma: no cover
    try:
        from gymnasium.envs.registration import register

        register(id="SparkSchedSimEnv-v0", entry_point="spark_sched_sim_amd.env:SparkSchedSimEnv")
    except Exception:
        pass
