"""A scheduler that looks ahead: at every decision it forks the env's state once per candidate, plays every copy to the end of the
episode on the device, and acts as the cheapest one says - the rollout / policy-switching construction (Bertsekas, Tsitsiklis & Wu,
"Rollout algorithms for combinatorial optimization", J. Heuristics 1997; Chang, Givan & Chong, "Parallel rollout for online solution
of partially observable Markov decision processes", DEDS 2004) over the heuristics the simulator has on the device. DESIGN.md 12
describes the construction, why costs are compared at the episode's end only, and its limits.

    env = VecSparkSchedSimEnv(cfg, 2 * (1 + 4), device="cuda:0")
    sched = LookaheadScheduler(env, parents=[0, 1], candidates=[("fair", 0), ("fifo", 0), ("sjfcp", 0), ("wfair", 1)])
    r = evaluation.run_lookahead(env, sched, seed=0)

One `decide_and_step()` is four kernel launches and no device->host read:
    1. `sss_env_copy`        every parent -> its K x S children (K candidates, S samples)
    2. `sss_rollout_each`    the children to the end of their episodes: candidate k's first step by candidate k, then by candidate k
                             again (policy switching, `base=None`) or by the base policy (the rollout algorithm, `base=(name, param)`)
    3. `sss_lookahead_pick`  total job time of every child, mean over a candidate's samples, arg-min -> the parents' policy entries
    4. `sss_rollout_each`    the parents take `replan_every` steps: the first by the winner, the rest by what the winner's children
                             played after their first step
With `reseed=None` a child continues the parent's own future exactly (same generator state), the system is deterministic and every
policy a function of the state: the best remaining cost never increases from one decision to the next, so the parent ends at or
below every candidate's own episode cost. With `reseed=int` sample s draws its own task durations - seed = a function of
(reseed, s, decision number), shared by the K candidates of a parent and by the parents (common random numbers) - and the choice is
a Monte-Carlo estimate without that guarantee.

`horizon=H` (simulated time, `float("inf")` allowed) bounds the children: launch 2 becomes `sss_rollout_until` - a child stops at the
first step boundary at or behind (the parent's wall time + H) - and launch 3 `sss_lookahead_pick_horizon`, which charges every
child for the jobs that arrived before that common time and, with `tail="srpt"`, adds an estimate of what the unfinished ones still
cost (include/sss.h). The cost of a decision then follows H, not the rest of the episode. A finite horizon is a
heuristic: the guarantee above does NOT carry over, the parent may end above a candidate's own episode.

`decima=<DecimaPolicy>` makes the learned scheduler one of the policies: `("decima", 0)` may then stand among `candidates` and as `base`
- "is my policy better than switching among the heuristics from this state", and the rollout algorithm over a learned base policy.
It is always the policy's ARG-MAX decision, a function of the state, so with `reseed=None` the guarantee above holds with Decima among
the candidates. Launches 2 and 4 are then `sss_rollout_decima` (`DecimaPolicy.rollout_env`: the same per-env arrays, policy id 5);
without a Decima candidate the launches are the ones listed above."""
from __future__ import annotations

from typing import Sequence

import torch

from .binding import LOOKAHEAD_TAILS, POLICY_DECIMA, POLICY_IDS

_KEYS = ("first_policy", "first_param", "policy", "param")
_GOLDEN = 0x9E3779B97F4A7C15
_LOG_ROWS = 1024  # decisions per block of the winners' log


def _signed64(x: int) -> int:
    x &= 2 ** 64 - 1
    return x - 2 ** 64 if x >= 2 ** 63 else x


class LookaheadScheduler:
    """`parents`: the env ids that are scheduled; `candidates`: [(policy name, param), ...] as `VecSparkSchedSimEnv.policy_actions`
    takes them; `base`: None = policy switching, (name, param) = the rollout algorithm over that base policy - it must be one of the
    candidates (then "do what the base does" is among the choices and the result is never worse than the base; ValueError otherwise);
    `samples` S and `reseed` as above; `replan_every`: steps a parent takes per decision; `max_steps`: bound of a child's steps (a
    child it cuts short is invalid and its candidate cannot win); `children`: the P x K x S env ids of the copies in [parent][candidate]
    [sample] order, default: the ids that follow the largest parent id. The env needs P * (1 + K * S) slots; a clash between
    parents and children, ids outside the env or too few slots raise ValueError. The env must not record a timeline.
    After a decision `last_best` (i32[P], -1: no candidate was valid - the parent then follows candidate 0) and `last_scores`
    (f64[P, K], NaN: a sample did not finish) are device tensors; `fallbacks` counts the (decision, parent) pairs with best == -1
    (one device->host read when asked).
    `horizon`: None = children play to the end of their episodes; a float > 0 (`float("inf")` included) = they stop that span of
    simulated time after the fork and are scored by `tail` ("srpt" or "none", `VecSparkSchedSimEnv.lookahead_pick_horizon`); a child
    that `max_steps` stops short of its horizon is invalid. `child_out` then also holds `t_stop` and `rem_work`. ValueError for a
    horizon that is <= 0 or NaN, or an unknown tail.
    `decima`: a `DecimaPolicy` for the env's executor count; with it the name "decima" (param ignored, arg-max decisions) is a policy
    like the others, as a candidate and as `base`. ValueError for "decima" without it, and for a Decima candidate together with
    `horizon` (there is no time-bounded Decima child)."""

    def __init__(self, env, parents: Sequence[int], candidates: Sequence[tuple[str, int]], base: tuple[str, int] | None = None, samples: int = 1,
                 reseed: int | None = None, replan_every: int = 1, max_steps: int = 200_000, children: Sequence[int] | None = None,
                 horizon: float | None = None, tail: str = "srpt", decima=None) -> None:
        self.env, self.decima = env, decima
        self.parents = [int(p) for p in parents]
        self.candidates = [(str(n), int(p)) for n, p in candidates]
        self.base = (str(base[0]), int(base[1])) if base is not None else None
        self.samples, self.replan_every, self.max_steps = int(samples), int(replan_every), int(max_steps)
        self.reseed = None if reseed is None else int(reseed)
        self.horizon, self.tail = (None if horizon is None else float(horizon)), str(tail)
        if self.horizon is not None and not self.horizon > 0:
            raise ValueError(f"LookaheadScheduler: horizon must be > 0 (float('inf') is allowed) or None, got {horizon}")
        if self.tail not in LOOKAHEAD_TAILS:
            raise ValueError(f"LookaheadScheduler: tail must be one of {sorted(LOOKAHEAD_TAILS)}, got {tail!r}")
        P, K, S, B, dev = len(self.parents), len(self.candidates), self.samples, env.num_envs, env.device
        if P < 1 or K < 1 or S < 1 or self.replan_every < 1 or self.max_steps < 1:
            raise ValueError("LookaheadScheduler: need at least one parent, one candidate, one sample, replan_every >= 1 and max_steps >= 1")
        if K * S > 1024:
            raise ValueError(f"LookaheadScheduler: candidates x samples must be at most 1024, got {K} x {S}")
        if self.reseed is not None and not 0 <= self.reseed < 2 ** 64:
            raise ValueError("LookaheadScheduler: reseed must be in [0, 2**64)")
        self._uses_decima = any(n == "decima" for n, _ in self.candidates + ([self.base] if self.base is not None else []))
        if self._uses_decima and decima is None:
            raise ValueError('LookaheadScheduler: the policy "decima" needs decima=<DecimaPolicy>')
        if self._uses_decima and self.horizon is not None:
            raise ValueError("LookaheadScheduler: a Decima candidate cannot be combined with a horizon (there is no time-bounded Decima child)")
        policy_id = lambda n, p: POLICY_DECIMA if n == "decima" else env._policy_id(n, p)  # noqa: E731
        ids = [(n, p, policy_id(n, p)) for n, p in self.candidates]  # (ValueError / KeyError for a name or alpha the env does not have)
        if self.base is not None and self.base not in self.candidates:
            raise ValueError(f"LookaheadScheduler: the base policy {self.base} must be one of the candidates {self.candidates}")
        if len(set(self.parents)) != P or any(not 0 <= p < B for p in self.parents):
            raise ValueError(f"LookaheadScheduler: parents must be distinct env ids in [0, {B}), got {self.parents}")
        if B < P * (1 + K * S):
            raise ValueError(f"LookaheadScheduler: {P} parents x (1 + {K} candidates x {S} samples) need {P * (1 + K * S)} envs, the env has {B}")
        if children is None:
            first = max(self.parents) + 1
            children = list(range(first, first + P * K * S))
        self.children = [int(c) for c in children]
        if len(self.children) != P * K * S:
            raise ValueError(f"LookaheadScheduler: need {P * K * S} children ({P} x {K} x {S}), got {len(self.children)}")
        if any(not 0 <= c < B for c in self.children):
            raise ValueError(f"LookaheadScheduler: not enough env slots behind the parents for {P * K * S} children (the env has {B}); pass `children`")
        if len(set(self.children)) != len(self.children) or set(self.children) & set(self.parents):
            raise ValueError("LookaheadScheduler: children must be distinct and disjoint from the parents")
        i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)  # noqa: E731
        base_id = (self.base[0], self.base[1], policy_id(*self.base)) if self.base is not None else None
        after = [base_id or c for c in ids]  # what candidate k's children play after their first step
        self._cand = {"first_policy": i32([c[2] for c in ids]), "first_param": i32([c[1] for c in ids]),
                      "policy": i32([c[2] for c in after]), "param": i32([c[1] for c in after])}
        self._parents = i32(self.parents)
        self._children = i32(self.children).reshape(P, K, S).contiguous()
        self._fork_src = i32([p for p in self.parents for _ in range(K * S)])
        self._fork_dst = self._children.reshape(-1)
        # the two launches' per-env policy arrays: the children's are fixed; the parents' are -1 until the pick kernel writes them
        kid = {k: [-1] * B for k in _KEYS}
        for n, c in enumerate(self.children):
            k = (n // S) % K
            kid["first_policy"][c], kid["first_param"][c], kid["policy"][c], kid["param"][c] = ids[k][2], ids[k][1], after[k][2], after[k][1]
        self._kid = {k: i32(v) for k, v in kid.items()}
        self._par = {k: torch.full((B,), -1, dtype=torch.int32, device=dev) for k in _KEYS}
        mk = lambda: {"steps": torch.zeros(B, dtype=torch.int32, device=dev), "first_stage_idx": torch.full((B,), -1, dtype=torch.int32, device=dev),  # noqa: E731
                      "first_num_exec": torch.zeros(B, dtype=torch.int32, device=dev)}
        self.child_out, self.parent_out = mk(), mk()  # what the two rollout launches of the last decision reported
        if self.horizon is not None:
            self.child_out["t_stop"] = torch.zeros(B, dtype=torch.float64, device=dev)
            self.child_out["rem_work"] = torch.zeros((B, env.dims.job_cap), dtype=torch.float64, device=dev)
        self.last_scores = torch.full((P, K), float("nan"), dtype=torch.float64, device=dev)
        self._seed_base = None
        if self.reseed is not None:  # seed(s, d) = reseed + (d * S + s) * GOLDEN mod 2^64 (`seed_for`), computed on the device
            s_of = torch.arange(S, dtype=torch.int64).repeat(P * K)  # sample index of fork pair n = (p * K + k) * S + s
            self._seed_base = (s_of * _signed64(_GOLDEN) + _signed64(self.reseed)).to(dev)
            self._seeds = torch.zeros(P * K * S, dtype=torch.int64, device=dev)
        self.reset()

    def reset(self) -> None:
        """forgets the decisions taken so far (the seeds of a reseeded lookahead start over): for a new episode of the parents"""
        P, dev = len(self.parents), self.env.device
        self.decisions = 0
        self._log = [torch.full((_LOG_ROWS, P), -1, dtype=torch.int32, device=dev)]
        self.last_best = self._log[0][0]
        for t in self._par.values():
            t.fill_(-1)

    def seed_for(self, sample: int, decision: int) -> int:
        """the generator seed of sample `sample`'s children at decision number `decision` (numpy's `default_rng(seed)`), the same
        for every candidate and every parent; None without `reseed`"""
        if self.reseed is None:
            return None
        return (self.reseed + (int(decision) * self.samples + int(sample)) * _GOLDEN) % 2 ** 64

    def _rollout_each(self, arrays: dict[str, torch.Tensor], n_steps: int, out: dict[str, torch.Tensor]) -> None:
        """the per-env fused rollout of launches 2 and 4: the kernel that knows Decima when a candidate needs it, else the heuristics' own"""
        if self._uses_decima:
            self.decima.rollout_env(self.env, n_steps, greedy=True, policy=arrays["policy"], param=arrays["param"], first_policy=arrays["first_policy"],
                                    first_param=arrays["first_param"], out=out)
        else:
            self.env.rollout_each(arrays["policy"], arrays["param"], n_steps, arrays["first_policy"], arrays["first_param"], out=out)

    def decide_and_step(self) -> None:
        """one decision for every parent and `replan_every` steps by it: four launches (five with `reseed`: one addition makes the
        decision's seeds), asynchronous, nothing is read back"""
        env, d = self.env, self.decisions
        seeds = None
        if self._seed_base is not None:
            seeds = torch.add(self._seed_base, _signed64(d * self.samples * _GOLDEN), out=self._seeds)
        env._env_copy(None, None, self._fork_src, self._fork_dst, seeds)
        if self.horizon is None:
            self._rollout_each(self._kid, self.max_steps, self.child_out)
        else:
            env.rollout_until(self._kid["policy"], self._kid["param"], self.horizon, self.max_steps, self._kid["first_policy"], self._kid["first_param"],
                              out=self.child_out)
        if d // _LOG_ROWS >= len(self._log):
            self._log.append(torch.full_like(self._log[0], -1))
        self.last_best = self._log[d // _LOG_ROWS][d % _LOG_ROWS]
        if self.horizon is None:
            env.lookahead_pick(self._parents, self._children, self._cand, self.last_best, self.last_scores, self._par)
        else:
            env.lookahead_pick_horizon(self._parents, self._children, self._cand, self.child_out["t_stop"], self.child_out["rem_work"], self.tail,
                                       self.last_best, self.last_scores, self._par)
        self._rollout_each(self._par, self.replan_every, self.parent_out)
        self.decisions = d + 1

    def winners(self) -> torch.Tensor:
        """the winner of every decision since `reset`, i32[decisions, P] on the device (-1: no valid candidate)"""
        return torch.cat(self._log)[: self.decisions]

    @property
    def fallbacks(self) -> int:
        return int((self.winners() == -1).sum())


class ActionLookaheadScheduler:
    """Lookahead over ACTIONS: at every decision the children of a parent take Decima's `k` best decisions of the parent's state -
    one each - and the base policy plays every child to the end of its episode; the parent takes the action whose children ended
    cheapest. This is the rollout algorithm proper (Bertsekas: branch over the actions of the state, follow the base policy from
    there), the policy-improvement step for the learned policy, where `LookaheadScheduler` branches over what other POLICIES would
    do first. DESIGN.md 12 ("Lookahead over actions") has the construction and its limits.

    `decima`: the `DecimaPolicy` whose arg-max top-`k` (`DecimaPolicy.topk_env`, 1 <= k <= 64) are the candidates; `base`: the
    policy that plays after the first step, any on-device policy name or "decima" (always its arg-max decision; the default);
    `parents`, `samples`, `reseed`, `replan_every`, `max_steps`, `children` (P x k x S ids in [parent][slot][sample] order) and the
    argument checks are `LookaheadScheduler`'s. One `decide_and_step()` is asynchronous and reads nothing back:
        1. `sss_env_copy`        every parent -> its k x S children (seeds as `LookaheadScheduler.seed_for`)
        2. `sss_decima_topk`     the parents' k best decisions (the other envs are inactive)
        3. a device scatter      slot r's action -> the children [p][r][.]
        4. `sss_rollout_action`  the children take their action, then the base policy to the end of their episodes; the children of
                                 an empty slot (fewer than k schedulable stages) sit out and are invalid in the pick
        5. `sss_lookahead_pick`  with all four candidate arrays set to the base policy; a parent without a valid slot takes slot 0
        6. a device gather       the winner's action -> the parents
        7. `sss_rollout_action`  the parents take it, then `replan_every - 1` steps of the base policy
    Slot 0 is the base policy's own decision when `base` is Decima: with `reseed=None` the best remaining cost then never increases
    from one decision to the next and the parent ends at or below Decima's own greedy episode. With another base, or with `reseed`,
    there is no such guarantee. There is NO `horizon` here: children always play to the end of their episodes (a time-bounded Decima
    child does not exist).
    After a decision: `last_best` i32[P] (-1: no valid slot), `last_scores` f64[P, k] (NaN: empty or unfinished), `last_actions` (the
    parents' top-k: {"stage_idx", "num_exec" i32[P, k], "lgprob" f32[P, k], "count" i32[P]}), `child_out`, `parent_out`, `winners()`
    and `fallbacks` as in `LookaheadScheduler`."""

    def __init__(self, env, parents: Sequence[int], decima, k: int, base: tuple[str, int] = ("decima", 0), samples: int = 1,
                 reseed: int | None = None, replan_every: int = 1, max_steps: int = 200_000, children: Sequence[int] | None = None) -> None:
        self.env, self.decima = env, decima
        self.parents = [int(p) for p in parents]
        self.k, self.base = int(k), (str(base[0]), int(base[1]))
        self.samples, self.replan_every, self.max_steps = int(samples), int(replan_every), int(max_steps)
        self.reseed = None if reseed is None else int(reseed)
        if decima is None:
            raise ValueError("ActionLookaheadScheduler: needs decima=<DecimaPolicy> (its top-k decisions are the candidates)")
        if not 1 <= self.k <= 64:
            raise ValueError(f"ActionLookaheadScheduler: k must be in [1, 64], got {k}")
        P, K, S, B, dev = len(self.parents), self.k, self.samples, env.num_envs, env.device
        if P < 1 or S < 1 or self.replan_every < 1 or self.max_steps < 1:
            raise ValueError("ActionLookaheadScheduler: need at least one parent, one sample, replan_every >= 1 and max_steps >= 1")
        if K * S > 1024:
            raise ValueError(f"ActionLookaheadScheduler: k x samples must be at most 1024, got {K} x {S}")
        if self.reseed is not None and not 0 <= self.reseed < 2 ** 64:
            raise ValueError("ActionLookaheadScheduler: reseed must be in [0, 2**64)")
        self._base_decima = self.base[0] == "decima"
        base_id = POLICY_DECIMA if self._base_decima else env._policy_id(*self.base)  # (ValueError / KeyError for a name or alpha the env does not have)
        if len(set(self.parents)) != P or any(not 0 <= p < B for p in self.parents):
            raise ValueError(f"ActionLookaheadScheduler: parents must be distinct env ids in [0, {B}), got {self.parents}")
        if B < P * (1 + K * S):
            raise ValueError(f"ActionLookaheadScheduler: {P} parents x (1 + {K} slots x {S} samples) need {P * (1 + K * S)} envs, the env has {B}")
        if children is None:
            first = max(self.parents) + 1
            children = list(range(first, first + P * K * S))
        self.children = [int(c) for c in children]
        if len(self.children) != P * K * S:
            raise ValueError(f"ActionLookaheadScheduler: need {P * K * S} children ({P} x {K} x {S}), got {len(self.children)}")
        if any(not 0 <= c < B for c in self.children):
            raise ValueError(f"ActionLookaheadScheduler: not enough env slots behind the parents for {P * K * S} children (the env has {B}); pass `children`")
        if len(set(self.children)) != len(self.children) or set(self.children) & set(self.parents):
            raise ValueError("ActionLookaheadScheduler: children must be distinct and disjoint from the parents")
        i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)  # noqa: E731
        # the pick kernel hands a candidate's four policy entries on: every slot's are the base policy's
        self._cand = {"first_policy": i32([base_id] * K), "first_param": i32([self.base[1]] * K), "policy": i32([base_id] * K), "param": i32([self.base[1]] * K)}
        self._parents = i32(self.parents)
        self._children = i32(self.children).reshape(P, K, S).contiguous()
        self._parents_l, self._children_l = self._parents.long(), self._children.reshape(-1).long()
        self._fork_src = i32([p for p in self.parents for _ in range(K * S)])
        self._fork_dst = self._children.reshape(-1)
        self._active = torch.zeros(B, dtype=torch.uint8, device=dev)
        self._active[self._parents_l] = 1
        # the two rollout launches' per-env arrays: policy / param are fixed for the children and written by the pick kernel for the
        # parents; the actions are scattered (children) and gathered (parents) at every decision. -1: the env sits out
        kid_pol, kid_par = [-1] * B, [-1] * B
        for c in self.children:
            kid_pol[c], kid_par[c] = base_id, self.base[1]
        self._kid = {"policy": i32(kid_pol), "param": i32(kid_par), "stage": torch.full((B,), -1, dtype=torch.int32, device=dev),
                     "exec": torch.full((B,), -1, dtype=torch.int32, device=dev)}
        self._par = {k_: torch.full((B,), -1, dtype=torch.int32, device=dev) for k_ in _KEYS}
        self._par_stage = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self._par_exec = torch.full((B,), -1, dtype=torch.int32, device=dev)
        mk = lambda: {"steps": torch.zeros(B, dtype=torch.int32, device=dev), "first_stage_idx": torch.full((B,), -1, dtype=torch.int32, device=dev),  # noqa: E731
                      "first_num_exec": torch.zeros(B, dtype=torch.int32, device=dev)}
        self.child_out, self.parent_out = mk(), mk()
        self._topk = None  # `topk_env`'s outputs over all envs, made by the first decision and written again by the later ones
        self.last_actions = None
        self.last_scores = torch.full((P, K), float("nan"), dtype=torch.float64, device=dev)
        self._seed_base = None
        if self.reseed is not None:  # as LookaheadScheduler: seed(s, d) = reseed + (d * S + s) * GOLDEN mod 2^64, computed on the device
            s_of = torch.arange(S, dtype=torch.int64).repeat(P * K)
            self._seed_base = (s_of * _signed64(_GOLDEN) + _signed64(self.reseed)).to(dev)
            self._seeds = torch.zeros(P * K * S, dtype=torch.int64, device=dev)
        self.reset()

    def reset(self) -> None:
        """forgets the decisions taken so far (the seeds of a reseeded lookahead start over): for a new episode of the parents"""
        P, dev = len(self.parents), self.env.device
        self.decisions = 0
        self._log = [torch.full((_LOG_ROWS, P), -1, dtype=torch.int32, device=dev)]
        self.last_best = self._log[0][0]
        for t in self._par.values():
            t.fill_(-1)

    def seed_for(self, sample: int, decision: int) -> int:
        """`LookaheadScheduler.seed_for`: the generator seed of sample `sample`'s children at decision `decision`; None without `reseed`"""
        if self.reseed is None:
            return None
        return (self.reseed + (int(decision) * self.samples + int(sample)) * _GOLDEN) % 2 ** 64

    def _rollout_action(self, policy: torch.Tensor, param: torch.Tensor, stage: torch.Tensor, nexec: torch.Tensor, n_steps: int, out: dict[str, torch.Tensor]) -> None:
        if self._base_decima:
            self.decima.rollout_action_env(self.env, n_steps, stage, nexec, greedy=True, policy=policy, param=param, out=out)
        else:
            self.env.rollout_action(policy, param, n_steps, stage, nexec, out=out)

    def decide_and_step(self) -> None:
        """one decision for every parent and `replan_every` steps by it; asynchronous, nothing is read back"""
        env, d = self.env, self.decisions
        P, K, S = len(self.parents), self.k, self.samples
        seeds = None
        if self._seed_base is not None:
            seeds = torch.add(self._seed_base, _signed64(d * S * _GOLDEN), out=self._seeds)
        env._env_copy(None, None, self._fork_src, self._fork_dst, seeds)
        self._topk = top = self.decima.topk_env(env, K, active=self._active, out=self._topk)
        act = {k_: top[k_].index_select(0, self._parents_l) for k_ in ("stage_idx", "num_exec", "lgprob", "count")}  # the parents' rows
        self.last_actions = act
        self._kid["stage"].index_copy_(0, self._children_l, act["stage_idx"][:, :, None].expand(P, K, S).reshape(-1))
        self._kid["exec"].index_copy_(0, self._children_l, act["num_exec"][:, :, None].expand(P, K, S).reshape(-1))
        self._rollout_action(self._kid["policy"], self._kid["param"], self._kid["stage"], self._kid["exec"], self.max_steps, self.child_out)
        if d // _LOG_ROWS >= len(self._log):
            self._log.append(torch.full_like(self._log[0], -1))
        self.last_best = self._log[d // _LOG_ROWS][d % _LOG_ROWS]
        env.lookahead_pick(self._parents, self._children, self._cand, self.last_best, self.last_scores, self._par)
        win = self.last_best.clamp(min=0).long()[:, None]  # (no valid slot: slot 0, which is always filled)
        self._par_stage.index_copy_(0, self._parents_l, act["stage_idx"].gather(1, win)[:, 0])
        self._par_exec.index_copy_(0, self._parents_l, act["num_exec"].gather(1, win)[:, 0])
        self._rollout_action(self._par["policy"], self._par["param"], self._par_stage, self._par_exec, self.replan_every, self.parent_out)
        self.decisions = d + 1

    def winners(self) -> torch.Tensor:
        """the winning slot of every decision since `reset`, i32[decisions, P] on the device (-1: no valid slot)"""
        return torch.cat(self._log)[: self.decisions]

    @property
    def fallbacks(self) -> int:
        return int((self.winners() == -1).sum())
