// sss_sim_action.h - part of the simulator device code (csrc/sss_sim.h includes it behind sss_sim_decima.h; not a stand-alone header):
// the per-env fused rollouts whose first step is a given ACTION instead of a policy's (include/sss.h sss_rollout_action) - "take
// action a in state s, then follow the policy", the Monte-Carlo form of Q(s, a), in one launch. What a lookahead over the ACTIONS of a
// state needs (spark_sched_sim_amd/lookahead.py ActionLookaheadScheduler: child [p][r] takes Decima's r-th best decision first).
//
// Per env they are sss_rollout_each_kernel (csrc/sss_sim_each.h) and the sss_rollout_decima kernels (csrc/sss_sim_decima.h) with the
// first-policy pair replaced by an action pair, first_stage_in / first_exec_in (i32[num_envs], both required):
//   - first_exec_in[env] >= 1: the first step takes (first_stage_in[env], first_exec_in[env]) verbatim - no policy is evaluated, do_step
//     gets the pair as sss_step's kernel hands it over. An action the env refuses leaves the env's error in its header, as there,
//     and ends the env's part in the launch (the refusals that do not ask for a reset would otherwise let the policy go on); that
//     step is not counted in steps. The step is it = 0 of Decima's draw counter: the follower's first decision draws with counter + 1;
//   - first_exec_in[env] == 0: no forced action, the env's policy decides the first step as well;
//   - first_exec_in[env] < 0: the env sits out untouched, byte for byte, like policy -1 (an empty top-K slot is handed over unread).
// Both entries are loaded before env_begin from addresses that depend on the workgroup id alone, like the policy entries.
// Everything else - policy -1, a bad id gives steps = -1, an env over at entry is not staged in, no auto-reset, the three outputs,
// Decima's hand-over arrays and LDS carving - is the two kernels'. Kernels of their own for the reason those are: the kernels that
// exist keep their code. No recording (-DSSS_TIMELINE) form: the host refuses the call while a timeline is bound.
#ifndef SSS_TIMELINE
// DECIMA: the policy table has id 5 and `d` is used; else the heuristics alone (`d` is not touched, no Decima LDS behind the pool)
template <bool DECIMA, bool ARGMAX>
SSS_DEV void rollout_action_env(const SssKernelArgs& a, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_stage_in,
                                const int32_t* first_exec_in, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec,
                                const SssDecimaPolicyArgs& d) {
  const int env = wave_env();
  // (everything up to env_begin is wave-uniform: loads from addresses that depend on the workgroup id alone)
  const int policy = policy_of ? policy_of[env] : (int)SSS_POLICY_DECIMA;  // no arrays (Decima form only): every env plays Decima
  if (policy == -1) return;
  const int forced_ne = first_exec_in[env], forced_si = first_stage_in[env];
  if (forced_ne < 0) return;
  const int param = policy_of ? param_of[env] : 0;
  if (!(DECIMA ? decima_rollout_policy_ok(policy, param) : each_policy_ok(policy, param))) {
    if (steps && wave_lane() == 0) steps[env] = -1;
    return;
  }
  uint8_t* base = (uint8_t*)a.B.state + (size_t)env * a.L.env_stride;
  const SssHdr* hdr = &((const SssHot*)base)->h;
  if (n_steps <= 0 || hdr->terminated || hdr->need_reset) {
    if (steps && wave_lane() == 0) steps[env] = 0;
    return;
  }
  uint8_t* const dp_lds = g_pool + ((a.P.pool_bytes + 15) & ~15);  // behind the simulator's pool (Decima form)
  ctx_init();
  env_begin(base);
  int taken = 0;
  for (int it = 0; it < n_steps; it++) {
    if (wave_ballot(g_hot.h.terminated || g_hot.h.need_reset) != 0) break;  // the episode's end or an env error: the env stays as it is
    const bool forced = it == 0 && forced_ne >= 1;  // wave-uniform
    int si, ne;
    if (forced) {
      si = forced_si, ne = forced_ne;
    } else if (DECIMA && policy == SSS_POLICY_DECIMA) {  // wave-uniform
      SssDecimaPolicyArgs ds = d;
      ds.rng_counter = d.rng_counter + (uint64_t)it;
      decima_policy_wave<ARGMAX>(a.L, a.B, a.L.E, ds, env, dp_lds);
      wave_sync();  // lane 0 wrote the decision
      si = (int)wave_bcast_u32((uint32_t)d.stage_idx[env], 0), ne = (int)wave_bcast_u32((uint32_t)d.num_exec[env], 0);
    } else {
      run_policy<true>(policy, param, si, ne);
    }
    if (it == 0 && wave_lane() == 0) {
      if (first_stage) first_stage[env] = si;
      if (first_exec) first_exec[env] = ne;
    }
    const double reward = do_step<true>(si, ne);
    write_observation(a.L, a.B, env, reward);
    wave_sync();  // ... and the next Decima step reads these rows
    if (forced && wave_ballot(g_hot.h.err != 0) != 0) break;  // the env refused the action: it keeps that error, as after sss_step
    taken++;
  }
  env_end(base);
  prof3_flush();
  if (steps && wave_lane() == 0) steps[env] = taken;
}

SSS_KERNEL void SSS_KNAME(sss_rollout_action_kernel)(SssKernelArgs a, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_stage_in,
                                                     const int32_t* first_exec_in, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec) {
  rollout_action_env<false, true>(a, policy_of, param_of, first_stage_in, first_exec_in, n_steps, steps, first_stage, first_exec, SssDecimaPolicyArgs());
}
// (one wave per SIMD and the full register file, as the sss_rollout_decima kernels; on the emulator SSS_KERNEL is extern "C")
#ifdef __HIP__
#define SSS_DECIMA_ACTION_KERNEL extern "C" __global__ __launch_bounds__(64, 1)
#else
#define SSS_DECIMA_ACTION_KERNEL SSS_KERNEL
#endif
SSS_DECIMA_ACTION_KERNEL void SSS_KNAME(sss_rollout_action_decima_kernel)(SssKernelArgs a, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_stage_in,
                                                                          const int32_t* first_exec_in, int n_steps, int32_t* steps, int32_t* first_stage,
                                                                          int32_t* first_exec, SssDecimaPolicyArgs d) {
  rollout_action_env<true, false>(a, policy_of, param_of, first_stage_in, first_exec_in, n_steps, steps, first_stage, first_exec, d);
}
SSS_DECIMA_ACTION_KERNEL void SSS_KNAME(sss_rollout_action_decima_argmax_kernel)(SssKernelArgs a, const int32_t* policy_of, const int32_t* param_of,
                                                                                 const int32_t* first_stage_in, const int32_t* first_exec_in, int n_steps, int32_t* steps,
                                                                                 int32_t* first_stage, int32_t* first_exec, SssDecimaPolicyArgs d) {
  rollout_action_env<true, true>(a, policy_of, param_of, first_stage_in, first_exec_in, n_steps, steps, first_stage, first_exec, d);
}
#undef SSS_DECIMA_ACTION_KERNEL

#ifndef __HIP__
#ifdef SSS_WIDE
#define SSS_ACTION_LAUNCHER sss_wide_launch_rollout_action
#else
#define SSS_ACTION_LAUNCHER sss_narrow_launch_rollout_action
#endif
// the CPU wave emulator's launcher, as in csrc/sss_sim_decima.h; the gfx950 ones are in csrc/sss_hip_sim.hip and csrc/sss_hip_wide.hip.
// d == nullptr: the heuristic kernel; else greedy picks the Decima kernel
int SSS_ACTION_LAUNCHER(const SssKernelArgs& a, int num_envs, int greedy, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_stage_in,
                        const int32_t* first_exec_in, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, const SssDecimaPolicyArgs* d, void*) {
  if (d && decima_rollout_pool_bytes(a) > (int)sizeof(g_pool)) return -1;
  emu::g_kernargs = &a;
  emu::launch(num_envs, [&]() {
    if (!d) SSS_KNAME(sss_rollout_action_kernel)(a, policy_of, param_of, first_stage_in, first_exec_in, n_steps, steps, first_stage, first_exec);
    else if (greedy) SSS_KNAME(sss_rollout_action_decima_argmax_kernel)(a, policy_of, param_of, first_stage_in, first_exec_in, n_steps, steps, first_stage, first_exec, *d);
    else SSS_KNAME(sss_rollout_action_decima_kernel)(a, policy_of, param_of, first_stage_in, first_exec_in, n_steps, steps, first_stage, first_exec, *d);
  });
  return 0;
}
#undef SSS_ACTION_LAUNCHER
#endif
#endif
