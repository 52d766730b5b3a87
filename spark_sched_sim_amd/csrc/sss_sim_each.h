// sss_sim_each.h - part of the simulator device code (csrc/sss_sim.h includes it behind the fused rollout kernels; not a stand-alone
// header): the fused rollout with a policy PER ENV (include/sss.h sss_rollout_each) - what a lookahead needs of the fused kernel:
// children of one parent under different policies in one launch, parents that sit it out, and a first step that may follow another
// policy than the rest ("child k: first step by candidate k, the base policy after"; spark_sched_sim_amd/lookahead.py).
//
// Per step it is ROLLOUT_BODY's `run_policy -> do_step<true> -> write_observation`, so an env goes through the states and outputs it
// goes through under sss_policy + sss_step, bit for bit. What differs from sss_rollout_kernel:
//   - the policy and its parameter come from per-env arrays. The env's identity is the workgroup id throughout the simulator
//     (ctx_make, tl_append read wave_env()), so the grid stays num_envs; an env with policy -1 costs one wave that returns at once
//     and is not touched at all - state, observation rows, outputs, counters (what SSS_SKIP_ENV is to sss_step);
//   - an id outside the policy table, or a weighted-fair exponent outside [-4, 4], cannot be refused by the host without reading
//     the arrays back: the env is left untouched as well and steps[env] = -1 says so;
//   - no auto-reset: an env stops at the end of its episode or at an env error, an env that is over at entry takes no step and is
//     not staged in (no byte of it is written);
//   - the number of steps taken and the action of the first one are reported per env.
// A kernel of its own with every policy inlined (run_policy<true>), for the reason sss_rollout_heur_kernel is one: the kernels
// tests/test_abi.py holds to their register budgets keep the code they had. There is no recording (-DSSS_TIMELINE) form: the host
// refuses the call while a timeline is bound.
#ifndef SSS_TIMELINE
SSS_DEV bool each_policy_ok(int policy, int param) {
  if (policy < SSS_POLICY_FAIR || policy > SSS_POLICY_SJFCP) return false;
  return !(policy == SSS_POLICY_WFAIR && (param < -4 || param > 4));
}

SSS_KERNEL void SSS_KNAME(sss_rollout_each_kernel)(SssKernelArgs a, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                                   const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec) {
  const int env = wave_env();
  // (everything up to env_begin is wave-uniform: loads from addresses that depend on the workgroup id alone)
  const int policy = policy_of[env];
  if (policy == -1) return;
  const int param = param_of[env];
  int pol = policy, par = param;  // of the next step: the first step's, then the env's
  if (first_policy_of && first_policy_of[env] >= 0) pol = first_policy_of[env], par = first_param_of[env];
  if (!each_policy_ok(policy, param) || !each_policy_ok(pol, par)) {
    if (steps && wave_lane() == 0) steps[env] = -1;
    return;
  }
  uint8_t* base = (uint8_t*)a.B.state + (size_t)env * a.L.env_stride;
  const SssHdr* hdr = &((const SssHot*)base)->h;
  if (n_steps <= 0 || hdr->terminated || hdr->need_reset) {
    if (steps && wave_lane() == 0) steps[env] = 0;
    return;
  }
  ctx_init();
  env_begin(base);
  int taken = 0;
  for (int it = 0; it < n_steps; it++) {
    if (wave_ballot(g_hot.h.terminated || g_hot.h.need_reset) != 0) break;  // the episode's end or an env error: the env stays as it is
    int si, ne;
    run_policy<true>(pol, par, si, ne);
    if (it == 0 && wave_lane() == 0) {
      if (first_stage) first_stage[env] = si;
      if (first_exec) first_exec[env] = ne;
    }
    const double reward = do_step<true>(si, ne);
    write_observation(a.L, a.B, env, reward);
    wave_sync();
    pol = policy, par = param;
    taken++;
  }
  env_end(base);
  prof3_flush();
  if (steps && wave_lane() == 0) steps[env] = taken;
}

#ifndef __HIP__
// the CPU wave emulator's launchers (tests/emu: both of its translation units include sss_sim.h behind their wave_rt.h, which
// declares emu::launch and emu::g_kernargs); the gfx950 ones are in csrc/sss_hip_sim.hip and csrc/sss_hip_wide.hip
#ifdef SSS_WIDE
#include "sss_wide.h"
#define SSS_EACH_LAUNCHER sss_wide_launch_rollout_each
#else
#include "sss_narrow.h"
#define SSS_EACH_LAUNCHER sss_narrow_launch_rollout_each
#endif
int SSS_EACH_LAUNCHER(const SssKernelArgs& a, int num_envs, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                      const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, void*) {
  emu::g_kernargs = &a;
  emu::launch(num_envs, [&]() { SSS_KNAME(sss_rollout_each_kernel)(a, policy_of, param_of, first_policy_of, first_param_of, n_steps, steps, first_stage, first_exec); });
  return 0;
}
#undef SSS_EACH_LAUNCHER
#endif
#endif
