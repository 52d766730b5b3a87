// sss_sim_until.h - part of the simulator device code (csrc/sss_sim.h includes it behind sss_sim_each.h; not a stand-alone header):
// the per-env fused rollout with a STOP TIME (include/sss.h sss_rollout_until) - what a lookahead with a horizon needs of the fused
// kernel: a child stops a fixed span of simulated time after the fork instead of at the end of its episode, and says how much work
// the state it stopped in still holds, so that a cost kernel (csrc/sss_lookahead.h, the horizon pick) can estimate the rest.
//
// Per env it is sss_rollout_each_kernel (csrc/sss_sim_each.h: policy -1 sits out untouched, a bad policy gives steps = -1, an env
// that is over at entry is not staged in, no auto-reset, the first step may follow another policy), and on top of it:
//   - T = wall_time at entry + horizon, ONE f64 addition (horizon > 0, +inf allowed: the host checks), written to t_stop[env] for
//     every env that takes part, an env that is over at entry included;
//   - before each step the env stops if it is terminated, needs a reset, has taken max_steps, or wall_time >= T. The wall time
//     sits in the staged header, so the exit is wave-uniform through the ballot that the episode's end goes through. (The first
//     step is taken whenever the addition moved T off the wall time, that is for every horizon that is not lost to rounding.)
//   - at exit, with the env still staged, the env's row of rem_work (f64[num_envs][J_cap], nullable) is zeroed and then, lanes over
//     the ordered active list as in policy_wfair's pass 1, rem_work[env][j] = job_work(jobview(j), active_mask): the f64 that
//     schedulers.job_work gives for that job on the env's observation, bit for bit. An env that is over at entry gets a zero row.
// A step is a step of sss_policy + sss_step, so a child can overshoot T by the length of its last step: the cost kernel knows.
// A kernel of its own with every policy inlined (run_policy<true>), for the reason sss_rollout_each_kernel is one: the kernels
// tests/test_abi.py holds to their register budgets keep the code they had. No recording (-DSSS_TIMELINE) form: the host refuses
// the call while a timeline is bound.
#ifndef SSS_TIMELINE
// the env's row of remaining work from the staged state (all lanes; wave-uniform control flow)
SSS_DEV void until_rem_work(double* row) {
  const int lane = wave_lane();
  for (int j = lane; j < g_c.J_cap; j += 64) row[j] = 0.0;
  wave_sync();  // a job's zero, written by one lane, comes before its work, written by another
  const int A = g_hot.h.n_active;
  for (int k = lane; k < A; k += 64) {
    const int j = (int)lds_active()[k];
    const JobView v = jobview(j);
    row[j] = job_work(v, v.job->active_mask);
  }
}

SSS_KERNEL void SSS_KNAME(sss_rollout_until_kernel)(SssKernelArgs a, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                                    const int32_t* first_param_of, double horizon, int max_steps, int32_t* steps, int32_t* first_stage,
                                                    int32_t* first_exec, double* t_stop, double* rem_work) {
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
  const double T = hdr->wall_time + horizon;
  if (wave_lane() == 0) t_stop[env] = T;
  double* row = rem_work ? rem_work + (size_t)env * (size_t)a.L.J_cap : nullptr;
  if (hdr->terminated || hdr->need_reset) {  // over at entry: not staged in, nothing is left to do in it
    if (steps && wave_lane() == 0) steps[env] = 0;
    if (row)
      for (int j = wave_lane(); j < a.L.J_cap; j += 64) row[j] = 0.0;
    return;
  }
  ctx_init();
  if (max_steps <= 0) {  // no step to take: the state is only read
    env_begin_readonly(base);
    if (row) until_rem_work(row);
    if (steps && wave_lane() == 0) steps[env] = 0;
    return;
  }
  env_begin(base);
  int taken = 0;
  for (int it = 0; it < max_steps; it++) {
    if (wave_ballot(g_hot.h.terminated || g_hot.h.need_reset || g_hot.h.wall_time >= T) != 0) break;  // the end, an env error, or the horizon
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
  if (row) until_rem_work(row);
  env_end(base);
  prof3_flush();
  if (steps && wave_lane() == 0) steps[env] = taken;
}

#ifndef __HIP__
// the CPU wave emulator's launchers, as in csrc/sss_sim_each.h; the gfx950 ones are in csrc/sss_hip_sim.hip and csrc/sss_hip_wide.hip
#ifdef SSS_WIDE
#include "sss_wide.h"
#define SSS_UNTIL_LAUNCHER sss_wide_launch_rollout_until
#else
#include "sss_narrow.h"
#define SSS_UNTIL_LAUNCHER sss_narrow_launch_rollout_until
#endif
int SSS_UNTIL_LAUNCHER(const SssKernelArgs& a, int num_envs, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                       const int32_t* first_param_of, double horizon, int max_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, double* t_stop,
                       double* rem_work, void*) {
  emu::g_kernargs = &a;
  emu::launch(num_envs, [&]() {
    SSS_KNAME(sss_rollout_until_kernel)(a, policy_of, param_of, first_policy_of, first_param_of, horizon, max_steps, steps, first_stage, first_exec, t_stop, rem_work);
  });
  return 0;
}
#undef SSS_UNTIL_LAUNCHER
#endif
#endif
