// sss_hip_sim.hip - gfx950 build of the simulator kernels for up to 64 executors (sss_sim.h: reset, step, bounded step, policy,
// rollout) and their launchers. A translation unit of its own - like the wide instantiation, sss_hip_wide.hip - because these two
// are the units compiled with `-mllvm -disable-machine-licm` (spark_sched_sim_amd/build.py says why); the C ABI, the Decima / GNN /
// training kernels and everything else live in sss_hip.hip and are compiled without that flag. -O3 -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "sss_sim.h"
#include "sss_narrow.h"

// the launchers of this unit: sss_narrow_launch_* - or, compiled with -DSSS_TIMELINE (csrc/sss_hip_sim_tl.hip), sss_narrow_tl_launch_* of the
// recording kernels, which the plain ones hand over to when a timeline is bound (SSS_TL_DISPATCH)
#ifdef SSS_TIMELINE
#define SSS_LAUNCHER(name) sss_narrow_tl_launch_##name
#define SSS_TL_DISPATCH(call)
#else
#define SSS_LAUNCHER(name) sss_narrow_launch_##name
#define SSS_TL_DISPATCH(call) \
  if (a.tl.t) return sss_narrow_tl_launch_##call
int sss_narrow_hot_bytes() { return (int)sizeof(SssHot); }
int sss_narrow_static_lds_bytes() { return SSS_STATIC_LDS_BYTES; }
#endif

int SSS_LAUNCHER(reset)(const SssKernelArgs& a, int num_envs, const uint64_t* seeds, const double* tl, const uint8_t* mask, void* stream) {
  SSS_TL_DISPATCH(reset(a, num_envs, seeds, tl, mask, stream));
  hipLaunchKernelGGL(SSS_KNAME(sss_reset_kernel), dim3(num_envs), dim3(64), (size_t)a.P.pool_bytes, (hipStream_t)stream, a, seeds, tl, mask);
  return (int)hipGetLastError();
}
int SSS_LAUNCHER(step_bounded)(const SssKernelArgs& a, int num_envs, const int32_t* stage_idx, const int32_t* num_exec, int auto_reset, uint64_t seed_stride,
                                   int budget, uint8_t* ready, void* stream) {
  SSS_TL_DISPATCH(step_bounded(a, num_envs, stage_idx, num_exec, auto_reset, seed_stride, budget, ready, stream));
  hipLaunchKernelGGL(SSS_KNAME(sss_step_bounded_kernel), dim3(num_envs), dim3(64), (size_t)a.P.pool_bytes, (hipStream_t)stream, a, stage_idx, num_exec, auto_reset, seed_stride,
                     budget, ready);
  return (int)hipGetLastError();
}
int SSS_LAUNCHER(step)(const SssKernelArgs& a, int num_envs, const int32_t* stage_idx, const int32_t* num_exec, int auto_reset, uint64_t seed_stride,
                           void* stream) {
  SSS_TL_DISPATCH(step(a, num_envs, stage_idx, num_exec, auto_reset, seed_stride, stream));
  hipLaunchKernelGGL(SSS_KNAME(sss_step_kernel), dim3(num_envs), dim3(64), (size_t)a.P.pool_bytes, (hipStream_t)stream, a, stage_idx, num_exec, auto_reset, seed_stride);
  return (int)hipGetLastError();
}
#ifndef SSS_TIMELINE
int SSS_LAUNCHER(policy)(const SssKernelArgs& a, int num_envs, int policy, int param, int32_t* stage_idx, int32_t* num_exec, void* stream) {
  if (policy == SSS_POLICY_HASH) {  // a thread per env, nothing staged (sss_sim.h)
    hipLaunchKernelGGL(SSS_KNAME(sss_policy_hash_kernel), dim3((num_envs + SSS_POLICY_HASH_THREADS - 1) / SSS_POLICY_HASH_THREADS), dim3(SSS_POLICY_HASH_THREADS), 0,
                       (hipStream_t)stream, a, num_envs, param, stage_idx, num_exec);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(SSS_KNAME(sss_policy_kernel), dim3(num_envs), dim3(64), (size_t)a.P.pool_bytes, (hipStream_t)stream, a, policy, param, stage_idx, num_exec);
  return (int)hipGetLastError();
}
int SSS_LAUNCHER(rollout_each)(const SssKernelArgs& a, int num_envs, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                               const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, void* stream) {
  hipLaunchKernelGGL(SSS_KNAME(sss_rollout_each_kernel), dim3(num_envs), dim3(64), (size_t)a.P.pool_bytes, (hipStream_t)stream, a, policy_of, param_of, first_policy_of,
                     first_param_of, n_steps, steps, first_stage, first_exec);
  return (int)hipGetLastError();
}
int SSS_LAUNCHER(rollout_until)(const SssKernelArgs& a, int num_envs, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                const int32_t* first_param_of, double horizon, int max_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec,
                                double* t_stop, double* rem_work, void* stream) {
  hipLaunchKernelGGL(SSS_KNAME(sss_rollout_until_kernel), dim3(num_envs), dim3(64), (size_t)a.P.pool_bytes, (hipStream_t)stream, a, policy_of, param_of, first_policy_of,
                     first_param_of, horizon, max_steps, steps, first_stage, first_exec, t_stop, rem_work);
  return (int)hipGetLastError();
}
// the fused rollout with Decima among the policies (csrc/sss_sim_decima.h): the simulator's pool and Decima's work space in one dynamic
// allocation. More than the default 64 KB of dynamic LDS has to be asked for, per device and kernel (as csrc/sss_hip.hip does for the
// policy kernels). -1: the working set does not fit a gfx950 workgroup's 160 KB (the host refuses that layout before it gets here)
int SSS_LAUNCHER(rollout_decima)(const SssKernelArgs& a, int num_envs, int greedy, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                 const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, const SssDecimaPolicyArgs& d,
                                 void* stream) {
  static size_t granted[2][64] = {{0}};
  const size_t lds = (size_t)decima_rollout_pool_bytes(a);
  if ((size_t)SSS_STATIC_LDS_BYTES + lds > (size_t)160 * 1024) return -1;
  auto kernel = greedy ? SSS_KNAME(sss_rollout_decima_argmax_kernel) : SSS_KNAME(sss_rollout_decima_kernel);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  size_t& g = granted[greedy ? 1 : 0][dev & 63];  // per device: the attribute belongs to the device's copy of the kernel
  if (lds > g) {
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -2;
    g = lds;
  }
  hipLaunchKernelGGL(kernel, dim3(num_envs), dim3(64), lds, (hipStream_t)stream, a, policy_of, param_of, first_policy_of, first_param_of, n_steps, steps, first_stage,
                     first_exec, d);
  return (int)hipGetLastError();
}
// the fused rollouts whose first step is a given action (csrc/sss_sim_action.h). d == nullptr: the heuristics' kernel and the
// simulator's pool alone; else the Decima kernel (greedy: its arg-max form) with the dynamic LDS of rollout_decima above
int SSS_LAUNCHER(rollout_action)(const SssKernelArgs& a, int num_envs, int greedy, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_stage_in,
                                 const int32_t* first_exec_in, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, const SssDecimaPolicyArgs* d,
                                 void* stream) {
  if (!d) {
    hipLaunchKernelGGL(SSS_KNAME(sss_rollout_action_kernel), dim3(num_envs), dim3(64), (size_t)a.P.pool_bytes, (hipStream_t)stream, a, policy_of, param_of, first_stage_in,
                       first_exec_in, n_steps, steps, first_stage, first_exec);
    return (int)hipGetLastError();
  }
  static size_t granted[2][64] = {{0}};
  const size_t lds = (size_t)decima_rollout_pool_bytes(a);
  if ((size_t)SSS_STATIC_LDS_BYTES + lds > (size_t)160 * 1024) return -1;
  auto kernel = greedy ? SSS_KNAME(sss_rollout_action_decima_argmax_kernel) : SSS_KNAME(sss_rollout_action_decima_kernel);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  size_t& g = granted[greedy ? 1 : 0][dev & 63];  // per device: the attribute belongs to the device's copy of the kernel
  if (lds > g) {
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -2;
    g = lds;
  }
  hipLaunchKernelGGL(kernel, dim3(num_envs), dim3(64), lds, (hipStream_t)stream, a, policy_of, param_of, first_stage_in, first_exec_in, n_steps, steps, first_stage,
                     first_exec, *d);
  return (int)hipGetLastError();
}
#endif
int SSS_LAUNCHER(rollout)(const SssKernelArgs& a, int num_envs, int policy, int param, int n_steps, int auto_reset, uint64_t seed_stride, void* stream) {
  SSS_TL_DISPATCH(rollout(a, num_envs, policy, param, n_steps, auto_reset, seed_stride, stream));
  if (policy >= SSS_POLICY_WFAIR)  // weighted fair / SJF-CP: the kernel that has them (sss_sim.h)
    hipLaunchKernelGGL(SSS_KNAME(sss_rollout_heur_kernel), dim3(num_envs), dim3(64), (size_t)a.P.pool_bytes, (hipStream_t)stream, a, policy, param, n_steps, auto_reset, seed_stride);
  else
    hipLaunchKernelGGL(SSS_KNAME(sss_rollout_kernel), dim3(num_envs), dim3(64), (size_t)a.P.pool_bytes, (hipStream_t)stream, a, policy, param, n_steps, auto_reset, seed_stride);
  return (int)hipGetLastError();
}

#if defined(SSS_EVPROF3) && !defined(SSS_TIMELINE)  // timing builds only (tools/debug/evprof3.py): reads and clears the scoped profiler's table
extern "C" int sss_debug_prof(unsigned long long* out64) {
  if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_prof3), sizeof(unsigned long long) * 96) != hipSuccess) return -1;
  static const unsigned long long zeros[96] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_prof3), zeros, sizeof(zeros)) == hipSuccess ? 0 : -1;
}
extern "C" int sss_debug_prof_min(unsigned long long min_step_ticks) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_prof3_min), &min_step_ticks, sizeof(min_step_ticks)) == hipSuccess ? 0 : -1;
}
#endif
