// sss_wide.h - what the host side (sss_host.h) needs of the WIDE instantiation of the simulator, the one that runs envs with
// 65..128 executors (sss_sim.h compiled with -DSSS_WIDE in its own translation unit: csrc/sss_hip_wide.hip on gfx950,
// tests/emu/emu_wide.cpp on the CPU wave emulator). Its SssHot / scratch have 128-entry executor arrays, so the layout
// sizes come from that unit; the launchers mirror be_launch_reset / _step / _policy / _rollout of the narrow unit.
#pragma once
#include <stdint.h>

#include "sss_layout.h"

int sss_wide_hot_bytes();         // sizeof(SssHot) with SSS_MAX_EXEC = 128
int sss_wide_static_lds_bytes();  // SSS_STATIC_LDS_BYTES of that instantiation
int sss_wide_launch_reset(const SssKernelArgs& a, int num_envs, const uint64_t* seeds, const double* tl, const uint8_t* mask, void* stream);
int sss_wide_launch_step_bounded(const SssKernelArgs& a, int num_envs, const int32_t* stage_idx, const int32_t* num_exec, int auto_reset, uint64_t seed_stride,
                                 int budget, uint8_t* ready, void* stream);
int sss_wide_launch_step(const SssKernelArgs& a, int num_envs, const int32_t* stage_idx, const int32_t* num_exec, int auto_reset, uint64_t seed_stride, void* stream);
int sss_wide_launch_policy(const SssKernelArgs& a, int num_envs, int policy, int param, int32_t* stage_idx, int32_t* num_exec, void* stream);
int sss_wide_launch_rollout(const SssKernelArgs& a, int num_envs, int policy, int param, int n_steps, int auto_reset, uint64_t seed_stride, void* stream);
// the fused rollout with a policy per env (csrc/sss_sim_each.h, which also holds the emulator's definition); no recording form
int sss_wide_launch_rollout_each(const SssKernelArgs& a, int num_envs, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                 const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, void* stream);
// ... and the one with a stop time that reports the remaining work per job (csrc/sss_sim_until.h, likewise); no recording form
int sss_wide_launch_rollout_until(const SssKernelArgs& a, int num_envs, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                  const int32_t* first_param_of, double horizon, int max_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, double* t_stop,
                                  double* rem_work, void* stream);
// ... and the one with Decima among the policies (csrc/sss_sim_decima.h, likewise; greedy: its arg-max kernel); no recording form.
// A negative return: the env layout's LDS working set does not fit
struct SssDecimaPolicyArgs;  // csrc/sss_decima_policy.h
int sss_wide_launch_rollout_decima(const SssKernelArgs& a, int num_envs, int greedy, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                    const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, const SssDecimaPolicyArgs& d,
                                    void* stream);
// ... and the ones whose first step is a given action (csrc/sss_sim_action.h, likewise; d == nullptr: the heuristics' kernel, else the
// Decima kernel, greedy: its arg-max form); no recording form. A negative return: the env layout's LDS working set does not fit
int sss_wide_launch_rollout_action(const SssKernelArgs& a, int num_envs, int greedy, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_stage_in,
                                    const int32_t* first_exec_in, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, const SssDecimaPolicyArgs* d,
                                    void* stream);
// ... and of the kernels that record the executor timelines (csrc/sss_hip_wide_tl.hip: the same unit compiled with -DSSS_TIMELINE;
// the launchers above hand over to these when SssKernelArgs::tl is bound)
int sss_wide_tl_launch_reset(const SssKernelArgs& a, int num_envs, const uint64_t* seeds, const double* tl, const uint8_t* mask, void* stream);
int sss_wide_tl_launch_step_bounded(const SssKernelArgs& a, int num_envs, const int32_t* stage_idx, const int32_t* num_exec, int auto_reset, uint64_t seed_stride,
                                 int budget, uint8_t* ready, void* stream);
int sss_wide_tl_launch_step(const SssKernelArgs& a, int num_envs, const int32_t* stage_idx, const int32_t* num_exec, int auto_reset, uint64_t seed_stride, void* stream);
int sss_wide_tl_launch_rollout(const SssKernelArgs& a, int num_envs, int policy, int param, int n_steps, int auto_reset, uint64_t seed_stride, void* stream);
