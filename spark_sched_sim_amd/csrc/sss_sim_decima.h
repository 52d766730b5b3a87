// sss_sim_decima.h - part of the simulator device code (csrc/sss_sim.h includes it behind sss_sim_until.h; not a stand-alone header):
// the per-env fused rollout with DECIMA among the policies (include/sss.h sss_rollout_decima) - a whole episode of the learned
// scheduler in one launch, every env at its own pace, and Decima as a candidate or base policy of the lookahead.
//
// Per env it is sss_rollout_each_kernel (csrc/sss_sim_each.h: policy -1 sits out untouched, a bad id gives steps = -1, an env that is
// over at entry is not staged in, no auto-reset, the first step may follow another policy, steps and the first action are reported)
// with one more policy id, SSS_POLICY_DECIMA = 5, legal in both the policy and the first-policy array; its param is ignored.
//   - a heuristic step is run_policy<true>, as there;
//   - a Decima step is decima_policy_wave<ARGMAX> (csrc/sss_decima_policy.h, unchanged) on the env's observation rows, a wave_sync,
//     then every lane loads the decision from d.stage_idx[env] / d.num_exec[env] - the function's own outputs are the hand-over and
//     end up holding the env's last decision - and do_step<true> takes it;
//   - the decision of the env's it-th step in this launch draws with rng_counter + it, `it` being the loop's count (heuristic
//     steps count too); seed, env and candidate key are the function's. A lock-step loop that passes counter0 + t at iteration t
//     draws the same numbers. The arg-max kernel ignores seed and counter.
// What a launch must get right that the lock-step pair gets for free:
//   - LDS. On the GPU every `extern __shared__` array starts at the same address: g_pool and the policy kernels' g_dp_lds alias.
//     This kernel names g_pool only and carves it: the simulator's pool first (P.pool_bytes), Decima's work space behind it
//     (decima_lds_bytes: 20 bytes per node slot + the global summary). The launcher asks for the sum.
//   - visibility. decima_policy_wave reads obs_i32, nodes, edge_links, dag_ptr and exec_supplies, which THIS wave wrote in
//     write_observation a moment earlier. Those are vector stores and vector loads of one wave with a wave_sync between them; no
//     pointer here or there is __restrict__ or marked invariant, so no load may go through the scalar cache or be hoisted over
//     the step loop (the fences of wave_sync are clobbers to the compiler).
//   - weights come from global memory (83 KB, L2-resident), as in sss_decima_policy_kernel: one wave per workgroup cannot pay for
//     the staged copy of the four-env policy kernel.
//   - registers. One wave per workgroup and the whole simulator plus the GNN inlined: the kernels carry their own launch bound
//     (one wave per SIMD, the full register file) instead of SSS_KERNEL's four.
// Kernels of their own for the reason sss_rollout_each_kernel is one. No recording (-DSSS_TIMELINE) form: the host refuses the
// call while a timeline is bound.
#ifndef SSS_TIMELINE
#ifndef __HIP__
#include <math.h>
#endif
#include "sss_gnn.h"
#define SSS_DECIMA_WAVE_ONLY
#include "sss_decima_policy.h"  // decima_policy_wave and what it needs; not the policy kernels (they live in another unit)
#undef SSS_DECIMA_WAVE_ONLY

enum { SSS_POLICY_DECIMA = 5 };

SSS_DEV bool decima_rollout_policy_ok(int policy, int param) { return policy == SSS_POLICY_DECIMA || each_policy_ok(policy, param); }
// Decima's LDS work space for n_cap node slots (csrc/sss_hip.hip be_launch_decima_policy_with uses the same figure per env)
static inline int decima_lds_bytes(int n_cap) { return (20 * n_cap + 64 + 63) & ~63; }
static inline int decima_rollout_pool_bytes(const SssKernelArgs& a) { return ((a.P.pool_bytes + 15) & ~15) + decima_lds_bytes(a.L.n_cap); }

template <bool ARGMAX>
SSS_DEV void rollout_decima_env(const SssKernelArgs& a, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec,
                                const SssDecimaPolicyArgs& d) {
  const int env = wave_env();
  // (everything up to env_begin is wave-uniform: loads from addresses that depend on the workgroup id alone)
  const int policy = policy_of ? policy_of[env] : (int)SSS_POLICY_DECIMA;  // no arrays: every env plays Decima
  if (policy == -1) return;
  const int param = policy_of ? param_of[env] : 0;
  int pol = policy, par = param;  // of the next step: the first step's, then the env's
  if (first_policy_of && first_policy_of[env] >= 0) pol = first_policy_of[env], par = first_param_of[env];
  if (!decima_rollout_policy_ok(policy, param) || !decima_rollout_policy_ok(pol, par)) {
    if (steps && wave_lane() == 0) steps[env] = -1;
    return;
  }
  uint8_t* base = (uint8_t*)a.B.state + (size_t)env * a.L.env_stride;
  const SssHdr* hdr = &((const SssHot*)base)->h;
  if (n_steps <= 0 || hdr->terminated || hdr->need_reset) {
    if (steps && wave_lane() == 0) steps[env] = 0;
    return;
  }
  uint8_t* const dp_lds = g_pool + ((a.P.pool_bytes + 15) & ~15);  // behind the simulator's pool
  ctx_init();
  env_begin(base);
  int taken = 0;
  for (int it = 0; it < n_steps; it++) {
    if (wave_ballot(g_hot.h.terminated || g_hot.h.need_reset) != 0) break;  // the episode's end or an env error: the env stays as it is
    int si, ne;
    if (pol == SSS_POLICY_DECIMA) {  // wave-uniform
      SssDecimaPolicyArgs ds = d;
      ds.rng_counter = d.rng_counter + (uint64_t)it;
      decima_policy_wave<ARGMAX>(a.L, a.B, a.L.E, ds, env, dp_lds);
      wave_sync();  // lane 0 wrote the decision
      si = (int)wave_bcast_u32((uint32_t)d.stage_idx[env], 0), ne = (int)wave_bcast_u32((uint32_t)d.num_exec[env], 0);
    } else {
      run_policy<true>(pol, par, si, ne);
    }
    if (it == 0 && wave_lane() == 0) {
      if (first_stage) first_stage[env] = si;
      if (first_exec) first_exec[env] = ne;
    }
    const double reward = do_step<true>(si, ne);
    write_observation(a.L, a.B, env, reward);
    wave_sync();  // ... and the next Decima step reads these rows
    pol = policy, par = param;
    taken++;
  }
  env_end(base);
  prof3_flush();
  if (steps && wave_lane() == 0) steps[env] = taken;
}

// (on the emulator SSS_KERNEL is extern "C": two named kernels over the one body)
#ifdef __HIP__
#define SSS_DECIMA_ROLLOUT_KERNEL extern "C" __global__ __launch_bounds__(64, 1)
#else
#define SSS_DECIMA_ROLLOUT_KERNEL SSS_KERNEL
#endif
SSS_DECIMA_ROLLOUT_KERNEL void SSS_KNAME(sss_rollout_decima_kernel)(SssKernelArgs a, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                                                    const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec,
                                                                    SssDecimaPolicyArgs d) {
  rollout_decima_env<false>(a, policy_of, param_of, first_policy_of, first_param_of, n_steps, steps, first_stage, first_exec, d);
}
SSS_DECIMA_ROLLOUT_KERNEL void SSS_KNAME(sss_rollout_decima_argmax_kernel)(SssKernelArgs a, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                                                                           const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage,
                                                                           int32_t* first_exec, SssDecimaPolicyArgs d) {
  rollout_decima_env<true>(a, policy_of, param_of, first_policy_of, first_param_of, n_steps, steps, first_stage, first_exec, d);
}

#ifndef __HIP__
#ifdef SSS_WIDE
#include "sss_wide.h"
#define SSS_DECIMA_LAUNCHER sss_wide_launch_rollout_decima
#else
#include "sss_narrow.h"
#define SSS_DECIMA_LAUNCHER sss_narrow_launch_rollout_decima
#endif
// the CPU wave emulator's launchers, as in csrc/sss_sim_each.h (its g_pool is a fixed 64 KB array: a larger working set is refused);
// the gfx950 ones, which ask for the dynamic LDS, are in csrc/sss_hip_sim.hip and csrc/sss_hip_wide.hip
int SSS_DECIMA_LAUNCHER(const SssKernelArgs& a, int num_envs, int greedy, const int32_t* policy_of, const int32_t* param_of, const int32_t* first_policy_of,
                        const int32_t* first_param_of, int n_steps, int32_t* steps, int32_t* first_stage, int32_t* first_exec, const SssDecimaPolicyArgs& d, void*) {
  if (decima_rollout_pool_bytes(a) > (int)sizeof(g_pool)) return -1;
  emu::g_kernargs = &a;
  emu::launch(num_envs, [&]() {
    if (greedy) SSS_KNAME(sss_rollout_decima_argmax_kernel)(a, policy_of, param_of, first_policy_of, first_param_of, n_steps, steps, first_stage, first_exec, d);
    else SSS_KNAME(sss_rollout_decima_kernel)(a, policy_of, param_of, first_policy_of, first_param_of, n_steps, steps, first_stage, first_exec, d);
  });
  return 0;
}
#undef SSS_DECIMA_LAUNCHER
#endif
#undef SSS_DECIMA_ROLLOUT_KERNEL
#endif
