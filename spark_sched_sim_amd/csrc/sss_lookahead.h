// sss_lookahead.h - from the children of a lookahead to its decision, in one launch (include/sss.h sss_lookahead_pick, where the
// outputs are defined; spark_sched_sim_amd/lookahead.py is the caller). Parent i of n_parents has K x S children - candidate k,
// sample s is env child[i][k][s] - that were forked from it and played to the end of their episodes; this kernel reads the
// children's blocks of the state arena (read only), scores the candidates and hands the winner's policy quadruple to the parent's
// entries of four per-env arrays: the arguments of the sss_rollout_each launch that then steps the parents. Nothing comes back to
// the host in between.
//   cost of a child    stats[1] of sss_job_stats, the same bits: ((0.0 + d_0) + d_1) + ... with js_duration over the arrived jobs in
//                      job-id order (sss_jobstats.h: js_env, js_duration; the order is the definition)
//   valid              its episode ended (terminated != 0) without an env error (err == 0); an id outside the arena is invalid
//   score of k         ((0.0 + cost[k][0]) + cost[k][1]) + ... over the samples, then one division by S; NaN if any sample is invalid
//   winner             the lowest score, ties to the lowest k, a NaN never wins; -1 when no candidate is valid - the parent then gets
//                      candidate 0's quadruple
// One wavefront per parent. Lanes stride over the parent's children (each walks its child's chain of additions: the chains are
// independent, the loads of a chain are), the costs meet in LDS (8 B x K x S <= 8 KB, hence the bound on K x S), lanes stride over
// the candidates for the scores, lane 0 takes the arg-min and writes the parent's entries. What bounds it is the latency of one
// child's chain (n additions and 16 n bytes of loads); the rollouts around it cost orders of magnitude more, it keeps no occupancy target.
// A parent id outside [0, num_envs) gets its best / score rows and no entry in the per-env arrays (as sss_env_copy skips pairs).
#pragma once
#include <stdint.h>

#include "sss_jobstats.h"

#define SSS_LA_MAX_CHILDREN 1024  // K * S per parent (the LDS cost table)

struct SssLookaheadArgs {
  SssJobStatsArgs js;  // the arena as js_env / the duration helpers take it: state, env_stride, off_t_arrival, off_t_completed, num_envs, J_cap
  int32_t n_parents, K, S, pad_;
  const int32_t* parent;  // i32[n_parents]
  const int32_t* child;   // i32[n_parents][K][S]
  const int32_t *cand_first_policy, *cand_first_param, *cand_policy, *cand_param;  // i32[K]
  int32_t* best;  // i32[n_parents]
  double* score;  // f64[n_parents][K]
  int32_t *env_first_policy, *env_first_param, *env_policy, *env_param;  // i32[num_envs], written at the parents' ids
};

// the cost of env `c`, NaN when it is no valid child
SSS_JS_ANY double la_child_cost(const SssLookaheadArgs& a, int c) {
  if (c < 0 || c >= a.js.num_envs) return (double)NAN;
  const uint8_t* base = a.js.state + (size_t)c * (size_t)a.js.env_stride;
  const SssHdr& h = *(const SssHdr*)base;
  if (!(h.terminated != 0 && h.err == 0)) return (double)NAN;
  const JsEnv e = js_env(a.js, h);
  const double* ta = (const double*)(base + a.js.off_t_arrival);
  const double* tc = (const double*)(base + a.js.off_t_completed);
  double total = 0.0;
  for (int j = 0; j < e.n; j++) total = total + js_duration(ta[j], tc[j], e.wall);
  return total;
}
// candidate k's score from the costs of its S samples (NaN = an invalid sample)
SSS_JS_ANY double la_score(const double* cost, int S) {
  double sum = 0.0;
  bool all_valid = true;
  for (int s = 0; s < S; s++) {
    all_valid = all_valid && cost[s] == cost[s];
    sum = sum + cost[s];
  }
  return all_valid ? sum / (double)S : (double)NAN;
}
SSS_JS_ANY int la_argmin(const double* score, int K) {
  int best = -1;
  for (int k = 0; k < K; k++)
    if (score[k] == score[k] && (best < 0 || score[k] < score[best])) best = k;
  return best;
}
// the decision of parent i: its row of `best`, and the winner's quadruple at the parent's id
SSS_JS_ANY void la_decide(const SssLookaheadArgs& a, int i, int best) {
  a.best[i] = best;
  const int p = a.parent[i], q = best < 0 ? 0 : best;
  if (p < 0 || p >= a.js.num_envs) return;
  a.env_first_policy[p] = a.cand_first_policy[q], a.env_first_param[p] = a.cand_first_param[q];
  a.env_policy[p] = a.cand_policy[q], a.env_param[p] = a.cand_param[q];
}

#if !defined(__HIPCC__)
// builds without a device compiler (the CPU wave emulator's library): the same functions in plain loops
static int be_launch_lookahead_pick(const SssLookaheadArgs& a, void*) {
  static thread_local double cost[SSS_LA_MAX_CHILDREN], score[SSS_LA_MAX_CHILDREN];
  const int KS = a.K * a.S;
  for (int i = 0; i < a.n_parents; i++) {
    for (int c = 0; c < KS; c++) cost[c] = la_child_cost(a, a.child[(size_t)i * KS + c]);
    for (int k = 0; k < a.K; k++) score[k] = a.score[(size_t)i * a.K + k] = la_score(cost + (size_t)k * a.S, a.S);
    la_decide(a, i, la_argmin(score, a.K));
  }
  return 0;
}
#else
__global__ __launch_bounds__(64) void sss_lookahead_pick_kernel(SssLookaheadArgs a) {
  __shared__ double cost[SSS_LA_MAX_CHILDREN], score[SSS_LA_MAX_CHILDREN];
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int KS = a.K * a.S;  // <= SSS_LA_MAX_CHILDREN (the host checks)
  for (int c = lane; c < KS; c += 64) cost[c] = la_child_cost(a, a.child[(size_t)i * KS + c]);
  __syncthreads();
  for (int k = lane; k < a.K; k += 64) score[k] = a.score[(size_t)i * a.K + k] = la_score(cost + (size_t)k * a.S, a.S);
  __syncthreads();
  if (lane == 0) la_decide(a, i, la_argmin(score, a.K));
}
static int be_launch_lookahead_pick(const SssLookaheadArgs& a, void* stream) {
  hipLaunchKernelGGL(sss_lookahead_pick_kernel, dim3((unsigned)a.n_parents), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
#endif
