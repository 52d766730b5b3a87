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

// ---- the same decision from children that stopped at a time horizon (include/sss.h sss_lookahead_pick_horizon) ----------------
// The children come from sss_rollout_until (csrc/sss_sim_until.h): child c stopped at its wall time w, at or behind the time
// T = t_stop[c] that all children of a parent share, and rem_work[c][j] is the work its job j still holds. Its cost is what its
// jobs have been charged so far plus, with tail = srpt, an estimate of what is left. The order of every sum is the definition:
//   valid      err == 0 and (terminated != 0 or w >= T), the id inside the arena; otherwise NaN (a child that max_steps cut short
//              of its horizon is invalid, as an unfinished child is to the pick above)
//   counted    the arrived jobs (j < n of js_env) with t_arrival[j] < T. Arrivals are drawn at reset and shared by every child of a
//              parent (also under `reseed`, which draws task durations only): the counted set is the SAME for all children of a
//              parent, which is what makes their costs comparable although they stopped at different wall times
//   tail none  cost = ((0.0 + d_0) + d_1) + ... over the counted jobs in id order, d_j = min(t_completed[j], min(T, w)) - t_arrival[j]:
//              every child is charged up to the common time T and nothing beyond
//   tail srpt  d_j = js_duration(t_arrival[j], t_completed[j], w): charged up to the child's own stop; and, unless the child is
//              terminated, plus the tail: W_j = rem_work[c][j] of the counted jobs with t_completed[j] > w, sorted ascending
//              W_(1) <= W_(2) <= ..., p_0 = 0.0, p_i = p_(i-1) + W_(i), tail = ((0.0 + p_1 / N) + p_2 / N) + ..., N = num_executors:
//              the flow time the unfinished jobs would still accrue if all executors served them as ONE machine, shortest
//              remaining work first. cost = sum + tail.
// With T = +inf every job counts and every valid child is terminated: both forms are la_child_cost, bit for bit.
// Scores, NaN handling, arg-min, ties, the -1 fallback and the per-env arrays are la_score / la_argmin / la_decide.
// One wavefront per parent again, looping over the parent's children: lanes fill the child's sort keys (LDS, 8 KB) while lane 0
// walks the chain of the d_j, the wave sorts the keys (js_key / js_compare_exchange, as sss_job_stats does), lane 0 walks the
// chain of the prefix sums. Latency of K x S such children per parent; the rollouts around it cost orders of magnitude more.
#define SSS_LA_TAIL_NONE 0
#define SSS_LA_TAIL_SRPT 1

struct SssLookaheadHorizonArgs {
  SssLookaheadArgs la;
  const double* t_stop;    // f64[num_envs]
  const double* rem_work;  // f64[num_envs][J_cap]
  int32_t tail, num_executors;
};

struct LhChild {  // what child c's header says (every field is the same on every lane)
  bool valid, terminated;
  int n;
  double w, T;
  const double *ta, *tc, *rw;
};
SSS_JS_ANY LhChild lh_child(const SssLookaheadHorizonArgs& a, int c) {
  LhChild ch;
  ch.valid = false, ch.terminated = false, ch.n = 0, ch.w = 0.0, ch.T = 0.0, ch.ta = ch.tc = ch.rw = nullptr;
  if (c < 0 || c >= a.la.js.num_envs) return ch;
  const uint8_t* base = a.la.js.state + (size_t)c * (size_t)a.la.js.env_stride;
  const SssHdr& h = *(const SssHdr*)base;
  const JsEnv e = js_env(a.la.js, h);
  ch.n = e.n, ch.w = e.wall, ch.T = a.t_stop[c], ch.terminated = h.terminated != 0;
  ch.valid = h.err == 0 && (ch.terminated || ch.w >= ch.T);
  ch.ta = (const double*)(base + a.la.js.off_t_arrival), ch.tc = (const double*)(base + a.la.js.off_t_completed);
  ch.rw = a.rem_work + (size_t)c * (size_t)a.la.js.J_cap;
  return ch;
}
// the srpt tail sorts the keys of the child's jobs; a job that is not in it sorts behind every work there is
SSS_JS_ANY bool lh_unfinished(const LhChild& ch, int j) { return ch.ta[j] < ch.T && ch.tc[j] > ch.w; }
SSS_JS_ANY uint64_t lh_key(const LhChild& ch, int j) { return lh_unfinished(ch, j) ? js_key(ch.rw[j]) : ~0ull; }
// the charged part: the counted jobs' d_j in id order; *m: the number of jobs whose keys the tail sorts
SSS_JS_ANY double lh_sum(const LhChild& ch, int tail, int* m) {
  const double upto = tail == SSS_LA_TAIL_SRPT ? ch.w : (ch.T < ch.w ? ch.T : ch.w);
  double total = 0.0;
  int cnt = 0;
  for (int j = 0; j < ch.n; j++) {
    if (!(ch.ta[j] < ch.T)) continue;
    total = total + js_duration(ch.ta[j], ch.tc[j], upto);
    cnt += lh_unfinished(ch, j) ? 1 : 0;
  }
  *m = cnt;
  return total;
}
SSS_JS_ANY double lh_tail(const uint64_t* sorted_key, int m, int num_executors) {
  const double N = (double)num_executors;
  double p = 0.0, tail = 0.0;
  for (int i = 0; i < m; i++) {
    p = p + js_unkey(sorted_key[i]);
    tail = tail + p / N;
  }
  return tail;
}

#if !defined(__HIPCC__)
static int be_launch_lookahead_pick_horizon(const SssLookaheadHorizonArgs& a, void*) {
  static thread_local double cost[SSS_LA_MAX_CHILDREN], score[SSS_LA_MAX_CHILDREN];
  static thread_local uint64_t key[SSS_MAX_JOBS];
  const int KS = a.la.K * a.la.S;
  for (int i = 0; i < a.la.n_parents; i++) {
    for (int c = 0; c < KS; c++) {
      const LhChild ch = lh_child(a, a.la.child[(size_t)i * KS + c]);
      if (!ch.valid) {
        cost[c] = (double)NAN;
        continue;
      }
      int m;
      const double sum = lh_sum(ch, a.tail, &m);
      cost[c] = sum;
      if (a.tail != SSS_LA_TAIL_SRPT || ch.terminated) continue;
      const int P = js_pow2(ch.n);
      for (int j = 0; j < P; j++) key[j] = j < ch.n ? lh_key(ch, j) : ~0ull;
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
          for (int t = 0; t < P / 2; t++) js_compare_exchange(key, k, j, t);
      cost[c] = sum + lh_tail(key, m, a.num_executors);
    }
    for (int k = 0; k < a.la.K; k++) score[k] = a.la.score[(size_t)i * a.la.K + k] = la_score(cost + (size_t)k * a.la.S, a.la.S);
    la_decide(a.la, i, la_argmin(score, a.la.K));
  }
  return 0;
}
#else
__global__ __launch_bounds__(64) void sss_lookahead_pick_horizon_kernel(SssLookaheadHorizonArgs a) {
  __shared__ double cost[SSS_LA_MAX_CHILDREN], score[SSS_LA_MAX_CHILDREN];
  __shared__ uint64_t key[SSS_MAX_JOBS];
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int KS = a.la.K * a.la.S;  // <= SSS_LA_MAX_CHILDREN (the host checks)
  for (int c = 0; c < KS; c++) {   // (everything that steers the loop body is block-uniform: it comes from the child's id and header)
    const LhChild ch = lh_child(a, a.la.child[(size_t)i * KS + c]);
    if (!ch.valid) {
      if (lane == 0) cost[c] = (double)NAN;
      continue;
    }
    const bool sort = a.tail == SSS_LA_TAIL_SRPT && !ch.terminated;
    const int P = sort ? js_pow2(ch.n) : 0;  // <= 1024: n <= J_cap <= SSS_MAX_JOBS (the host checks J_cap)
    for (int j = lane; j < P; j += 64) key[j] = j < ch.n ? lh_key(ch, j) : ~0ull;
    double sum = 0.0;
    int m = 0;
    if (lane == 0) sum = lh_sum(ch, a.tail, &m);  // (global loads only: the other lanes meet it at the sort's first barrier)
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = lane; t < P / 2; t += 64) js_compare_exchange(key, k, j, t);
        __syncthreads();
      }
    if (lane == 0) cost[c] = sort ? sum + lh_tail(key, m, a.num_executors) : sum;
    __syncthreads();  // the keys are free for the next child
  }
  __syncthreads();
  for (int k = lane; k < a.la.K; k += 64) score[k] = a.la.score[(size_t)i * a.la.K + k] = la_score(cost + (size_t)k * a.la.S, a.la.S);
  __syncthreads();
  if (lane == 0) la_decide(a.la, i, la_argmin(score, a.la.K));
}
static int be_launch_lookahead_pick_horizon(const SssLookaheadHorizonArgs& a, void* stream) {
  hipLaunchKernelGGL(sss_lookahead_pick_horizon_kernel, dim3((unsigned)a.la.n_parents), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
#endif
