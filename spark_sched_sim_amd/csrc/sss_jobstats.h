// sss_jobstats.h - the episode metrics of every env in one launch (include/sss.h sss_job_stats, where the columns are defined):
//   job durations         spark_sched_sim/metrics.py:4-10: d_j = min(t_completed[j], wall_time) - t_arrival[j], jobs in id order
//   their sum             Python's sum(): ((0.0 + d_0) + d_1) + ...          (metrics.py:16-18 divides it by the wall time)
//   their mean            numpy.mean: numpy's pairwise order (js_pairwise), one division by n
//   their percentiles     numpy.percentile, default method "linear" (js_percentile)
//   the ring's mean       spark_sched_sim.py:243-245: numpy.mean over the deque of the last <= 200 completed jobs, * 1e-3
// The host functions (metrics.py here) copy an env's whole block to the host, once per env, for any of these; torch reductions over
// the arena (VecSparkSchedSimEnv.rollout_stats) add in another order and have no percentiles. Here every sum's ORDER is its
// definition, so one lane walks each chain; the wave's lanes share the loads, the sort and the percentiles.
//
// One wavefront per env. The env's durations go to LDS twice: in job-id order (the sums) and as order-preserving 64-bit keys
// padded with the largest key to a power of two P >= n, which a bitonic network sorts in place - log2(P) * (log2(P) + 1) / 2 <= 55
// rounds of P / 2 compare-exchanges, lanes striding over the pairs. LDS: 8 KB + 8 KB + the ring's 1.6 KB, static.
// What bounds it: the three dependent chains of f64 additions (n + n + dur_n <= 2248 additions at n = 1024, one lane, LDS
// operands) and the sort's rounds (<= 55 * 8 pair steps per lane, each two LDS reads and at most two writes) - latency, not
// bandwidth: an env contributes 16 n + 1920 bytes of reads (its two time arrays, header and ring) and 64 + 8 n_q bytes of writes.
// It is on no training path and keeps no occupancy target.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "sss_layout.h"

#if defined(__HIPCC__)
#define SSS_JS_ANY __host__ __device__ inline
#else
#define SSS_JS_ANY static inline
#endif

#define SSS_JS_MAX_Q 16
#define SSS_JS_COLS 8

struct SssJobStatsArgs {
  const uint8_t* state;  // the arena (read only)
  int64_t env_stride, off_t_arrival, off_t_completed, off_dur_ring;
  int32_t num_envs, J_cap, n_q, pad_;
  const double* q;        // f64[n_q] percents
  double* stats;          // f64[B][SSS_JS_COLS]
  double* pct;            // f64[B][n_q]
  double* sorted;         // nullable: f64[B][J_cap] the sorted durations, NaN behind them
  const uint8_t* active;  // nullable: u8[B], 0 = the env's rows are left alone
};

// a double as a 64-bit key that orders as the value does (any sign; the durations are non-negative, where this is the bit pattern
// with the top bit set)
SSS_JS_ANY uint64_t js_key(double d) {
  uint64_t u;
  memcpy(&u, &d, 8);
  return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
}
SSS_JS_ANY double js_unkey(uint64_t k) {
  const uint64_t u = k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull);
  double d;
  memcpy(&d, &u, 8);
  return d;
}
SSS_JS_ANY int js_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
// pair t (of P / 2) of the bitonic network's round (k, j): elements i and i + j, ascending where bit k of i is clear
SSS_JS_ANY void js_compare_exchange(uint64_t* key, int k, int j, int t) {
  const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
  const bool up = (i & k) == 0;
  const uint64_t a = key[i], b = key[l];
  if ((a > b) == up) key[i] = b, key[l] = a;
}

SSS_JS_ANY double js_duration(double t_arrival, double t_completed, double wall) { return (t_completed < wall ? t_completed : wall) - t_arrival; }

// The sum of a[0 .. n) in the order numpy's add.reduce takes over a contiguous float64 array (numpy/core/src/umath/
// loops_utils.h.src, DOUBLE_pairwise_sum; restated for the baselines as baseline_pairwise in sss_returns.h): fewer than 8 terms one
// after the other from 0.0; up to 128 terms eight strided partial sums combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
// tail; above that the range is halved, the first half rounded down to a multiple of 8.
SSS_JS_ANY double js_sum_block(const double* a, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; i++) res = res + a[i];
    return res;
  }
  double r[8];
  for (int k = 0; k < 8; k++) r[k] = a[k];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int k = 0; k < 8; k++) r[k] = r[k] + a[i + k];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; i++) res = res + a[i];
  return res;
}
// The halving is a recursion of bounded depth, unrolled by the template: a piece of n terms leaves pieces of at most
// ceil(n / 2) + 7, so 1024 -> 519 -> 267 -> 141 -> 78: four levels reach blocks of <= 128 terms for every n <= SSS_MAX_JOBS.
#define SSS_JS_SPLITS 4
static_assert(SSS_MAX_JOBS <= 1024 && SSS_DUR_RING <= 1024, "js_pairwise: SSS_JS_SPLITS halvings must reach 128 terms");
template <int D>
SSS_JS_ANY double js_pairwise_d(const double* a, int n) {
  if constexpr (D == 0) {
    return js_sum_block(a, n);
  } else {
    if (n <= 128) return js_sum_block(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return js_pairwise_d<D - 1>(a, n2) + js_pairwise_d<D - 1>(a + n2, n - n2);
  }
}
SSS_JS_ANY double js_pairwise(const double* a, int n) { return js_pairwise_d<SSS_JS_SPLITS>(a, n); }
// Python's sum(): from 0, term after term
SSS_JS_ANY double js_ordered_sum(const double* a, int n) {
  double res = 0.0;
  for (int i = 0; i < n; i++) res = res + a[i];
  return res;
}

// numpy.percentile(d, q) with the default method over the n sorted keys (numpy 2.2 numpy/lib/_function_base_impl.py):
//   :106-109 the method's virtual index: (n - 1) * quantiles ("linear" has its own lambda; the alpha / beta form of
//              _compute_virtual_index, :4590, serves the other methods), quantiles = q / 100 (:4257 true_divide)
//   :4736-4768 _get_indexes: previous = floor(vi), next = previous + 1; vi >= n - 1: both -1 (the last element); vi < 0: both 0
//   :4615-4636 _get_gamma: vi - previous, previous AFTER that replacement
//   :4639-4662 _lerp: a + (b - a) * t, replaced by b - (b - a) * (1 - t) where t >= 0.5
// A percent outside [0, 100] (numpy raises; the host refuses it before the launch) and n = 0 give NaN.
SSS_JS_ANY double js_percentile(const uint64_t* key, int n, double q) {
  if (n <= 0 || !(q >= 0.0 && q <= 100.0)) return (double)NAN;
  const double quant = q / 100.0;
  const double vi = (double)(n - 1) * quant;
  double prev = floor(vi), next = prev + 1.0;
  if (vi >= (double)(n - 1)) prev = -1.0, next = -1.0;
  if (vi < 0.0) prev = 0.0, next = 0.0;
  const int ip = (int)prev, in = (int)next;
  const double gamma = vi - (double)ip;
  const double a = js_unkey(key[ip < 0 ? n + ip : ip]), b = js_unkey(key[in < 0 ? n + in : in]);
  const double diff = b - a;
  double r = a + diff * gamma;
  if (gamma >= 0.5) r = b - diff * (1.0 - gamma);
  return r;
}

struct JsEnv {  // what the header says, clamped to what the arrays hold
  int n, ring_n, ring_head;
  double wall, n_completed, n_active;
};
SSS_JS_ANY JsEnv js_env(const SssJobStatsArgs& a, const SssHdr& h) {
  JsEnv e;
  e.n = h.next_arrival < 0 ? 0 : (h.next_arrival > a.J_cap ? a.J_cap : h.next_arrival);
  e.ring_n = h.dur_n < 0 ? 0 : (h.dur_n > SSS_DUR_RING ? SSS_DUR_RING : h.dur_n);
  e.ring_head = ((h.dur_head % SSS_DUR_RING) + SSS_DUR_RING) % SSS_DUR_RING;
  e.wall = h.wall_time, e.n_completed = (double)h.n_completed, e.n_active = (double)h.n_active;
  return e;
}
// the env's eight columns from its durations in job-id order and its ring in deque order
SSS_JS_ANY void js_columns(const JsEnv& e, const double* dur, const double* ring, double* out) {
  const double total = js_ordered_sum(dur, e.n);
  out[0] = (double)e.n;
  out[1] = total;
  out[2] = e.n > 0 ? js_pairwise(dur, e.n) / (double)e.n : (double)NAN;
  out[3] = total / e.wall;
  out[4] = e.ring_n > 0 ? js_pairwise(ring, e.ring_n) / (double)e.ring_n * 1e-3 : (double)NAN;
  out[5] = e.n_completed, out[6] = e.n_active, out[7] = e.wall;
}

#if !defined(__HIPCC__)
// builds without a device compiler (the CPU wave emulator's library): the same functions in plain loops
static int be_launch_job_stats(const SssJobStatsArgs& a, void*) {
  static thread_local double dur[SSS_MAX_JOBS], ring[SSS_DUR_RING];
  static thread_local uint64_t key[SSS_MAX_JOBS];
  for (int env = 0; env < a.num_envs; env++) {
    if (a.active && !a.active[env]) continue;
    const uint8_t* base = a.state + (size_t)env * (size_t)a.env_stride;
    const JsEnv e = js_env(a, *(const SssHdr*)base);
    const double* ta = (const double*)(base + a.off_t_arrival);
    const double* tc = (const double*)(base + a.off_t_completed);
    const double* rg = (const double*)(base + a.off_dur_ring);
    const int P = js_pow2(e.n);
    for (int j = 0; j < e.n; j++) dur[j] = js_duration(ta[j], tc[j], e.wall), key[j] = js_key(dur[j]);
    for (int j = e.n; j < P; j++) key[j] = ~0ull;
    for (int k = 0; k < e.ring_n; k++) ring[k] = rg[(e.ring_head + k) % SSS_DUR_RING];
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1)
        for (int t = 0; t < P / 2; t++) js_compare_exchange(key, k, j, t);
    if (a.sorted)
      for (int j = 0; j < a.J_cap; j++) a.sorted[(size_t)env * a.J_cap + j] = j < e.n ? js_unkey(key[j]) : (double)NAN;
    for (int k = 0; k < a.n_q; k++) a.pct[(size_t)env * a.n_q + k] = js_percentile(key, e.n, a.q[k]);
    js_columns(e, dur, ring, a.stats + (size_t)env * SSS_JS_COLS);
  }
  return 0;
}
#else
__global__ __launch_bounds__(64) void sss_job_stats_kernel(SssJobStatsArgs a) {
  __shared__ double dur[SSS_MAX_JOBS], ring[SSS_DUR_RING];
  __shared__ uint64_t key[SSS_MAX_JOBS];
  const int env = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (a.active && !a.active[env]) return;  // (block-uniform)
  const uint8_t* base = a.state + (size_t)env * (size_t)a.env_stride;
  const JsEnv e = js_env(a, *(const SssHdr*)base);
  const double* ta = (const double*)(base + a.off_t_arrival);
  const double* tc = (const double*)(base + a.off_t_completed);
  const double* rg = (const double*)(base + a.off_dur_ring);
  const int P = js_pow2(e.n);  // <= 1024: n <= J_cap <= SSS_MAX_JOBS (the host checks J_cap)
  for (int j = lane; j < e.n; j += 64) {
    const double d = js_duration(ta[j], tc[j], e.wall);
    dur[j] = d, key[j] = js_key(d);
  }
  for (int j = e.n + lane; j < P; j += 64) key[j] = ~0ull;
  for (int k = lane; k < e.ring_n; k += 64) ring[k] = rg[(e.ring_head + k) % SSS_DUR_RING];
  __syncthreads();
  // lane 0 walks the three chains (nothing below reads `dur` or `ring` again); the other lanes meet it at the sort's first barrier
  if (lane == 0) js_columns(e, dur, ring, a.stats + (size_t)env * SSS_JS_COLS);
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < P / 2; t += 64) js_compare_exchange(key, k, j, t);
      __syncthreads();
    }
  if (a.sorted)
    for (int j = lane; j < a.J_cap; j += 64) a.sorted[(size_t)env * a.J_cap + j] = j < e.n ? js_unkey(key[j]) : (double)NAN;
  if (lane < a.n_q) a.pct[(size_t)env * a.n_q + lane] = js_percentile(key, e.n, a.q[lane]);
}
static int be_launch_job_stats(const SssJobStatsArgs& a, void* stream) {
  hipLaunchKernelGGL(sss_job_stats_kernel, dim3((unsigned)a.num_envs), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
#endif
