// sss_returns.h - what the trainer computes from the collected rollouts before the PPO epochs:
//   discounted returns   trainers/utils/returns_calculator.py:67-76: R_k = r_k + exp(-beta * 1e-3 * dt_k) * R_{k+1}, per rollout, from its end
//   baselines            trainers/utils/baselines.py:12-37 with trainer.py:206-207: for the rollouts of one job sequence, every
//                        rollout's value curve (step times -> returns) interpolated (numpy.interp) at each rollout's own step
//                        times; the baseline is the mean over the sequence's rollouts
// over the [T, B] record of `RolloutCollector` (row = step, column = env; `active` marks the rows an env recorded: a prefix of its
// column). As tensor operations these were a Python loop over T (7 441 rows at BASELINE config 5: 0.30 s) and twenty operations on
// [sequences, R, R, T] tensors (0.25 s) - a fifth of an update. One thread per env (returns: the recurrence is sequential in k,
// the loads are not) and one per (step, env) query (baselines); the arithmetic is the tensor form's, operation by operation - the
// mean over a sequence's rollouts in numpy's own summation order (baseline_pairwise).
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define SSS_ANY __host__ __device__ inline
#else
#define SSS_ANY static inline
#endif

struct SssReturnsArgs {
  int64_t T, B;
  const uint8_t* active;   // [T][B]
  const double* t_before;  // [T][B]
  const double* t_after;   // [T][B]
  const double* rewards;   // [T][B]
  double beta;
  double* out;             // [T][B]
};

SSS_ANY void returns_env(const SssReturnsArgs& a, int64_t b) {
  const double c = -a.beta * 1e-3;
  double R = 0.0;
  for (int64_t k = a.T - 1; k >= 0; k--) {
    const int64_t i = k * a.B + b;
    const bool on = a.active[i] != 0;
    if (on) R = a.rewards[i] + exp(c * (a.t_after[i] - a.t_before[i])) * R;
    a.out[i] = R * (on ? 1.0 : 0.0);
  }
}

struct SssBaselineArgs {
  int64_t T, B;
  int32_t R;               // rollouts per job sequence: envs g * R .. g * R + R - 1 belong together
  int32_t skip_empty;      // != 0: rollouts that recorded nothing are left out of their sequence's mean
  const uint8_t* active;   // [T][B]
  const double* times;     // [T][B] step times (non-decreasing along a column's active prefix)
  const double* values;    // [T][B]
  const int64_t* n;        // [B] recorded steps per env
  double* out;             // [T][B]
};

// numpy.interp's case analysis on column `col` with n knots: the LAST knot j with xp[j] <= x (0 if none), clamp at the last knot,
// exact hit -> fp[j], else slope * (x - xp[j]) + fp[j]
SSS_ANY double baseline_interp(const SssBaselineArgs& a, int64_t col, double x) {
  const int64_t n = a.n[col], last = n > 0 ? n - 1 : 0;
  int64_t lo = 0, hi = n;  // first knot > x (searchsorted right)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a.times[mid * a.B + col] <= x) lo = mid + 1; else hi = mid;
  }
  int64_t j = lo - 1;
  if (j < 0) j = 0;
  if (j > last) j = last;
  const int64_t j1 = j + 1 < last ? j + 1 : last;
  const double x0 = a.times[j * a.B + col], x1 = a.times[j1 * a.B + col], y0 = a.values[j * a.B + col], y1 = a.values[j1 * a.B + col];
  if (x == x0 || j == last || x < x0) return y0;
  const double slope = (y1 - y0) / (x1 - x0);
  return slope * (x - x0) + y0;
}
// one term of a sequence's mean: rollout j's curve at x (an empty rollout contributes 0 with skip_empty)
SSS_ANY double baseline_term(const SssBaselineArgs& a, int64_t g0, int j, double x) {
  const double y = baseline_interp(a, g0 + j, x);
  return a.skip_empty ? y * (a.n[g0 + j] > 0 ? 1.0 : 0.0) : y;
}
// The sum of terms [lo, lo + n) in the order numpy's add.reduce takes over a float64 axis - what `y_hat.mean()` does
// (baselines.py:33; numpy/core/src/umath/loops_utils.h.src, DOUBLE_pairwise_sum): fewer than 8 terms one after the other from
// 0.0; up to 128 terms eight strided partial sums combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail; above that the
// range is halved (the first half rounded down to a multiple of 8). With fewer than 8 rollouts per sequence (decima_tpch.yaml: 4)
// this is the plain running sum. Pinned against numpy itself in tests/test_emu_training.py.
SSS_ANY double baseline_pairwise(const SssBaselineArgs& a, int64_t g0, double x, int lo, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; i++) res = res + baseline_term(a, g0, lo + i, x);
    return res;
  }
  if (n <= 128) {
    double r[8];
    for (int k = 0; k < 8; k++) r[k] = baseline_term(a, g0, lo + k, x);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int k = 0; k < 8; k++) r[k] = r[k] + baseline_term(a, g0, lo + i + k, x);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res = res + baseline_term(a, g0, lo + i, x);
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return baseline_pairwise(a, g0, x, lo, n2) + baseline_pairwise(a, g0, x, lo + n2, n - n2);
}
SSS_ANY void baseline_query(const SssBaselineArgs& a, int64_t t, int64_t b) {
  const int64_t g0 = (b / a.R) * a.R;
  const double x = a.times[t * a.B + b];
  const double acc = baseline_pairwise(a, g0, x, 0, a.R);
  double cnt = (double)a.R;
  if (a.skip_empty) {
    cnt = 0.0;
    for (int j = 0; j < a.R; j++) cnt = cnt + (a.n[g0 + j] > 0 ? 1.0 : 0.0);
  }
  const double mean = a.skip_empty ? acc / (cnt < 1.0 ? 1.0 : cnt) : acc / (double)a.R;
  a.out[t * a.B + b] = mean * (a.active[t * a.B + b] ? 1.0 : 0.0);
}

// ---- differential (average-reward) returns: trainers/utils/returns_calculator.py:6-22 (CircularArray), :52-65, :78-89 ----------
// The moving window of (dt, reward) rows lives on the device as f64[cap][2]. One update takes the record's rows with dt > 0 in
// the reference's order (env-major: env 0's active steps in step order, then env 1's, ...; `chain(*deltas_list)`), keeps the last
// `cap` of them and shifts the window as CircularArray.extend does: the last keep = cap - n rows of the old window move to the
// front, the new rows follow. The move overlaps itself, so the update writes a second buffer (`dst`) from the first (`src`).
// The record is [T][B] row-major (lanes along b read coalesced) while the row order is env-major, so a row's slot is
//   env_off[b] (surviving rows of the envs before b) + pre[c][b] (those of env b in the chunks of WINDOW_CHUNK steps before
//   chunk c) + its rank inside its chunk - the overflow beyond cap
// in three passes: counts per (chunk, env), the two exclusive prefixes, then move + scatter. Integer counters only.
// The sums of the window's columns are taken over all cap rows in row order from 0.0 (numpy's axis-0 sum of a C-contiguous
// (cap, 2) array adds in exactly that order): one dependent chain of cap additions per column - the order is the definition.
#define WINDOW_CHUNK 64
struct SssWindowArgs {
  int64_t T, B, cap;
  const uint8_t* active;   // [T][B]
  const double* t_before;  // [T][B]
  const double* t_after;   // [T][B]
  const double* rewards;   // [T][B]
  const double* src;       // [cap][2] the window before
  double* dst;             // [cap][2] the window after
  int64_t n_chunks;        // ceil(T / WINDOW_CHUNK)
  int64_t* pre;            // [n_chunks][B] counts, then their exclusive prefix along the chunks of an env
  int64_t* env_off;        // [B] exclusive prefix over the envs of their surviving rows
  int64_t* n_new;          // [1] surviving rows of the record
};

SSS_ANY bool window_row_survives(const SssWindowArgs& a, int64_t i) { return a.active[i] != 0 && a.t_after[i] - a.t_before[i] > 0.0; }
// pass 1: surviving rows of env b in chunk c
SSS_ANY void window_count(const SssWindowArgs& a, int64_t c, int64_t b) {
  const int64_t t0 = c * WINDOW_CHUNK, t1 = t0 + WINDOW_CHUNK < a.T ? t0 + WINDOW_CHUNK : a.T;
  int64_t n = 0;
  for (int64_t t = t0; t < t1; t++) n += window_row_survives(a, t * a.B + b) ? 1 : 0;
  a.pre[c * a.B + b] = n;
}
// pass 2a: env b's counts -> their exclusive prefix along its chunks; returns the env's total
SSS_ANY int64_t window_env_prefix(const SssWindowArgs& a, int64_t b) {
  int64_t run = 0;
  for (int64_t c = 0; c < a.n_chunks; c++) {
    const int64_t n = a.pre[c * a.B + b];
    a.pre[c * a.B + b] = run;
    run += n;
  }
  return run;
}
// pass 3a: row i of the new window that comes from the old one (the last `keep` old rows move to the front)
SSS_ANY void window_move(const SssWindowArgs& a, int64_t i) {
  const int64_t n = *a.n_new < a.cap ? *a.n_new : a.cap, keep = a.cap - n;
  if (i < keep) a.dst[2 * i] = a.src[2 * (n + i)], a.dst[2 * i + 1] = a.src[2 * (n + i) + 1];
}
// pass 3b: env b's surviving rows of chunk c to their slots behind the kept rows (of more than cap new rows the last cap count)
SSS_ANY void window_scatter(const SssWindowArgs& a, int64_t c, int64_t b) {
  const int64_t n_new = *a.n_new, n = n_new < a.cap ? n_new : a.cap, keep = a.cap - n, drop = n_new - n;
  const int64_t t0 = c * WINDOW_CHUNK, t1 = t0 + WINDOW_CHUNK < a.T ? t0 + WINDOW_CHUNK : a.T;
  int64_t g = a.env_off[b] + a.pre[c * a.B + b];
  for (int64_t t = t0; t < t1; t++) {
    const int64_t i = t * a.B + b;
    if (!window_row_survives(a, i)) continue;
    if (g >= drop) {  // (keep + g - drop < cap: g < n_new)
      const int64_t s = keep + g - drop;
      a.dst[2 * s] = a.t_after[i] - a.t_before[i], a.dst[2 * s + 1] = a.rewards[i];
    }
    g++;
  }
}
// `n` rows added to the two running column sums, row after row
SSS_ANY void window_sum_rows(const double* rows, int64_t n, double& s0, double& s1) {
  for (int64_t i = 0; i < n; i++) s0 = s0 + rows[2 * i], s1 = s1 + rows[2 * i + 1];
}

struct SssDiffretArgs {
  int64_t T, B;
  const uint8_t* active;   // [T][B]
  const double* t_before;  // [T][B]
  const double* t_after;   // [T][B]
  const double* rewards;   // [T][B]
  const double* sums;      // [2] total time, reward sum (of this rank's window, or pooled over the ranks)
  double* out;             // [T][B]
  double* avg;             // [1]
};
// avg_num_jobs = -rew_sum / total_time (returns_calculator.py:52-55; an empty window gives -0.0 / 0.0 = nan, as there)
SSS_ANY double diffret_avg(const SssDiffretArgs& a) { return -a.sums[1] / a.sums[0]; }
// R = -(job_time - expected_job_time) + R with job_time = -r, expected_job_time = dt * avg (returns_calculator.py:57-60, 78-89),
// per env from its last row; the operations of training.DifferentialReturns in its order
SSS_ANY void diffret_env(const SssDiffretArgs& a, int64_t b) {
  const double avg = diffret_avg(a);
  double R = 0.0;
  for (int64_t k = a.T - 1; k >= 0; k--) {
    const int64_t i = k * a.B + b;
    const bool on = a.active[i] != 0;
    if (on) R = -(-a.rewards[i] - (a.t_after[i] - a.t_before[i]) * avg) + R;
    a.out[i] = R * (on ? 1.0 : 0.0);
  }
}

#if !defined(__HIPCC__)
// builds without a device compiler (the CPU wave emulator's library): the same functions in plain loops
static int be_launch_reward_window(const SssWindowArgs& a, void*) {
  for (int64_t c = 0; c < a.n_chunks; c++)
    for (int64_t b = 0; b < a.B; b++) window_count(a, c, b);
  int64_t run = 0;
  for (int64_t b = 0; b < a.B; b++) a.env_off[b] = run, run += window_env_prefix(a, b);
  *a.n_new = run;
  for (int64_t i = 0; i < a.cap; i++) window_move(a, i);
  for (int64_t c = 0; c < a.n_chunks; c++)
    for (int64_t b = 0; b < a.B; b++) window_scatter(a, c, b);
  return 0;
}
static int be_launch_window_sums(const double* win, int64_t cap, double* sums, void*) {
  double s0 = 0.0, s1 = 0.0;
  window_sum_rows(win, cap, s0, s1);
  sums[0] = s0, sums[1] = s1;
  return 0;
}
static int be_launch_diffret(const SssDiffretArgs& a, void*) {
  if (a.avg) *a.avg = diffret_avg(a);
  for (int64_t b = 0; b < a.B; b++) diffret_env(a, b);
  return 0;
}
#endif

#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void sss_window_count_kernel(SssWindowArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_chunks * a.B) window_count(a, i / a.B, i % a.B);
}
// one workgroup: a thread per env walks the env's chunks, then the envs' totals are scanned (shuffles inside a wave, LDS across
// the waves, a carry from one round of WINDOW_SCAN_THREADS envs to the next)
#define WINDOW_SCAN_THREADS 1024
__global__ __launch_bounds__(WINDOW_SCAN_THREADS) void sss_window_scan_kernel(SssWindowArgs a) {
  __shared__ int64_t wave_tot[WINDOW_SCAN_THREADS / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < a.B; b0 += WINDOW_SCAN_THREADS) {
    const int64_t b = b0 + tid;
    const int64_t tot = b < a.B ? window_env_prefix(a, b) : 0;
    int64_t incl = tot;
    for (int s = 1; s < 64; s <<= 1) {
      const int64_t t = __shfl_up(incl, s);
      if (lane >= s) incl += t;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int64_t base = carry + incl - tot, all = 0;
    for (int w = 0; w < WINDOW_SCAN_THREADS / 64; w++) {
      if (w < wave) base += wave_tot[w];
      all += wave_tot[w];
    }
    if (b < a.B) a.env_off[b] = base;
    carry += all;
    __syncthreads();  // (wave_tot is written again in the next round)
  }
  if (tid == 0) *a.n_new = carry;
}
__global__ __launch_bounds__(256) void sss_window_scatter_kernel(SssWindowArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.cap) window_move(a, i);
  if (i < a.n_chunks * a.B) window_scatter(a, i / a.B, i % a.B);
}
// The ordered sums: one workgroup. Every thread loads its share of the next tile of rows from memory (coalesced 16-byte rows)
// before thread 0 walks the current tile in LDS - the two columns are two independent chains in one lane, and the loads of
// the next tile are in flight while it adds.
#define WINDOW_SUM_THREADS 256
#define WINDOW_SUM_PER_THREAD 4
#define WINDOW_SUM_TILE (WINDOW_SUM_THREADS * WINDOW_SUM_PER_THREAD)
__global__ __launch_bounds__(WINDOW_SUM_THREADS) void sss_window_sum_kernel(const double* win, int64_t cap, double* sums) {
  __shared__ __attribute__((aligned(16))) double tile[2][2 * WINDOW_SUM_TILE];  // 2 x 16 KB
  const int tid = (int)threadIdx.x;
  const double2* rows = (const double2*)win;
  double2 reg[WINDOW_SUM_PER_THREAD];
  auto fetch = [&](int64_t r0) {
#pragma unroll
    for (int j = 0; j < WINDOW_SUM_PER_THREAD; j++) {
      const int64_t r = r0 + j * WINDOW_SUM_THREADS + tid;
      reg[j] = r < cap ? rows[r] : make_double2(0.0, 0.0);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int j = 0; j < WINDOW_SUM_PER_THREAD; j++) ((double2*)tile[buf])[j * WINDOW_SUM_THREADS + tid] = reg[j];
  };
  double s0 = 0.0, s1 = 0.0;
  fetch(0);
  stash(0);
  __syncthreads();
  int buf = 0;
  for (int64_t r0 = 0; r0 < cap; r0 += WINDOW_SUM_TILE, buf ^= 1) {
    const bool more = r0 + WINDOW_SUM_TILE < cap;
    if (more) fetch(r0 + WINDOW_SUM_TILE);
    if (tid == 0) window_sum_rows(tile[buf], cap - r0 < WINDOW_SUM_TILE ? cap - r0 : WINDOW_SUM_TILE, s0, s1);
    if (more) stash(buf ^ 1);
    __syncthreads();
  }
  if (tid == 0) sums[0] = s0, sums[1] = s1;
}
__global__ __launch_bounds__(64) void sss_diffret_kernel(SssDiffretArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b == 0 && a.avg) *a.avg = diffret_avg(a);
  if (b < a.B) diffret_env(a, b);
}

__global__ __launch_bounds__(64) void sss_returns_kernel(SssReturnsArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b < a.B) returns_env(a, b);
}
__global__ __launch_bounds__(256) void sss_baseline_kernel(SssBaselineArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.T * a.B) baseline_query(a, i / a.B, i % a.B);
}
#endif
