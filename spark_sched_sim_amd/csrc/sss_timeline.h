// sss_timeline.h - the Gantt rasteriser of the executor timelines (include/sss.h sss_timeline_render): what the reference's
// renderer draws from Executor.history (components/renderer.py:84-135, spark_sched_sim.py:408-424) - one band of pixel rows per
// executor, coloured by the job the executor belongs to over time, with a red column where a job completed - as a uint8
// [height][width][3] frame per selected env, written by one kernel. The reference lays its segments out by accumulated
// ceil() widths in a pygame surface; here a frame is DEFINED by the rules below, all in fp64 (the units build with
// -ffp-contract=off), so that it can be checked bit for bit against a few lines of numpy:
//   T = the env's wall time, J = the episode's job count; executor i owns rows [i * rh, min((i + 1) * rh, height)), rh = ceil(height / E);
//   column x shows the entry in force at tx = (x + 0.5) * (T / width): the first entry k with tx < release_k (the open entry's
//   release is +inf; entries of zero length are therefore never chosen); T <= 0: the open entry everywhere;
//   job j >= 0 has colour trunc(c1 + p * (c2 - c1)) per channel, p = (j + 1) / J, c1 = (0, 100, 255), c2 = (2, 247, 112); -1 is black;
//   a row that overflowed its capacity is mid-grey (128, 128, 128) from the release time of its last stored entry on;
//   every job with t_completed < T draws a red (255, 0, 0) column over the whole height at x = min(width - 1, floor(width * t_completed / T)).
// The functions of one column are shared by the kernel and - builds without a device compiler (the CPU wave emulator's
// library) - by plain loops.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sss_layout.h"

#if defined(__HIPCC__)
#define SSS_TL_ANY __host__ __device__ inline
#else
#define SSS_TL_ANY static inline
#endif

struct SssRenderArgs {
  const uint8_t* state;     // the arena: header (wall time, job count) and the jobs' completion times
  int64_t env_stride, off_t_completed;
  int32_t num_envs, E;
  SssTimeline tl;
  const int32_t* env_ids;   // i32[n] or nullptr (= envs 0 .. n - 1); an id outside [0, num_envs) leaves its frame untouched
  int32_t n, W, H;
  int32_t rh, n_bands;      // rows per band = ceil(H / E); bands that own a row = ceil(H / rh) <= E
  uint8_t* rgb;             // u8[n][H][W][3]
};

#define TL_RED 0x0000FFu   // r | g << 8 | b << 16
#define TL_GREY 0x808080u

SSS_TL_ANY uint32_t tl_job_colour(int j, int J) {
  if (j < 0 || J <= 0) return 0u;
  const double p = (double)(j + 1) / (double)J;
  const double r = 0.0 + p * 2.0, g = 100.0 + p * 147.0, b = 255.0 + p * -143.0;
  const uint32_t ri = r > 255.0 ? 255u : (uint32_t)r, gi = g > 255.0 ? 255u : (uint32_t)g, bi = b < 0.0 ? 0u : (uint32_t)b;
  return ri | (gi << 8) | (bi << 16);
}

// what one executor's row shows: `count` as recorded (may exceed cap), `t` / `job` the row's cap entries
struct TlRow {
  const double* t;
  const int32_t* job;
  int closed;     // stored entries that have a release time: count - 1, or cap for a row that overflowed
  bool overflow;  // count > cap: the open entry is not stored
  int open_job;   // job of the open entry (rows that did not overflow)
};
SSS_TL_ANY TlRow tl_row(const SssTimeline& tl, size_t row) {
  TlRow r;
  const int cap = tl.cap;
  int count = tl.count[row];
  if (count < 1) count = 1;  // (rows are initialised with one entry; anything else is a caller's buffer that was never reset)
  r.t = tl.t + row * (size_t)cap, r.job = tl.job + row * (size_t)cap;
  r.overflow = count > cap;
  r.closed = r.overflow ? cap : count - 1;
  r.open_job = r.overflow ? -1 : r.job[count - 1];
  return r;
}
// colour of column x of the row's band (before the completion markers)
SSS_TL_ANY uint32_t tl_column_colour(const TlRow& r, double T, int J, int W, int x) {
  if (!(T > 0.0)) return r.overflow ? TL_GREY : tl_job_colour(r.open_job, J);
  const double tx = ((double)x + 0.5) * (T / (double)W);
  int lo = 0, hi = r.closed;  // the first k in [0, closed) with tx < t[k]; release times never decrease
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tx < r.t[mid]) hi = mid; else lo = mid + 1;
  }
  if (lo < r.closed) return tl_job_colour(r.job[lo], J);
  return r.overflow ? TL_GREY : tl_job_colour(r.open_job, J);
}
// the column a completed job marks, or -1
SSS_TL_ANY int tl_marker_column(double t_completed, double T, int W) {
  if (!(T > 0.0) || !(t_completed < T)) return -1;
  const double x = floor(((double)W * t_completed) / T);
  return x < 0.0 ? 0 : (x > (double)(W - 1) ? W - 1 : (int)x);
}
SSS_TL_ANY int tl_env_of(const SssRenderArgs& a, int sel) {
  const int env = a.env_ids ? a.env_ids[sel] : sel;
  return env >= 0 && env < a.num_envs ? env : -1;
}

#if !defined(__HIPCC__)
// builds without a device compiler (the CPU wave emulator's library): the same functions in plain loops
static int be_launch_timeline_render(const SssRenderArgs& a, void*) {
  for (int sel = 0; sel < a.n; sel++) {
    const int env = tl_env_of(a, sel);
    if (env < 0) continue;
    const uint8_t* base = a.state + (size_t)env * (size_t)a.env_stride;
    const SssHdr& h = ((const SssHot*)base)->h;
    const double T = h.wall_time;
    const int J = h.J;
    uint8_t* img = a.rgb + (size_t)sel * (size_t)a.H * (size_t)a.W * 3;
    for (int i = 0; i < a.n_bands; i++) {
      const TlRow r = tl_row(a.tl, (size_t)env * (size_t)a.E + (size_t)i);
      const int y0 = i * a.rh, y1 = (i + 1) * a.rh < a.H ? (i + 1) * a.rh : a.H;
      for (int x = 0; x < a.W; x++) {
        const uint32_t c = tl_column_colour(r, T, J, a.W, x);
        for (int y = y0; y < y1; y++) {
          uint8_t* px = img + ((size_t)y * (size_t)a.W + (size_t)x) * 3;
          px[0] = (uint8_t)c, px[1] = (uint8_t)(c >> 8), px[2] = (uint8_t)(c >> 16);
        }
      }
    }
    const double* tc = (const double*)(base + a.off_t_completed);
    for (int j = 0; j < J; j++) {
      const int x = tl_marker_column(tc[j], T, a.W);
      if (x < 0) continue;
      for (int y = 0; y < a.H; y++) {
        uint8_t* px = img + ((size_t)y * (size_t)a.W + (size_t)x) * 3;
        px[0] = 255, px[1] = 0, px[2] = 0;
      }
    }
  }
  return 0;
}
#else
// One wavefront per (selected env, band). The band's pixel rows are all the same W * 3 bytes, and - the frame being row-major -
// the band is ONE contiguous run of (rows * W * 3) bytes: that period is built once in LDS (lanes stride over the columns,
// each binary-searches the row's release times; the env's marker columns come from a bit map the lanes fill from the jobs'
// completion times first) and then streamed out as whole dwords, lane after lane (256 contiguous bytes per wave store), with
// byte stores only for the up to three bytes before the first and after the last aligned dword of the run.
// Dynamic LDS: the period (+ 3 bytes of wrap-around) and the bit map: render_lds_bytes(W).
static inline size_t render_lds_bytes(int W) { return (size_t)((W * 3 + 3 + 3) & ~3) + (size_t)((W + 31) / 32) * 4; }
__global__ __launch_bounds__(64) void sss_timeline_render_kernel(SssRenderArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t tl_lds[];
  const int lane = (int)threadIdx.x;
  const int sel = (int)(blockIdx.x / (unsigned)a.n_bands), band = (int)(blockIdx.x % (unsigned)a.n_bands);
  const int env = tl_env_of(a, sel);
  if (env < 0) return;  // (block-uniform)
  const int W = a.W, period = W * 3;
  uint8_t* const rowbuf = tl_lds;
  uint32_t* const marks = (uint32_t*)(tl_lds + ((period + 3 + 3) & ~3));
  const uint8_t* base = a.state + (size_t)env * (size_t)a.env_stride;
  const SssHdr& h = ((const SssHot*)base)->h;
  const double T = h.wall_time;
  const int J = h.J;
  for (int w = lane; w < (W + 31) / 32; w += 64) marks[w] = 0u;
  __syncthreads();
  const double* tc = (const double*)(base + a.off_t_completed);
  for (int j = lane; j < J; j += 64) {
    const int x = tl_marker_column(tc[j], T, W);
    if (x >= 0) atomicOr(&marks[x >> 5], 1u << (x & 31));
  }
  __syncthreads();
  const TlRow r = tl_row(a.tl, (size_t)env * (size_t)a.E + (size_t)band);
  for (int x = lane; x < W; x += 64) {
    const uint32_t c = ((marks[x >> 5] >> (x & 31)) & 1u) ? TL_RED : tl_column_colour(r, T, J, W, x);
    rowbuf[3 * x] = (uint8_t)c, rowbuf[3 * x + 1] = (uint8_t)(c >> 8), rowbuf[3 * x + 2] = (uint8_t)(c >> 16);
  }
  __syncthreads();
  if (lane < 3) rowbuf[period + lane] = rowbuf[lane % period];  // wrap-around: a dword may start in the period's last three bytes
  __syncthreads();
  const int y0 = band * a.rh, y1 = (band + 1) * a.rh < a.H ? (band + 1) * a.rh : a.H;
  const size_t nbytes = (size_t)(y1 - y0) * (size_t)period;
  uint8_t* const out = a.rgb + ((size_t)sel * (size_t)a.H + (size_t)y0) * (size_t)period;
  size_t head = (size_t)((0 - (uintptr_t)out) & 3);
  if (head > nbytes) head = nbytes;
  const size_t n_dw = (nbytes - head) / 4, tail0 = head + n_dw * 4;
  if ((size_t)lane < head) out[lane] = rowbuf[lane % period];
  if ((size_t)lane < nbytes - tail0) out[tail0 + lane] = rowbuf[(tail0 + lane) % (size_t)period];
  // byte position inside the period of this lane's dword, advanced by (256 mod period) per round instead of a division
  uint32_t pos = (uint32_t)((head + (size_t)lane * 4) % (size_t)period);
  const uint32_t adv = 256u % (uint32_t)period;
  uint32_t* const out_dw = (uint32_t*)(out + head);
  for (size_t d = (size_t)lane; d < n_dw; d += 64) {
    // (period >= 3 may be shorter than a dword: byte k of the dword sits at (pos + k) mod period)
    uint32_t v;
    if (period >= 4) {
      v = (uint32_t)rowbuf[pos] | ((uint32_t)rowbuf[pos + 1] << 8) | ((uint32_t)rowbuf[pos + 2] << 16) | ((uint32_t)rowbuf[pos + 3] << 24);
    } else {
      v = (uint32_t)rowbuf[pos] | ((uint32_t)rowbuf[(pos + 1) % 3] << 8) | ((uint32_t)rowbuf[(pos + 2) % 3] << 16) | ((uint32_t)rowbuf[pos] << 24);
    }
    out_dw[d] = v;
    pos += adv;
    if (pos >= (uint32_t)period) pos -= (uint32_t)period;
  }
}
static int be_launch_timeline_render(const SssRenderArgs& a, void* stream) {
  const size_t lds = render_lds_bytes(a.W);
  hipLaunchKernelGGL(sss_timeline_render_kernel, dim3((unsigned)a.n * (unsigned)a.n_bands), dim3(64), lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
#endif
