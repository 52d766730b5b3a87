// sss_fork.h - copies of running environments (include/sss.h sss_env_copy): what `copy.deepcopy(env)` is for the reference's
// SparkSchedSimEnv (spark_sched_sim.py:34-125 - every field of the env, its executors, jobs, tracker and sampler), for n
// (source, destination) pairs in one launch. An env lives in a STORE - its block of a state arena, its rows of the six observation
// buffers and, optionally, its rows of the three timeline arrays; the two ends of a pair may be in different stores of one layout:
// the buffers bound to the handle (fork), or slots the caller allocated (snapshot one way, restore the other).
//
// What moves per pair - the env's IMAGE:
//   the dense part of the block   [0, off_pool_tab) and [off_dur_ring, env_stride): SssHot, the active lists, jobs, arrival and
//                                 completion times, stages, durations, pool records, the duration ring, the old-active list
//   the overflow area             only the table slots of pools whose record says mask != 7. A slot behind a mask == 7 record is
//                                 never interpreted: pool_open / pool_stage_in / pool_pair_* work on the record's inline bytes then,
//                                 a table that grows is cleared over its whole new size before the keys go in (set_resize), the
//                                 staged forms write back only the words they changed, and a table of mask m is read in [0, m]
//                                 alone. do_reset relies on the same thing: it rewrites the records and leaves the area as it is.
//   the observation rows          their live prefix: n_nodes node rows, n_edges edge rows, n_jobs + 1 / n_jobs entries of dag_ptr /
//                                 exec_supplies (the counts are the source's obs_i32 row, clamped to the capacities), obs_i32, obs_f64
//   the timeline rows             min(count, cap) entries per executor and the count - when both stores have a timeline
// What does NOT move: the destination's lifetime counters (n_steps, n_events, model_bytes, prof[5], n_fast, n_batched, n_rounds - the
// sums of VecSparkSchedSimEnv.counters() are the same before and after). obs_bind_gen becomes the destination store's buffer
// generation when the source's rows were current in the source store (else 0: the next observation writes the edge rows again).
// Optionally the destination's generator becomes Generator(PCG64(SeedSequence(seed))) afresh - numpy's construction, restated
// below from sss_sim_rng.h rng_seed (that file is a part of the simulator units and cannot be included on its own; the tests pin
// both against numpy): every arrival was drawn at reset, so a reseeded copy keeps the job sequence and draws new task durations.
//
// One workgroup of 256 threads per pair; no LDS, no barrier: every byte of the destination image is written by one thread from
// bytes of the source alone. The dense part goes in 16-byte accesses, lane after lane (256 contiguous bytes per wave instruction);
// the pool records are walked 64 at a time per wave (one record's mask per lane, a ballot, then the wave copies each grown table
// with one 16-byte access per lane); the observation and timeline rows in 16-byte accesses where both ends are aligned, else in
// dwords. It is a copy: what bounds it is HBM bandwidth over the bytes of the image (about a tenth of the block: the overflow
// area is 256 B x (1 + J + J * SP) pools), profiles/fork.md.
// A pair with an id outside its store is skipped. Destination ids must be distinct and - within one store - disjoint from the
// source ids (the caller's duty): otherwise an image may be garbage, but every access stays inside the two stores.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sss_layout.h"

#if defined(__HIPCC__)
#define SSS_FK_ANY __host__ __device__ inline
#else
#define SSS_FK_ANY static inline
#endif

#define SSS_FK_THREADS 256
#define SSS_FK_FOREIGN_GEN 0xFFFFFFFFu  // buffer generation of a caller-allocated store (a handle's generations count up from 1)

struct SssStore {
  uint8_t* state;  // blocks of env_stride bytes, 256-byte aligned
  float* nodes;
  int32_t *edge_links, *dag_ptr, *exec_supplies, *obs_i32;
  double* obs_f64;
  SssTimeline tl;  // t == nullptr: the store has no timeline rows
  int32_t num_slots;
  uint32_t gen;
};

struct SssForkArgs {
  SssStore src, dst;
  const int32_t *src_ids, *dst_ids;  // i32[n]
  const uint64_t* reseed;            // u64[n] or nullptr
  int32_t n, E, J_cap, n_cap, ed_cap, n_pools, table_bytes, pad_;
  int64_t env_stride, off_pool_hdr, off_pool_tab, off_dur_ring;
};

static_assert(sizeof(SssHdr) % 8 == 0 && offsetof(SssHdr, n_steps) % 8 == 0 && offsetof(SssHdr, prof) % 8 == 0 && offsetof(SssHdr, err_line) % 8 == 0 &&
                  offsetof(SssHdr, obs_n_edges) % 8 == 0 && offsetof(SssHdr, obs_bind_gen) == offsetof(SssHdr, obs_n_edges) + 4 &&
                  offsetof(SssHdr, rng_has32) == 32 && offsetof(SssHdr, wall_time) == 40,
              "the header is merged as 64-bit words (fk_header_word)");
#define SSS_FK_HDR_WORDS ((int)(sizeof(SssHdr) / 8))

// word w of the header belongs to the env's lifetime: n_steps, n_events, model_bytes; prof[5], n_fast, n_batched, n_rounds
SSS_FK_ANY bool fk_lifetime_word(int w) {
  return (w >= (int)(offsetof(SssHdr, n_steps) / 8) && w <= (int)(offsetof(SssHdr, model_bytes) / 8)) ||
         (w >= (int)(offsetof(SssHdr, prof) / 8) && w < (int)(offsetof(SssHdr, err_line) / 8));
}
// the destination's header word w from the source's and its own
SSS_FK_ANY uint64_t fk_header_word(int w, uint64_t src, uint64_t own, uint32_t src_gen, uint32_t dst_gen) {
  if (fk_lifetime_word(w)) return own;
  if (w == (int)(offsetof(SssHdr, obs_n_edges) / 8)) {  // obs_n_edges | obs_bind_gen << 32
    const bool current = (uint32_t)(src >> 32) == src_gen;
    return (src & 0xFFFFFFFFull) | ((uint64_t)(current ? dst_gen : 0u) << 32);
  }
  return src;
}

SSS_FK_ANY uint64_t fk_mul64hi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// one step of numpy's pcg64 (128-bit LCG, multiplier 0x2360ED051FC65DA44385DF649FCCF645) on out[0..3] = state hi, lo, inc hi, lo
SSS_FK_ANY void fk_pcg_step(uint64_t* s) {
  const uint64_t mh = 0x2360ED051FC65DA4ull, ml = 0x4385DF649FCCF645ull;
  const uint64_t plo = s[1] * ml, phi = fk_mul64hi(s[1], ml) + s[0] * ml + s[1] * mh;
  const uint64_t rlo = plo + s[3];
  s[0] = phi + s[2] + (rlo < plo ? 1ull : 0ull), s[1] = rlo;
}
SSS_FK_ANY uint32_t fk_hashmix(uint32_t value, uint32_t& hash_const) {
  value ^= hash_const;
  hash_const *= 0x931e8875u;
  value *= hash_const;
  value ^= value >> 16;
  return value;
}
SSS_FK_ANY uint32_t fk_mix(uint32_t x, uint32_t y) {
  uint32_t r = 0xca01f9ddu * x - 0x4973f715u * y;
  r ^= r >> 16;
  return r;
}
// Generator(PCG64(SeedSequence(seed))): header words 0..3 (rng_state_hi, rng_state_lo, rng_inc_hi, rng_inc_lo); word 4
// (rng_has32, rng_u32) is 0 for a fresh generator
SSS_FK_ANY void fk_seed(uint64_t seed, uint64_t* out) {
  const uint32_t ent0 = (uint32_t)seed, ent1 = (uint32_t)(seed >> 32);
  uint32_t pool[4];
  uint32_t hc = 0x43b0d7e5u;
  pool[0] = fk_hashmix(ent0, hc);
  pool[1] = fk_hashmix(ent1, hc);  // (a seed below 2^32 is one word of entropy, the second pool word mixes 0: the same thing)
  pool[2] = fk_hashmix(0u, hc);
  pool[3] = fk_hashmix(0u, hc);
  for (int s = 0; s < 4; s++)
    for (int d = 0; d < 4; d++)
      if (s != d) pool[d] = fk_mix(pool[d], fk_hashmix(pool[s], hc));
  uint32_t w[8];
  uint32_t hb = 0x8b51f9ddu;
  for (int i = 0; i < 8; i++) {
    uint32_t v = pool[i & 3];
    v ^= hb;
    hb *= 0x58f38dedu;
    v *= hb;
    v ^= v >> 16;
    w[i] = v;
  }
  const uint64_t s0 = (uint64_t)w[0] | ((uint64_t)w[1] << 32), s1 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
  const uint64_t s2 = (uint64_t)w[4] | ((uint64_t)w[5] << 32), s3 = (uint64_t)w[6] | ((uint64_t)w[7] << 32);
  out[2] = (s2 << 1) | (s3 >> 63), out[3] = (s3 << 1) | 1ull;  // inc = (initseq << 1) | 1
  out[0] = 0, out[1] = 0;
  fk_pcg_step(out);
  const uint64_t lo = out[1] + s1;
  out[0] = out[0] + s0 + (lo < s1 ? 1ull : 0ull), out[1] = lo;
  fk_pcg_step(out);
}

SSS_FK_ANY int fk_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
struct FkCounts {
  int n_nodes, n_edges, n_jobs;
};
SSS_FK_ANY FkCounts fk_counts(const SssForkArgs& a, int s) {
  const int32_t* o = a.src.obs_i32 + (size_t)s * SSS_OBS_I32;
  FkCounts c;
  c.n_nodes = fk_clamp(o[OBS_N_NODES], a.n_cap), c.n_edges = fk_clamp(o[OBS_N_EDGES], a.ed_cap), c.n_jobs = fk_clamp(o[OBS_N_JOBS], a.J_cap);
  return c;
}
// the ids of pair i, or false when one lies outside its store
SSS_FK_ANY bool fk_pair(const SssForkArgs& a, int i, int& s, int& d) {
  s = a.src_ids[i], d = a.dst_ids[i];
  return s >= 0 && s < a.src.num_slots && d >= 0 && d < a.dst.num_slots;
}
// entries of executor row `row` that both timelines store
SSS_FK_ANY int fk_tl_entries(const SssForkArgs& a, int count) {
  const int cap = a.src.tl.cap < a.dst.tl.cap ? a.src.tl.cap : a.dst.tl.cap;
  return fk_clamp(count, cap);
}

#if !defined(__HIPCC__)
// builds without a device compiler (the CPU wave emulator's library): the same image in plain loops
static int be_launch_env_copy(const SssForkArgs& a, void*) {
  for (int i = 0; i < a.n; i++) {
    int s, d;
    if (!fk_pair(a, i, s, d)) continue;
    const uint8_t* sb = a.src.state + (size_t)s * (size_t)a.env_stride;
    uint8_t* db = a.dst.state + (size_t)d * (size_t)a.env_stride;
    uint64_t seeded[5] = {0, 0, 0, 0, 0};
    if (a.reseed) fk_seed(a.reseed[i], seeded);
    for (int w = 0; w < SSS_FK_HDR_WORDS; w++) {
      uint64_t sv, own;
      memcpy(&sv, sb + 8 * w, 8), memcpy(&own, db + 8 * w, 8);
      const uint64_t v = (a.reseed && w < 5) ? seeded[w] : fk_header_word(w, sv, own, a.src.gen, a.dst.gen);
      memcpy(db + 8 * w, &v, 8);
    }
    memmove(db + sizeof(SssHdr), sb + sizeof(SssHdr), (size_t)a.off_pool_tab - sizeof(SssHdr));
    memmove(db + a.off_dur_ring, sb + a.off_dur_ring, (size_t)(a.env_stride - a.off_dur_ring));
    for (int p = 0; p < a.n_pools; p++) {
      const SssPoolHdr* ph = (const SssPoolHdr*)(sb + a.off_pool_hdr) + p;
      if (ph->mask != 7) memmove(db + a.off_pool_tab + (size_t)p * a.table_bytes, sb + a.off_pool_tab + (size_t)p * a.table_bytes, (size_t)a.table_bytes);
    }
    const FkCounts c = fk_counts(a, s);
    memmove(a.dst.nodes + (size_t)d * a.n_cap * 3, a.src.nodes + (size_t)s * a.n_cap * 3, (size_t)c.n_nodes * 12);
    memmove(a.dst.edge_links + (size_t)d * a.ed_cap * 2, a.src.edge_links + (size_t)s * a.ed_cap * 2, (size_t)c.n_edges * 8);
    memmove(a.dst.dag_ptr + (size_t)d * (a.J_cap + 1), a.src.dag_ptr + (size_t)s * (a.J_cap + 1), (size_t)(c.n_jobs + 1) * 4);
    memmove(a.dst.exec_supplies + (size_t)d * a.J_cap, a.src.exec_supplies + (size_t)s * a.J_cap, (size_t)c.n_jobs * 4);
    memmove(a.dst.obs_i32 + (size_t)d * SSS_OBS_I32, a.src.obs_i32 + (size_t)s * SSS_OBS_I32, SSS_OBS_I32 * 4);
    memmove(a.dst.obs_f64 + (size_t)d * SSS_OBS_F64, a.src.obs_f64 + (size_t)s * SSS_OBS_F64, SSS_OBS_F64 * 8);
    if (a.src.tl.t && a.dst.tl.t)
      for (int e = 0; e < a.E; e++) {
        const size_t sr = (size_t)s * a.E + e, dr = (size_t)d * a.E + e;
        const int count = a.src.tl.count[sr], m = fk_tl_entries(a, count);
        memmove(a.dst.tl.t + dr * a.dst.tl.cap, a.src.tl.t + sr * a.src.tl.cap, (size_t)m * 8);
        memmove(a.dst.tl.job + dr * a.dst.tl.cap, a.src.tl.job + sr * a.src.tl.cap, (size_t)m * 4);
        a.dst.tl.count[dr] = count;
      }
  }
  return 0;
}
#else
// n_words dwords from src to dst, the threads of the workgroup striding over them: 16 bytes per access where both ends allow it
__device__ __forceinline__ void fk_copy_words(void* dst, const void* src, size_t n_words, int tid) {
  size_t done = 0;
  if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
    const size_t n16 = n_words / 4;
    for (size_t k = (size_t)tid; k < n16; k += SSS_FK_THREADS) ((uint4*)dst)[k] = ((const uint4*)src)[k];
    done = n16 * 4;
  }
  for (size_t k = done + (size_t)tid; k < n_words; k += SSS_FK_THREADS) ((uint32_t*)dst)[k] = ((const uint32_t*)src)[k];
}
__global__ __launch_bounds__(SSS_FK_THREADS) void sss_env_copy_kernel(SssForkArgs a) {
  const int pair = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int s, d;
  if (!fk_pair(a, pair, s, d)) return;  // (block-uniform)
  const uint8_t* sb = a.src.state + (size_t)s * (size_t)a.env_stride;
  uint8_t* db = a.dst.state + (size_t)d * (size_t)a.env_stride;
  // the header, a 64-bit word per thread: the lifetime words stay, the generator's five come from the seed when there is one
  if (tid < SSS_FK_HDR_WORDS) {
    if (a.reseed && tid < 5) {
      if (tid == 0) {
        uint64_t seeded[5] = {0, 0, 0, 0, 0};
        fk_seed(a.reseed[pair], seeded);
        for (int w = 0; w < 5; w++) ((uint64_t*)db)[w] = seeded[w];
      }
    } else
      ((uint64_t*)db)[tid] = fk_header_word(tid, ((const uint64_t*)sb)[tid], ((const uint64_t*)db)[tid], a.src.gen, a.dst.gen);
  }
  // the dense part on either side of the overflow area
  fk_copy_words(db + sizeof(SssHdr), sb + sizeof(SssHdr), ((size_t)a.off_pool_tab - sizeof(SssHdr)) / 4, tid);
  fk_copy_words(db + a.off_dur_ring, sb + a.off_dur_ring, (size_t)(a.env_stride - a.off_dur_ring) / 4, tid);
  // the overflow area: each wave takes 64 pool records at a time - a record's mask per lane - and copies the tables that have grown
  for (int p0 = wave * 64; p0 < a.n_pools; p0 += SSS_FK_THREADS) {
    const int p = p0 + lane;
    const uint32_t mask = p < a.n_pools ? (uint32_t)((const SssPoolHdr*)(sb + a.off_pool_hdr))[p].mask : 7u;
    uint64_t grown = __builtin_amdgcn_ballot_w64(mask != 7u);
    while (grown) {  // (wave-uniform)
      const size_t off = (size_t)a.off_pool_tab + (size_t)(p0 + __builtin_ctzll(grown)) * (size_t)a.table_bytes;
      grown &= grown - 1;
      if (lane * 16 < a.table_bytes) ((uint4*)(db + off))[lane] = ((const uint4*)(sb + off))[lane];
    }
  }
  // the observation rows' live prefix
  const FkCounts c = fk_counts(a, s);
  fk_copy_words(a.dst.nodes + (size_t)d * a.n_cap * 3, a.src.nodes + (size_t)s * a.n_cap * 3, (size_t)c.n_nodes * 3, tid);
  fk_copy_words(a.dst.edge_links + (size_t)d * a.ed_cap * 2, a.src.edge_links + (size_t)s * a.ed_cap * 2, (size_t)c.n_edges * 2, tid);
  fk_copy_words(a.dst.dag_ptr + (size_t)d * (a.J_cap + 1), a.src.dag_ptr + (size_t)s * (a.J_cap + 1), (size_t)c.n_jobs + 1, tid);
  fk_copy_words(a.dst.exec_supplies + (size_t)d * a.J_cap, a.src.exec_supplies + (size_t)s * a.J_cap, (size_t)c.n_jobs, tid);
  fk_copy_words(a.dst.obs_i32 + (size_t)d * SSS_OBS_I32, a.src.obs_i32 + (size_t)s * SSS_OBS_I32, SSS_OBS_I32, tid);
  fk_copy_words(a.dst.obs_f64 + (size_t)d * SSS_OBS_F64, a.src.obs_f64 + (size_t)s * SSS_OBS_F64, SSS_OBS_F64 * 2, tid);
  // the timeline rows, an executor per wave at a time
  if (a.src.tl.t && a.dst.tl.t)
    for (int e = wave; e < a.E; e += SSS_FK_THREADS / 64) {
      const size_t sr = (size_t)s * a.E + e, dr = (size_t)d * a.E + e;
      const int count = a.src.tl.count[sr], m = fk_tl_entries(a, count);
      const double* st = a.src.tl.t + sr * (size_t)a.src.tl.cap;
      double* dt = a.dst.tl.t + dr * (size_t)a.dst.tl.cap;
      const int32_t* sj = a.src.tl.job + sr * (size_t)a.src.tl.cap;
      int32_t* dj = a.dst.tl.job + dr * (size_t)a.dst.tl.cap;
      for (int k = lane; k < m; k += 64) dt[k] = st[k], dj[k] = sj[k];
      if (lane == 0) a.dst.tl.count[dr] = count;
    }
}
static int be_launch_env_copy(const SssForkArgs& a, void* stream) {
  hipLaunchKernelGGL(sss_env_copy_kernel, dim3((unsigned)a.n), dim3(SSS_FK_THREADS), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
#endif
