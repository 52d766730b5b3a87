// sss_sim.h - the batched Spark-scheduling simulator, device side (gfx950, wave64).
//
// One wavefront (one 64-thread workgroup) simulates one environment. The env's hot block
// (header, per-executor event slots, commitment list) is staged HBM -> LDS at kernel entry and
// written back at exit. Inside a launch the wave alternates between
//   * serial phases, executed by lane 0 only (the discrete-event logic is one dependent chain
//     per env by construction), and
//   * wave-parallel phases: the event-queue pop (arg-min over one lane per executor), the
//     schedulable-stage scan (one lane per stage, ballot), the observation writer (lanes over
//     stages / edges with ballot prefix compaction), state staging and episode initialisation,
// separated by wave_sync(). Collectives are only issued from wave-uniform control flow; the
// branch conditions come from LDS flags lane 0 publishes before the sync.
//
// What each function restates is cited as ENV:n (reference spark_sched_sim/spark_sched_sim.py),
// TRK:n (components/executor_tracker.py), JOB:n (components/job.py), STG:n (components/stage.py),
// TPCH:n (data_samplers/tpch.py), EVQ:n (components/event.py). Behavioural quirks that must be
// kept are listed in SURVEY.md appendix B; the CPython-set and numpy-Generator models are
// described in DESIGN.md ("Third-party semantics").
//
// No oracle code is used here: this is an independent implementation on different data
// structures (bit masks, flat slot arrays, fixed-capacity set images); tests compare the two.
#pragma once
// -DSSS_WIDE: the instantiation for 65..128 executors (csrc/sss_hip_wide.hip, tests/emu/emu_wide.cpp): 128-entry executor arrays,
// job.local_executors kept as a count, set images of up to 1024 slots, and TWO EXECUTORS PER LANE wherever lanes stand for
// executors. Outside the event chain (the queue's pop, staging at launch boundaries, episode initialisation) a lane simply handles
// both. In the lane-parallel event machinery - fast runs, event batches - a lane speaks for the one of its two executors whose
// pending event comes first (lane_event); the other one's event is an outsider that bounds the window like any event of another
// kind. That costs window length, never correctness: a window may always be cut short, and the event that cut it is its lane's
// first event in the next round. The wave-uniform single-event paths, chunked fulfilment and the pair staging take executor ids
// and list positions, not lanes, and only needed their tables and masks widened. -DSSS_NO_BATCH (either instantiation): every
// event through the one-at-a-time handlers - the reference's control flow restated - for the byte-identity tests.
// -DSSS_TIMELINE (either instantiation; csrc/sss_hip_sim_tl.hip, sss_hip_wide_tl.hip): the kernels that also record the executor
// timelines (tl_append below), as SECOND instantiations under their own names. The ones without it are, instruction for
// instruction, what they were before the recording existed - the launchers pick by whether a timeline is bound.
#ifdef SSS_WIDE
#ifdef SSS_TIMELINE
#define SSS_KNAME(name) name##_wide_tl
#else
#define SSS_KNAME(name) name##_wide
#endif
#else
#ifdef SSS_TIMELINE
#define SSS_KNAME(name) name##_tl
#else
#define SSS_KNAME(name) name
#endif
#endif
#include "../../include/sss.h"
#include "sss_layout.h"
#include <wave_rt.h>  // csrc/wave_rt.h (gfx950) or tests/emu/wave_rt.h (CPU emulator), chosen by -I order

// ------------------------------------------------------------------------------------------
// per-wave context
// ------------------------------------------------------------------------------------------

// LDS of one workgroup (= one env). File-scope objects so that every access is a ds_* instruction
// (a pointer passed through a call would degrade to flat_*). Static part: the hot block and the
// scratch below; dynamic part (g_pool, sized by the host, see SssParams::off_*): the ordered
// active-job list, the job -> cache-slot map, the LDS cache of the ACTIVE jobs' records and stage
// counters (what the event chain touches on every event), and scratch for set images.
// Aliased by the observation writer (sss_sim_observe.h, OBS_*): setA, setB, fc_dst, fc_num, rl_old and rl_seq hold its per-job
// records of a chunk of 64 active jobs. They are scratch of one event-loop round each and the observation is written after the
// step's last round; whoever makes one of them live across the end of a step has to move the writer's records elsewhere.
struct alignas(16) SssScratch {
  uint8_t pool8[8];  // the 8-slot table of the pool that is open (pool_open / pool_close)
  uint8_t pool8b[8]; // ... of a second pool staged next to it (pool_pair_stage)
  // the next raw outputs of the env's PCG64 stream, produced 64 at a time by the whole wave
  // (rng_refill); rng_pos of them are consumed; rng_pos == 64: none buffered, the header holds the
  // generator's state as numpy would have it
  uint64_t rng_buf[64];
  int32_t rng_pos, pad0_[3];
  uint8_t setA[SSS_SET_TABLE];
  uint8_t setB[SSS_SET_TABLE];
  // flags lane 0 publishes for the uniform control flow
  int32_t f_done, f_scan, f_round_continues;
  int32_t m_n_active, m_src_job;  // mailbox for find_schedulable_all
  int32_t n_old_active;
  int32_t events_this_step;
  int32_t events_at_launch;       // ... of which taken by earlier launches (a step cut at its event budget, sss_step_bounded)
  int32_t pending_free;           // job whose cache slot is to be released (-1: none)
  int32_t pinned_job;             // job of the event being handled: its cache slot is not given away
  int32_t sel_job, sel_stage;     // the stage an action names (select_stage_wave -> take_action)
  // the idle executors of pool `idle_key`, found with one ballot right before a lane-0 section that asks for
  // them (publish_idle_mask); consumed by the next get_idle_source_executors, valid for nothing else
  uint32_t idle_key;
  int32_t idle_valid;
  uint64_t idle_mask;
#ifdef SSS_WIDE
  uint64_t idle_mask_hi;          // ... executors 64..127
#endif
  int32_t jobset_mask, f_need_jobtime;
  // the set image of (old active list + active list) only changes when a job arrives or completes:
  // versions of the two lists it was built from (valid within one launch)
  uint32_t active_version, old_version, jobset_old_v, jobset_new_v;
  int32_t jobset_valid;
  int32_t active_dirty;           // the ordered active-job list has changed since it was staged in (env_end writes it back only then)
  uint64_t free_slots;            // bit k set <=> cache slot k is free
  double wall_old;
  uint32_t fc_dst[SSS_MAX_EXEC];  // snapshot of the source's commitments (fulfill_commitments_from_source)
#ifdef SSS_WIDE
  uint32_t fc_seq[SSS_MAX_EXEC];  // their insertion numbers while the snapshot is sorted (fulfil_order_commitments)
#endif
  int16_t fc_num[SSS_MAX_EXEC];
  // the executors that fulfil them, in the order the reference pops them (fulfil_build_list): executor,
  // index of its commitment in the snapshot, and what became of it in a lane-parallel chunk
  uint8_t fi_e[SSS_MAX_EXEC], fi_k[SSS_MAX_EXEC], fi_type[SSS_MAX_EXEC];
  int32_t fi_m, fi_m_par, f_fulfil;
  int32_t fc_n, fc_pad_[3];       // entries of the snapshot
  uint32_t rl_old[SSS_MAX_EXEC];  // batch_released_events: the members' old pools and commitment entries, by rank
  uint8_t rl_idx[SSS_MAX_EXEC];
  uint32_t rl_seq[SSS_MAX_EXEC];
  uint64_t fi_detach;             // executors a chunk detaches from the source's job
  double reset_t;                 // do_reset: arrival time of the next job while the job sequence is drawn in chunks
  int32_t reset_more, reset_pad;
  uint32_t fi_rng_pos, fi_rng_has32, fi_rng_u32, fi_pad;
};

#define SSS_STATIC_LDS_BYTES ((int)(sizeof(SssHot) + sizeof(SssScratch)))

SSS_SHARED SssHot g_hot;
SSS_SHARED SssScratch g_sc;
SSS_SHARED_DYN(g_pool);

// Per-launch context: this env's HBM pointers, the workload-pack pointers and the small parameters.
// All of it is a function of the kernel arguments (every simulator kernel takes SssKernelArgs first)
// and the workgroup id, so any function - inlined or not - reads what it needs from the
// kernel-argument segment: scalar loads the compiler knows to be invariant (they are merged and
// hoisted freely, cost no LDS round trip and no LDS space) plus a little scalar arithmetic.
// `g_c.x` builds the view and uses one member; everything unused folds away.
struct Ctx {
  uint16_t* active_g;
  SssJob* jobs;
  double* t_arrival;
  double* t_completed;
  SssStage* stages;
  float* durations;
  SssPoolHdr* pool_hdr;
  uint8_t* pool_tab;
  double* dur_ring;
  SssPackDev pk;
  SssParams P;
  int E, J_cap, SP;
};
SSS_DEV Ctx ctx_make() {
  const SssKernelArgs* a = (const SssKernelArgs*)SSS_KERNARG_PTR();
  uint8_t* env_base = (uint8_t*)a->B.state + (size_t)wave_env() * (size_t)a->L.env_stride;
  Ctx c;
  c.active_g = (uint16_t*)(env_base + a->L.off_active);
  c.jobs = (SssJob*)(env_base + a->L.off_jobs);
  c.t_arrival = (double*)(env_base + a->L.off_t_arrival);
  c.t_completed = (double*)(env_base + a->L.off_t_completed);
  c.stages = (SssStage*)(env_base + a->L.off_stages);
  c.durations = (float*)(env_base + a->L.off_durations);
  c.pool_hdr = (SssPoolHdr*)(env_base + a->L.off_pool_hdr);
  c.pool_tab = env_base + a->L.off_pool_tab;
  c.dur_ring = (double*)(env_base + a->L.off_dur_ring);
  c.pk = a->pk;
  c.P = a->P;
  c.E = a->L.E, c.J_cap = a->L.J_cap, c.SP = a->L.SP;
  return c;
}
#define g_c (ctx_make())

SSS_DEV void prof3_clear();
SSS_DEV void ctx_init() { prof3_clear(); }

// ---- executor timelines (SssTimeline: the reference's Executor.history, executor.py:21-44) ----
// Recording is a compile-time switch of the kernels: on gfx950 the two functions below are empty unless the unit is compiled with
// -DSSS_TIMELINE. With a run-time test on the bound pointer in the ONE form of each kernel, the fused rollout kernels went from
// 0 / 8 to 6 / 11 spilled vector registers (narrow / wide; the budget tests/test_abi.py holds them to is 8) although the test is a
// scalar branch - the address arithmetic of the appends lives across the event loop. The CPU emulator has no register budget:
// one form, which looks at the pointer. The pointers ride in the kernel-argument segment. A row belongs to one executor
// and is only ever written by the lane that handles that executor's event (lane 0 in the serial handlers, the executor's own
// lane in the batches), with an ordering point between two events of one executor: plain loads and stores.
#if defined(SSS_TIMELINE) || !defined(__HIP__)
#define SSS_TL_RECORDS 1
#else
#define SSS_TL_RECORDS 0
#endif
// Executor.add_history(t, job) (executor.py:34-44): the open entry gets its release time, a new open entry [None, job] follows.
// Entries from index cap on are counted only; every store is guarded by its own index, whatever the count buffer holds.
SSS_DEV void tl_append(int e, double t, int job) {
  if (!SSS_TL_RECORDS) return;
  const SssKernelArgs* a = (const SssKernelArgs*)SSS_KERNARG_PTR();
  double* const tt = a->tl.t;
  if (!tt) return;
  const int cap = a->tl.cap;
  const size_t row = (size_t)wave_env() * (size_t)a->L.E + (size_t)e;
  int32_t* const cnt = a->tl.count + row;
  const int c = *cnt;
  if (c >= 1 && c <= cap) tt[row * (size_t)cap + (size_t)(c - 1)] = t;
  if (c >= 0 && c < cap) tt[row * (size_t)cap + (size_t)c] = __builtin_nan(""), a->tl.job[row * (size_t)cap + (size_t)c] = job;
  *cnt = c + 1;
}
// Executor.__init__ (executor.py:25): history = [[None, -1]] - the row of executor e starts over (episode initialisation)
SSS_DEV void tl_reset_row(int e) {
  if (!SSS_TL_RECORDS) return;
  const SssKernelArgs* a = (const SssKernelArgs*)SSS_KERNARG_PTR();
  double* const tt = a->tl.t;
  if (!tt) return;
  const size_t row = (size_t)wave_env() * (size_t)a->L.E + (size_t)e;
  tt[row * (size_t)a->tl.cap] = __builtin_nan(""), a->tl.job[row * (size_t)a->tl.cap] = -1;  // (cap >= 1: sss_bind_timeline)
  a->tl.count[row] = 1;
}

#define SSS_SRC_ID 0  // which source file a failed check sits in: 0 = this file, 1.. = the parts below in include order
#define H (g_hot.h)
#ifdef SSS_CHECK_TRACE  // emulator debugging: say which invariant broke
#include <stdio.h>
#define FAIL(code)                                                                          \
  do {                                                                                      \
    if (H.err == 0) fprintf(stderr, "[FAIL] line %d: code %d\n", __LINE__, (int)(code)), H.err = (code), H.err_line = (uint64_t)SSS_SRC_ID * 100000u + __LINE__; \
  } while (0)
#else
#define FAIL(code)                                         \
  do {                                                     \
    if (H.err == 0) H.err = (code), H.err_line = (uint64_t)SSS_SRC_ID * 100000u + __LINE__; \
  } while (0)
#endif
#ifdef SSS_CHECK_TRACE
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      if (H.err == 0) fprintf(stderr, "[CHECK] line %d: %s\n", __LINE__, #cond);         \
      FAIL(SSS_ERR_INVARIANT);                                                          \
    }                                                                                   \
  } while (0)
#else
#define CHECK(cond)                          \
  do {                                       \
    if (!(cond)) FAIL(SSS_ERR_INVARIANT);     \
  } while (0)
#endif

#if defined(__HIP_DEVICE_COMPILE__) || defined(__clang__)
#define SSS_UNROLL4 _Pragma("unroll 4")
#define SSS_UNROLL8 _Pragma("unroll 8")
#else
#define SSS_UNROLL4
#define SSS_UNROLL8
#endif

#ifdef SSS_BATCH_STATS  // emulator-only census of why rounds end (tests/emu, never in the product build)
extern "C" { extern long long sss_batch_stats[128]; }
#define STAT(i, v) ((void)(wave_lane() == 0 ? (sss_batch_stats[i] += (v)) : 0))
#else
#define STAT(i, v) ((void)0)
#endif

#include "sss_prof.h"  // PROF3 scopes: empty unless a timing build defines SSS_EVPROF3
#if defined(SSS_CHECK_TRACE) && defined(SSS_UTRACE)
#define UTRACE(tag) do { if (wave_lane() < 2 && getenv("SSS_UTRACE")) fprintf(stderr, "[u] lane %d %s\n", wave_lane(), tag); } while (0)
#else
#define UTRACE(tag) ((void)0)
#endif

// ---- LDS pool views ----
#define LENW_LEN 0x3FFFFFFF  // list length in a duration descriptor (bit 30: warmup_delay is added)
#define SLOT_NONE 255
SSS_DEV uint16_t* lds_active() { return (uint16_t*)(g_pool + g_c.P.off_active); }
SSS_DEV uint8_t* lds_slot_of() { return g_pool + g_c.P.off_slot_of; }
SSS_DEV uint16_t* lds_keys() { return (uint16_t*)(g_pool + g_c.P.off_keys); }
SSS_DEV uint16_t* lds_jobset() { return (uint16_t*)(g_pool + g_c.P.off_jobset); }
SSS_DEV SssJob* lds_cjobs() { return (SssJob*)(g_pool + g_c.P.off_cjobs); }
SSS_DEV SssStage* lds_cstages() { return (SssStage*)(g_pool + g_c.P.off_cstages); }
SSS_DEV float* lds_cdur() { return (float*)(g_pool + g_c.P.off_cdur); }
SSS_DEV SssExDesc* lds_exdesc() { return (SssExDesc*)(g_pool + g_c.P.off_exdesc); }
SSS_DEV uint16_t* lds_old_active() { return (uint16_t*)(g_pool + g_c.P.off_old_active); }
SSS_DEV uint16_t* lds_slot_job() { return (uint16_t*)(g_pool + g_c.P.off_slot_job); }  // job held by a cache slot
SSS_DEV uint8_t* lds_slot_ref() { return g_pool + g_c.P.off_slot_ref; }                // pending events that name the slot

// record of job j: its LDS cache slot if it has one, else the HBM copy
SSS_DEV SssJob* jobp(int j) {
  int s = lds_slot_of()[j];
  return s != SLOT_NONE ? lds_cjobs() + s : g_c.jobs + j;
}
SSS_DEV SssStage* stgp(int j, int st) {
  int s = lds_slot_of()[j];
  return s != SLOT_NONE ? lds_cstages() + s * g_c.SP + st : g_c.stages + j * g_c.SP + st;
}
SSS_DEV float* durp(int j, int st) {  // stage.most_recent_duration (observed as f32, ENV:381)
  int s = lds_slot_of()[j];
  return s != SLOT_NONE ? lds_cdur() + s * g_c.SP + st : g_c.durations + j * g_c.SP + st;
}

// all three at once (one look-up of the job's slot). A view stays valid until the next cache_acquire / cache_release:
// those can move a job's records between HBM and LDS
struct JobView {
  SssJob* job;
  SssStage* st;  // [stage]
  float* dur;    // [stage]
};
SSS_DEV JobView jobview(int j) {
  const int s = lds_slot_of()[j];
  JobView v;
  if (s != SLOT_NONE)
    v.job = lds_cjobs() + s, v.st = lds_cstages() + s * g_c.SP, v.dur = lds_cdur() + s * g_c.SP;
  else
    v.job = g_c.jobs + j, v.st = g_c.stages + j * g_c.SP, v.dur = g_c.durations + j * g_c.SP;
  return v;
}

// pool keys
SSS_DEV uint32_t key_job_pool(int j) { return (uint32_t)(j + 1) << 8; }
SSS_DEV uint32_t key_stage_pool(int j, int s) { return ((uint32_t)(j + 1) << 8) | (uint32_t)(s + 1); }
SSS_DEV int key_job(uint32_t k) { return k == POOL_NONE ? -1 : (int)(k >> 8) - 1; }   // pool_key[0], -1 = None
SSS_DEV int key_stage(uint32_t k) { return k == POOL_NONE ? -1 : (int)(k & 0xFF) - 1; }  // pool_key[1], -1 = None
SSS_DEV int pool_index(uint32_t k) {
  int j = key_job(k), s = key_stage(k);
  if (j < 0) return 0;
  if (s < 0) return 1 + j;
  return 1 + g_c.J_cap + j * g_c.SP + s;
}
// The same rule with the env's dimensions handed in (policy_hash_direct: a lane whose env is not the wave's). Written out a second
// time: with pool_index calling this one, the reset and fused rollout kernels came out with another register allocation
// (profiles/policy_hash_launch.md section 4), and tests/test_abi.py holds theirs.
SSS_DEV int pool_index_in(uint32_t k, int J_cap, int SP) {
  int j = key_job(k), s = key_stage(k);
  if (j < 0) return 0;
  if (s < 0) return 1 + j;
  return 1 + J_cap + j * SP + s;
}

// job.local_executors (JOB:81-89) is only ever counted (TPCH:217, the executor-level key). Up to 64 executors it is kept as a
// bit mask (the event batches update it with lane masks); the wide instantiation keeps the count itself in the same field.
#ifdef SSS_WIDE
SSS_DEV int local_count(uint64_t m) { return (int)m; }
SSS_DEV uint64_t local_with(uint64_t m, int) { return m + 1; }
SSS_DEV uint64_t local_without(uint64_t m, int) { return m - 1; }
SSS_DEV bool local_has(uint64_t m, int) { return m != 0; }
// several lanes at once (event batches); the count lives in the low word and never carries or borrows out of it
SSS_DEV void local_atomic_attach(SssJob* jp, int) { lane_atomic_add_u32((uint32_t*)&jp->local_mask, 1u); }
SSS_DEV void local_atomic_detach(SssJob* jp, int) { lane_atomic_add_u32((uint32_t*)&jp->local_mask, 0u - 1u); }
// a group of executors that leaves a job together (lane 0): gathered one by one, taken off the job's record at once
struct LocalGroup { uint32_t n; };
SSS_DEV LocalGroup local_group() { return LocalGroup{0u}; }
SSS_DEV void local_group_add(LocalGroup& g, int) { g.n++; }
SSS_DEV void local_group_detach(SssJob* jp, const LocalGroup& g) {
  CHECK(jp->local_mask >= g.n);
  jp->local_mask -= g.n;
}
#else
SSS_DEV int local_count(uint64_t m) { return popc64(m); }
SSS_DEV uint64_t local_with(uint64_t m, int e) { return m | bit64(e); }
SSS_DEV uint64_t local_without(uint64_t m, int e) { return m & ~bit64(e); }
SSS_DEV bool local_has(uint64_t m, int e) { return (m & bit64(e)) != 0; }
SSS_DEV void local_atomic_attach(SssJob* jp, int e) { lane_atomic_or_u64(&jp->local_mask, bit64(e)); }
SSS_DEV void local_atomic_detach(SssJob* jp, int e) { lane_atomic_and_u64(&jp->local_mask, ~bit64(e)); }
struct LocalGroup { uint64_t m; };
SSS_DEV LocalGroup local_group() { return LocalGroup{0ull}; }
SSS_DEV void local_group_add(LocalGroup& g, int e) { g.m |= bit64(e); }
SSS_DEV void local_group_detach(SssJob* jp, const LocalGroup& g) {
  CHECK((jp->local_mask & g.m) == g.m);
  jp->local_mask &= ~g.m;
}
#endif

// ---- executors per lane ----
// Where lanes stand for executors: one each up to 64 executors; in the wide instantiation lane l holds executors l and l + 64
// (slots beyond num_executors are empty: t = +inf, EV_NONE).
#ifdef SSS_WIDE
#define SSS_EPL 2
#else
#define SSS_EPL 1
#endif
SSS_DEV int head_lane(int ex) { return ex & 63; }  // the lane that speaks for executor `ex`
// The pending event a lane speaks for in the lane-parallel event machinery, its executor, and - wide - the time of the lane's
// OTHER event, which takes no part: it bounds every window like an event of another kind (t_alt = +inf when there is none,
// and always with one executor per lane).
struct LaneEvent {
  SssEvSlot sl;
  int ex;
  double t_alt;
};
SSS_DEV LaneEvent lane_event(int lane) {
  LaneEvent le;
#ifdef SSS_WIDE
  const SssEvSlot a = g_hot.ev[lane], b = g_hot.ev[lane + 64];
  const bool b_first = b.t < a.t || (b.t == a.t && b.seq < a.seq);  // heapq's order (EVQ:35); empty slots hold +inf
  le.sl = b_first ? b : a, le.ex = b_first ? lane + 64 : lane, le.t_alt = b_first ? a.t : b.t;
#else
  le.sl = g_hot.ev[lane], le.ex = lane, le.t_alt = __builtin_inf();
#endif
  return le;
}
SSS_DEV double min_f64(double a, double b) { return b < a ? b : a; }

// ---- the device code by concern (each part cites what it restates; the order is the dependency order) ----
#include "sss_sim_rng.h"  // the numpy Generator(PCG64) stream: SeedSequence, PCG64, Lemire bounded ints, ziggurat exponential, FDLIBM log1p / exp; wave-wide jump-ahead refill
#include "sss_sim_pyset.h"  // CPython 3.10 set images (executor pools, the job-id set of the reward): add / remove / pop / resize / copy, lane-0 and wave-wide forms
#include "sss_sim_tracker.h"  // ExecutorTracker restated: commitments, pool records, moving an executor between two pools (pool_pair_*)
#include "sss_sim_jobs.h"  // jobs / stages, the task-duration sampler, the serial schedulable-stage search, executor movement (lane 0)
#include "sss_sim_fulfil.h"  // lane-parallel fulfilment of commitments
#include "sss_sim_events.h"  // the one-at-a-time event handlers (lane 0), the wave-parallel queue pop, the LDS job cache
#include "sss_sim_fast_run.h"  // the fast run: consecutive "task finished, its stage has more tasks" events in registers
#include "sss_sim_batches.h"  // lane-parallel batches of released and of arriving executors
#include "sss_sim_lean.h"  // one released / one arriving executor with wave-uniform control flow; the flush of a completing job
#include "sss_sim_observe.h"  // the wave-parallel schedulable-stage scan and the observation writer
#include "sss_sim_env.h"  // staging at launch boundaries, the pieces of a step (action, reward), the event loop, episode initialisation, do_step
#undef SSS_SRC_ID
#define SSS_SRC_ID 0
// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------

// reset envs whose mask byte is non-zero (mask == nullptr: all)
SSS_KERNEL void SSS_KNAME(sss_reset_kernel)(SssKernelArgs a, const uint64_t* seeds, const double* time_limits, const uint8_t* mask) {
  int env = wave_env();
  if (mask && !mask[env]) return;
  uint8_t* base = (uint8_t*)a.B.state + (size_t)env * a.L.env_stride;
  ctx_init();
  env_begin(base);
  do_reset(a.L, seeds[env], time_limits ? time_limits[env] : __builtin_inf());
  write_observation(a.L, a.B, env, 0.0);
  env_end(base);
}

// one step() per env; with auto_reset != 0 an env that is terminated at entry starts its next
// episode instead (seed += seed_stride), like a vector env in "next-step" autoreset mode
SSS_DEV void step_env(const SssKernelArgs& a, const int32_t* stage_idx, const int32_t* num_exec, int auto_reset, uint64_t seed_stride, int budget, uint8_t* ready) {
  int env = wave_env();
  if (stage_idx[env] == SSS_SKIP_ENV) return;  // wave-uniform: the env is not touched at all
  uint8_t* base = (uint8_t*)a.B.state + (size_t)env * a.L.env_stride;
  ctx_init();
  env_begin(base);
  double reward = 0.0;
  bool yielded = false;
  // the ballot doubles as the barrier between "all lanes read the header" and lane 0 rewriting it
  bool start_next_episode = wave_ballot(auto_reset && g_hot.h.terminated && !g_hot.h.err) != 0;
  if (start_next_episode) {
    do_reset(a.L, g_hot.h.seed + seed_stride, g_hot.h.time_limit);
  } else {
    reward = do_step(stage_idx[env], num_exec[env], budget, &yielded);
  }
  if (!yielded) write_observation(a.L, a.B, env, reward);  // (a step that goes on in the next launch has no observation yet)
  if (ready && wave_lane() == 0) ready[env] = yielded ? 0 : 1;
  env_end(base);
  prof3_flush();
}
SSS_KERNEL void SSS_KNAME(sss_step_kernel)(SssKernelArgs a, const int32_t* stage_idx, const int32_t* num_exec, int auto_reset, uint64_t seed_stride) {
  step_env(a, stage_idx, num_exec, auto_reset, seed_stride, 0, nullptr);
}
// sss_step_bounded: the same with an event budget per launch. A launch of sss_step_kernel ends with its slowest env - one with
// 170 events in its step where the mean is 21 (profiles/r04_bench.md) - while the other waves' SIMDs idle. Here an env whose step
// has taken `budget` events stops at the top of its next round (mid_step in its header, ready[env] = 0), the launch ends, and the
// next launch continues that step (its action arguments are not looked at) while the other envs take their next steps. Every
// env's trajectory is the one sss_step_kernel produces; what changes is which launch an env's k-th step ends in.
SSS_KERNEL void SSS_KNAME(sss_step_bounded_kernel)(SssKernelArgs a, const int32_t* stage_idx, const int32_t* num_exec, int auto_reset, uint64_t seed_stride,
                                                   int budget, uint8_t* ready) {
  step_env(a, stage_idx, num_exec, auto_reset, seed_stride, budget, ready);
}

// ------------------------------------------------------------------------------------------
// on-device policies: the build's batched counterparts of the reference's heuristic plugins.
// They read the same quantities a `Scheduler.schedule(obs)` plugin gets from the observation
// (per-job schedulable / frontier stages, exec_supplies, num_committable_execs, source_job_idx),
// but straight from the env state, so that no observation round trip is needed.
// ------------------------------------------------------------------------------------------

SSS_DEV int obs_num_committable() {
  uint32_t srck = g_hot.h.curr_source;
  if (srck == POOL_NONE) return 0;
  int p = pool_index(srck);
  return (int)g_c.pool_hdr[p].used - (int)g_c.pool_hdr[p].commit_from;
}

// find_stage of one job: its first schedulable stage with no active parent, else its first schedulable stage, else -1
SSS_DEV int find_stage_dev(uint64_t sm, uint64_t act, int gs) {
  int best = -1;
  uint64_t m = sm;
  while (m) {
    int s = ctz64(m);
    m &= m - 1;
    if ((g_c.pk.stage_parent_mask[gs + s] & act) == 0) {
      best = s;
      break;
    }
  }
  if (best < 0 && sm) best = ctz64(sm);
  return best;
}

// RoundRobinScheduler.schedule (reference schedulers/heuristics/round_robin.py:14-49 with
// find_stage / preprocess_obs of heuristics/utils.py:5-37). All lanes; results are uniform.
SSS_DEV void policy_fair(bool dynamic_partition, int& stage_idx, int& num_exec) {
  int lane = wave_lane();
  // shared state is read up front; at least one collective follows before anything returns
  int A = g_hot.h.n_active;
  uint32_t srck = g_hot.h.curr_source;
  int ncommit = obs_num_committable();
  int src_job = (srck == POOL_NONE || srck == POOL_COMMON) ? -1 : key_job(srck);
  int denom = A > 1 ? A : 1;
  int cap = dynamic_partition ? (g_c.E + denom - 1) / denom : g_c.E;  // int(ceil(E / max(1, A)))
  int src_rank = -1, first_rank = -1, first_sup = 0;
  uint32_t base = 0;
  int n_chunks = (A + 63) / 64;
  if (n_chunks == 0) n_chunks = 1;
  for (int ch = 0; ch < n_chunks; ch++) {
    int k = ch * 64 + lane;
    bool valid = k < A;
    int j = valid ? (int)lds_active()[k] : 0;
    uint64_t sm = 0, act = 0;
    int sup = 0, gs = 0;
    if (valid) {
      const SssJob& job = (*jobp(j));
      sm = job.sched_mask, act = job.active_mask, sup = job.supply, gs = job.gs_base;
    }
    int best = find_stage_dev(sm, act, gs);
    uint32_t cnt = (uint32_t)popc64(sm);
    uint32_t excl = wave_scan_excl_u32(cnt);
    uint32_t total = wave_sum_u32(cnt);
    uint32_t abs_rank = base + excl + (best >= 0 ? (uint32_t)popc64(sm & (bit64(best) - 1)) : 0u);
    bool is_src = valid && j == src_job;
    uint64_t m_src = wave_ballot(is_src && best >= 0);
    uint64_t m_el = wave_ballot(valid && best >= 0 && !(sup >= cap || is_src));
    if (m_src != 0 && src_rank < 0) src_rank = (int)wave_bcast_u32(abs_rank, ctz64(m_src));
    if (m_el != 0 && first_rank < 0) {
      int l = ctz64(m_el);
      first_rank = (int)wave_bcast_u32(abs_rank, l);
      first_sup = (int)wave_bcast_u32((uint32_t)sup, l);
    }
    base += total;
  }
  if (src_rank >= 0) {
    stage_idx = src_rank, num_exec = ncommit;
  } else if (first_rank >= 0) {
    int room = cap - first_sup;
    stage_idx = first_rank, num_exec = ncommit < room ? ncommit : room;
  } else {
    stage_idx = -1, num_exec = ncommit;
  }
  if (num_exec < 1) num_exec = 1;
}

// ---- weighted fair and SJF-CP: the stronger heuristics of the Decima paper (Mao et al., SIGCOMM 2019, 7.2) ----
// Both are defined on the observation (schedulers.py WeightedFairScheduler / SJFCPScheduler), and must agree with
// those host plugins bit for bit. work(n) = f64(nodes[n,0]) * f64(nodes[n,1]) = (double)(float)remaining * (double)duration is
// one exact product of two f32 values, so only the order of the sums is fixed: a job's work W_j is summed from 0.0 over its
// active stages in ascending stage id (the order of its node rows), the weighted-fair total S over the active jobs in active
// order. f64 adds and multiplies only (the unit builds with -ffp-contract=off), no pow.

SSS_DEV double stage_work(const JobView& v, int s) { return (double)(float)v.st[s].remaining * (double)v.dur[s]; }

SSS_DEV double job_work(const JobView& v, uint64_t act) {
  double w = 0.0;
  for (uint64_t m = act; m; m &= m - 1) w += stage_work(v, ctz64(m));
  return w;
}

// w_j = max(W_j, 1)^alpha by repeated multiplication (host and device pow differ in the last ulp), alpha in [-4, 4]
SSS_DEV double wfair_weight(double W, int alpha) {
  if (alpha == 0) return 1.0;
  const double x = W > 1.0 ? W : 1.0;
  const int k = alpha < 0 ? -alpha : alpha;
  double p = x;
  for (int i = 1; i < k; i++) p *= x;
  return alpha > 0 ? p : 1.0 / p;
}

// weighted fair: RoundRobinScheduler's structure with the per-job cap min(E, max(1, ceil(E * w_j / S))) in place of
// ceil(E / A). All lanes; results are uniform.
SSS_DEV void policy_wfair(int alpha, int& stage_idx, int& num_exec) {
  int lane = wave_lane();
  int A = g_hot.h.n_active;
  uint32_t srck = g_hot.h.curr_source;
  int ncommit = obs_num_committable();
  int src_job = (srck == POOL_NONE || srck == POOL_COMMON) ? -1 : key_job(srck);
  const int E = g_c.E;
  int n_chunks = (A + 63) / 64;
  if (n_chunks == 0) n_chunks = 1;
  // pass 1 - lanes over jobs: the weights; S summed left to right by wave-uniform lane reads (no LDS array)
  double S = 0.0, w_last = 1.0;
  for (int ch = 0; ch < n_chunks; ch++) {
    int k = ch * 64 + lane;
    double w = 1.0;
    if (k < A) {
      const JobView v = jobview(lds_active()[k]);
      w = wfair_weight(job_work(v, v.job->active_mask), alpha);
    }
    int n = A - ch * 64 < 64 ? A - ch * 64 : 64;
    for (int l = 0; l < n; l++) S += wave_readlane_f64(w, l);
    w_last = w;
  }
  // pass 2 - find_stage per job, the caps, the first eligible job (as policy_fair); one chunk keeps its weights in registers
  int src_rank = -1, first_rank = -1, first_sup = 0, first_cap = 0;
  uint32_t base = 0;
  for (int ch = 0; ch < n_chunks; ch++) {
    int k = ch * 64 + lane;
    bool valid = k < A;
    int j = valid ? (int)lds_active()[k] : 0;
    uint64_t sm = 0, act = 0;
    int sup = 0, gs = 0, cap = 0;
    if (valid) {
      const JobView v = jobview(j);
      sm = v.job->sched_mask, act = v.job->active_mask, sup = v.job->supply, gs = v.job->gs_base;
      const double w = n_chunks == 1 ? w_last : wfair_weight(job_work(v, act), alpha);
      const double c = __builtin_ceil(((double)E * w) / S);
      cap = c < 1.0 ? 1 : (c > (double)E ? E : (int)c);
    }
    int best = find_stage_dev(sm, act, gs);
    uint32_t cnt = (uint32_t)popc64(sm);
    uint32_t excl = wave_scan_excl_u32(cnt);
    uint32_t total = wave_sum_u32(cnt);
    uint32_t abs_rank = base + excl + (best >= 0 ? (uint32_t)popc64(sm & (bit64(best) - 1)) : 0u);
    bool is_src = valid && j == src_job;
    uint64_t m_src = wave_ballot(is_src && best >= 0);
    uint64_t m_el = wave_ballot(valid && best >= 0 && !(sup >= cap || is_src));
    if (m_src != 0 && src_rank < 0) src_rank = (int)wave_bcast_u32(abs_rank, ctz64(m_src));
    if (m_el != 0 && first_rank < 0) {
      int l = ctz64(m_el);
      first_rank = (int)wave_bcast_u32(abs_rank, l);
      first_sup = (int)wave_bcast_u32((uint32_t)sup, l);
      first_cap = (int)wave_bcast_u32((uint32_t)cap, l);
    }
    base += total;
  }
  if (src_rank >= 0) {
    stage_idx = src_rank, num_exec = ncommit;
  } else if (first_rank >= 0) {
    int room = first_cap - first_sup;
    stage_idx = first_rank, num_exec = ncommit < room ? ncommit : room;
  } else {
    stage_idx = -1, num_exec = ncommit;
  }
  if (num_exec < 1) num_exec = 1;
}

// SJF-CP: the job of least work W_j among those with a schedulable stage (ties: earliest active position), inside it the
// schedulable stage at the head of the longest critical path CP(n) = work(n) + max over active children CP(c) (ties: lowest
// stage id), all committable executors. All lanes; results are uniform.
SSS_DEV void policy_sjfcp(int& stage_idx, int& num_exec) {
  int lane = wave_lane();
  int A = g_hot.h.n_active;
  int ncommit = obs_num_committable();
  int n_chunks = (A + 63) / 64;
  if (n_chunks == 0) n_chunks = 1;
  // lanes over jobs: arg-min of (W_j, position). W_j >= 0, so its bit pattern orders like its value
  uint64_t best_key = ~0ull;
  int best_j = -1;
  uint32_t best_base = 0, base = 0;  // best_base: rank of the chosen job's first schedulable node among all of them
  for (int ch = 0; ch < n_chunks; ch++) {
    int k = ch * 64 + lane;
    bool valid = k < A;
    int j = valid ? (int)lds_active()[k] : 0;
    uint64_t sm = 0;
    double W = 0.0;
    if (valid) {
      const JobView v = jobview(j);
      sm = v.job->sched_mask;
      W = job_work(v, v.job->active_mask);
    }
    uint32_t cnt = (uint32_t)popc64(sm);
    uint32_t excl = wave_scan_excl_u32(cnt);
    uint32_t total = wave_sum_u32(cnt);
    bool cand = valid && sm != 0;
    uint64_t key = cand ? f64_bits(W) : ~0ull;
    uint64_t mn = wave_min_u64(key);
    uint64_t hit = wave_ballot(cand && key == mn);
    if (hit != 0 && mn < best_key) {  // strictly less: an equal W in a later chunk comes later in active order
      int l = ctz64(hit);
      best_key = mn, best_j = (int)wave_bcast_u32((uint32_t)j, l), best_base = base + wave_bcast_u32(excl, l);
    }
    base += total;
  }
  stage_idx = -1, num_exec = ncommit;
  if (best_j >= 0) {
    // lanes over the chosen job's stages: CP by relaxation. Each round is a Jacobi sweep (cp of every child read from the
    // previous round); from cp = work, a stage's value is final once the rounds reach its height, and a max is exact, so
    // the fixed point is the same bits in any order. A DAG of at most 64 stages settles within 64 rounds.
    const JobView v = jobview(best_j);
    const uint64_t act = v.job->active_mask, sm = v.job->sched_mask;
    const bool mine = (act >> lane) & 1;
    const double w = mine ? stage_work(v, lane) : 0.0;
    const uint64_t kids = mine ? g_c.pk.stage_child_mask[v.job->gs_base + lane] & act : 0;
    double cp = w;
    for (int r = 0; r <= 64; r++) {
      double mx = 0.0;  // CP >= 0: max(0, max over children) = max over children
      uint64_t rem = kids;
      while (wave_ballot(rem != 0)) {
        const bool take = rem != 0;
        const int c = take ? ctz64(rem) : lane;
        rem &= rem - 1;
        const double vc = wave_bcast_f64(cp, c);
        if (take && vc > mx) mx = vc;
      }
      const double nc = kids ? w + mx : w;
      const bool changed = wave_ballot(f64_bits(nc) != f64_bits(cp)) != 0;
      cp = nc;
      if (!changed) break;
    }
    // the schedulable stage of largest CP, lowest id on ties: arg-min of the complemented bit pattern
    const bool cand = (sm >> lane) & 1;
    const uint64_t key = cand ? ~f64_bits(cp) : ~0ull;
    const uint64_t mn = wave_min_u64(key);
    const uint64_t hit = wave_ballot(cand && key == mn);
    if (hit != 0) stage_idx = (int)best_base + popc64(sm & (bit64(ctz64(hit)) - 1));
  }
  if (num_exec < 1) num_exec = 1;
}

SSS_DEV uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the build's counter-based uniform-random policy, keyed (episode seed, step in episode); mirrors
// hash_policy in tests/golden/make_golden.py. SURVEY 8(d) C2: stage uniform over the schedulable
// stages, num_exec uniform in [1, num_committable]; `p_none_permille` adds stage_idx = -1 draws.
// The policy is two parts. hash_action is the pure mapping from what the policy sees of an env to its action - the one
// definition of the arithmetic; the two functions after it only differ in where they fetch those inputs from. (`step` is the
// header's ep_steps, widened by the caller: policy_hash widens it where it always has, ahead of its ordering point, and the fused
// rollout kernels keep their code, scalar spills included - profiles/policy_hash_launch.md section 4.)
SSS_DEV void hash_action(uint64_t seed, uint64_t step, int n_sched, int ncommit, int p_none_permille, int& stage_idx, int& num_exec) {
  uint64_t h = splitmix64((seed << 32) ^ step), h2 = splitmix64(h), h3 = splitmix64(h2);
  if (n_sched == 0 || (int)(h3 % 1000) < p_none_permille)
    stage_idx = -1;
  else
    stage_idx = (int)(h % (uint64_t)n_sched);
  num_exec = 1 + (int)(h2 % (uint64_t)(ncommit > 0 ? ncommit : 1));
}
// ... from the env the wave has staged (the header in LDS, the pool records through g_c): the fused rollout kernels
SSS_DEV void policy_hash(int p_none_permille, int& stage_idx, int& num_exec) {
  uint64_t seed = g_hot.h.seed;
  uint64_t step = (uint64_t)g_hot.h.ep_steps;
  int n_sched = g_hot.h.n_sched;
  int ncommit = obs_num_committable();
  wave_sync();  // reads above vs. lane 0's writes in the step that follows
  hash_action(seed, step, n_sched, ncommit, p_none_permille, stage_idx, num_exec);
}
// ... from the HBM image of env `env`, by one lane that stages nothing: two dependent loads (four header words, then the source
// pool's record - none when there is no source), no LDS, no collective. The env's regions are found through the layout in `a`,
// not through g_c, which describes the one env of a wave: here every lane may have an env of its own (sss_policy_hash_kernel).
SSS_DEV void policy_hash_direct(const SssKernelArgs& a, int env, int p_none_permille, int& stage_idx, int& num_exec) {
  const uint8_t* base = (const uint8_t*)a.B.state + (size_t)env * (size_t)a.L.env_stride;
  const auto* hd = SSS_AS_HBM(SssHdr, base);  // (the hot block, header first, opens the env's image)
  const uint64_t seed = hd->seed;
  const uint64_t step = (uint64_t)hd->ep_steps;
  const int n_sched = hd->n_sched;
  const uint32_t srck = hd->curr_source;
  int ncommit = 0;
  if (srck != POOL_NONE) {
    // of the pool's 16-byte record the word that holds used | commit_from << 16, as the observation writer reads it
    const auto* rec = SSS_AS_HBM(SssPoolHdr, base + a.L.off_pool_hdr) + pool_index_in(srck, a.L.J_cap, a.L.SP);
    const uint32_t used_cf = *SSS_AS_HBM(uint32_t, &rec->used);
    ncommit = (int)(uint16_t)used_cf - (int)(int16_t)(used_cf >> 16);
  }
  hash_action(seed, step, n_sched, ncommit, p_none_permille, stage_idx, num_exec);
}

enum { SSS_POLICY_FAIR = 0, SSS_POLICY_FIFO = 1, SSS_POLICY_HASH = 2, SSS_POLICY_WFAIR = 3, SSS_POLICY_SJFCP = 4 };
#define SSS_POLICY_HASH_THREADS 256  // envs per workgroup of sss_policy_hash_kernel (below; its launchers: sss_hip_sim.hip, sss_hip_wide.hip)

// kHeuristics: with weighted fair / SJF-CP (ids 3, 4). Without them the code is fair / FIFO / hash only, so that the rollout
// kernel those run in keeps its register allocation (see sss_rollout_heur_kernel)
template <bool kHeuristics = true>
SSS_DEV void run_policy(int policy, int param, int& stage_idx, int& num_exec) {
  PROF3(29);
  if (policy == SSS_POLICY_HASH)
    policy_hash(param, stage_idx, num_exec);
  else if (kHeuristics && policy == SSS_POLICY_WFAIR)
    policy_wfair(param, stage_idx, num_exec);
  else if (kHeuristics && policy == SSS_POLICY_SJFCP)
    policy_sjfcp(stage_idx, num_exec);
  else
    policy_fair(policy == SSS_POLICY_FAIR, stage_idx, num_exec);
}

// writes one action per env into stage_idx / num_exec (for sss_step)
#ifndef SSS_TIMELINE  // (reads the state only: there is no recording form of it)
SSS_KERNEL void SSS_KNAME(sss_policy_kernel)(SssKernelArgs a, int policy, int param, int32_t* stage_idx, int32_t* num_exec) {
  int env = wave_env();
  int si, ne;
  if (policy == SSS_POLICY_HASH) {
    // The hash policy needs nothing staged. The launchers of the gfx950 build send it to sss_policy_hash_kernel below and never
    // get here; the CPU emulator launches this kernel for every policy and so runs the same loads, on every lane of the wave.
    policy_hash_direct(a, env, param, si, ne);
  } else {
    uint8_t* base = (uint8_t*)a.B.state + (size_t)env * a.L.env_stride;
    ctx_init();
    env_begin_readonly(base);
    run_policy(policy, param, si, ne);
  }
  if (wave_lane() == 0) stage_idx[env] = si, num_exec[env] = ne;
}
// The hash policy with a thread per env: a workgroup per env above means 4096 dispatches, each staging the header, the slot
// map and the active-job list, for four header words and one pool record. Here 256 envs share a workgroup, nothing is staged
// and no LDS is asked for. (No emulator form: there a "kernel" is a wave with one env.)
#ifdef __HIP__
extern "C" __global__ __launch_bounds__(SSS_POLICY_HASH_THREADS) void SSS_KNAME(sss_policy_hash_kernel)(SssKernelArgs a, int num_envs, int param, int32_t* stage_idx,
                                                                                                     int32_t* num_exec) {
  const int env = (int)(blockIdx.x * SSS_POLICY_HASH_THREADS + threadIdx.x);
  if (env >= num_envs) return;
  int si, ne;
  policy_hash_direct(a, env, param, si, ne);
  stage_idx[env] = si, num_exec[env] = ne;
}
#endif
#endif

// n_steps x (policy -> step -> observe) per env in one launch; the env's hot block and job cache
// stay in LDS in between. Every step still writes the full observation, as the reference's step() does.
// the body of the fused rollout kernels (a macro, not a function: sss_rollout_kernel keeps the code generation it had alone)
#define ROLLOUT_BODY(kHeuristics) \
  int env = wave_env(); \
  uint8_t* base = (uint8_t*)a.B.state + (size_t)env * a.L.env_stride; \
  ctx_init(); \
  env_begin(base); \
  for (int it = 0; it < n_steps; it++) { \
    bool over = wave_ballot(g_hot.h.terminated || g_hot.h.need_reset) != 0; \
    double reward = 0.0; \
    if (over) { \
      if (!auto_reset || wave_ballot(g_hot.h.err != 0) != 0) break; /* failed envs stay failed */ \
      do_reset(a.L, g_hot.h.seed + seed_stride, g_hot.h.time_limit); \
    } else { \
      int si, ne; \
      run_policy<kHeuristics>(policy, param, si, ne); \
      reward = do_step<true>(si, ne); \
    } \
    write_observation(a.L, a.B, env, reward); \
    wave_sync(); \
  } \
  env_end(base); \
  prof3_flush();

// On the GPU the fused rollout is two kernels: sss_rollout_kernel for fair / FIFO / hash, sss_rollout_heur_kernel for every
// policy (the launchers pick it for ids 3 and 4). Inlined into the one kernel, the weighted-fair / SJF-CP bodies changed its
// register allocation and pushed the wide instantiation past its spill budget (tests/test_abi.py); apart, the existing policies
// run the code they ran before. (A call instead of inlining is no way out: a callee cannot read the kernel-argument segment
// that g_c is built from.) The CPU emulator has no register budget and runs every policy through sss_rollout_kernel.
#ifdef __HIP__
#define SSS_ROLLOUT_HEURISTICS false
#else
#define SSS_ROLLOUT_HEURISTICS true
#endif
SSS_KERNEL void SSS_KNAME(sss_rollout_kernel)(SssKernelArgs a, int policy, int param, int n_steps, int auto_reset, uint64_t seed_stride) {
  ROLLOUT_BODY(SSS_ROLLOUT_HEURISTICS)
}
#ifdef __HIP__
SSS_KERNEL void SSS_KNAME(sss_rollout_heur_kernel)(SssKernelArgs a, int policy, int param, int n_steps, int auto_reset, uint64_t seed_stride) {
  ROLLOUT_BODY(true)
}
#endif
#undef ROLLOUT_BODY
#undef SSS_ROLLOUT_HEURISTICS

#include "sss_sim_each.h"  // the fused rollout with a policy per env (sss_rollout_each): a kernel of its own, and the emulator's launchers of it
#include "sss_sim_until.h"  // ... and the one that stops at a time horizon and reports the remaining work (sss_rollout_until), likewise

#undef H
#undef FAIL
#undef CHECK

// (behind the #undefs: it brings in the GNN headers, whose names the short macros above must not touch)
#ifndef SSS_TIMELINE
#include "sss_sim_decima.h"  // ... and the one with Decima among the policies (sss_rollout_decima): the GNN inlined, kernels with a launch bound of their own
#include "sss_sim_action.h"  // ... and the ones whose first step is a given action (sss_rollout_action), with and without Decima
#endif
