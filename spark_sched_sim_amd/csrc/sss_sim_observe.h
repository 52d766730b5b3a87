// sss_sim_observe.h - part of the simulator device code (csrc/sss_sim.h includes the parts in order; not a stand-alone header):
// the wave-parallel schedulable-stage scan and the observation writer.
// Reference citations as in sss_sim.h (ENV / TRK / JOB / STG / TPCH / EVQ : line).
#undef SSS_SRC_ID
#define SSS_SRC_ID 10  // SssHdr::err_line = SSS_SRC_ID * 100000 + line of the check that failed
#include <stddef.h>
// _find_schedulable_stages() over all active jobs (ENV:505-540): one lane per stage of a job,
// ballot gives the job's ready mask; sat_mask makes the parent test a mask operation.
// Returns len(schedulable_stages); lane 0 stores the per-job masks.
// n_active / source job come from the mailbox lane 0 filled before the preceding wave_sync
// (publish_scan_inputs): lane 0 may already be past this function when another lane reads them.
SSS_DEV int find_schedulable_all() {
  PROF3(21);
  int lane = wave_lane();
  int A = g_sc.m_n_active;
  int src_job = g_sc.m_src_job;
  uint32_t total = 0;
  // one lane per active job; readiness of a stage is a mask test against the job's saturated mask
  for (int a0 = 0; a0 < A; a0 += 64) {
    int a = a0 + lane;
    uint32_t cnt = 0;
    if (a < A) {
      int j = lds_active()[a];
      SssJob* job = jobp(j);
      uint64_t m = 0;
      if (j == src_job || (int)job->supply < g_c.E) m = ready_mask_of_job(*job, false);
      job->sched_mask = m;
      cnt = (uint32_t)popc64(m);
    }
    total += wave_sum_u32(cnt);
  }
  return (int)total;
}

// ---- what pass 1 of write_observation leaves for the node and edge passes, per job of the current chunk of 64 active jobs ----
// The areas are scratch of the event handlers (SssScratch in sss_sim.h: pool tables staged by pool_pair_stage / pool_open, the
// commitment snapshot of a fulfilment, the members of a batch of released / arriving executors). Each of them is filled and
// consumed inside one event-loop round; the observation is written after the step's last round, so all of them are dead here,
// and nothing is expected in them when the next step starts. (The arrays have SSS_MAX_EXEC >= 64 entries, the tables >= 256 bytes.)
#define OBS_ACT_LO ((uint32_t*)g_sc.setA)     // active_mask, low and high word
#define OBS_ACT_HI ((uint32_t*)g_sc.setB)
#define OBS_EOFF (g_sc.fc_dst)                // edge_off: the job's first edge row in the pack
#define OBS_PREF (g_sc.rl_old)                // bits 0..15: stage slots (n_stages) of the chunk's jobs before this one, bits 16..31: their node rows
#define OBS_LOC (g_sc.rl_seq)                 // where the job's records are: its cache slot, or OBS_LOC_HBM | job
#define OBS_EPREF ((uint16_t*)g_sc.fc_num)    // template edges (n_edges) of the chunk's jobs before this one
#define OBS_LOC_HBM 0x80000000u
#define OBS_NO_ROW 0xFFFFFFFFu                // (node rows are below 2^17: SSS_MAX_JOBS * SSS_MAX_STAGES)
#define OBS_PREF_END 0xFFFFu                  // ... of the positions past the chunk's last job: above every index searched for
static_assert(offsetof(SssPoolHdr, commit_from) == offsetof(SssPoolHdr, used) + 2 && offsetof(SssPoolHdr, used) % 4 == 0, "used and commit_from are read as one word");
static_assert(SSS_SET_TABLE >= 256 && SSS_MAX_EXEC >= 64, "the observation writer's per-job scratch is 64 entries of 4 bytes per area");

// On the GPU the two copies of a record are read through pointers of their own address space, so that the two code paths stay
// two (the same statements on a cache slot and on the HBM copy otherwise fold into one flat access through a selected
// pointer), and SSS_USE_HERE pins what is computed from a loaded value to the place it is written at - after the other loads
// have been issued - instead of the place of the load, where it would wait for that load alone. Plain C++ elsewhere.
#if defined(__HIP_DEVICE_COMPILE__)
#define SSS_AS_LDS(T, p) ((const __attribute__((address_space(3))) T*)(p))
#define SSS_AS_HBM(T, p) ((const __attribute__((address_space(1))) T*)(p))
#define SSS_USE_HERE(x) asm volatile("" : "+v"(x))
#else
#define SSS_AS_LDS(T, p) ((const T*)(p))
#define SSS_AS_HBM(T, p) ((const T*)(p))
#define SSS_USE_HERE(x) ((void)(x))
#endif

// the job of the chunk that index i falls into: the last position whose prefix is <= i (prefixes ascend, position 0 holds 0,
// the positions past the last job hold OBS_PREF_END; jobs that contribute nothing share their prefix with the next one and are
// never found). Six LDS reads, no memory round trip.
SSS_DEV int obs_find_by_slot(int i) {
  int lo = 0;
  SSS_UNROLL8 for (int w = 32; w >= 1; w >>= 1)
    if ((int)(OBS_PREF[lo + w] & 0xFFFFu) <= i) lo += w;
  return lo;
}
SSS_DEV int obs_find_by_edge(int i) {
  int lo = 0;
  SSS_UNROLL8 for (int w = 32; w >= 1; w >>= 1)
    if ((int)OBS_EPREF[lo + w] <= i) lo += w;
  return lo;
}

// _observe (ENV:345-406) + utils.subgraph (utils.py:5-22) into the env's padded output rows.
// Every job's record is read once (pass 1); the node pass has a lane per stage the jobs really have and the edge pass a lane per
// edge they really have - not per (job, widest job of the pack) - and each of them issues all its loads before its first store:
// at C2 sizes (about 25 active jobs, 150 node rows, 150 edges) the whole function waits for memory four times - the job records,
// the node loads, the node stores (at the head of the edge loop), the edge loads - where it waited about twelve times.
SSS_DEV void write_observation(const SssLayout& L, const SssBuffers& B, int env, double reward) {
  PROF3(22);
  int lane = wave_lane();
  uint64_t t_obs0 = wave_clock();
  const SssHdr& h = g_hot.h;
  // the output rows alias nothing that is read here: the loads of later iterations may pass earlier stores
  float* __restrict__ nodes = B.nodes + (size_t)env * L.n_cap * 3;
  int32_t* __restrict__ el = B.edge_links + (size_t)env * L.ed_cap * 2;
  int32_t* __restrict__ dag_ptr = B.dag_ptr + (size_t)env * (L.J_cap + 1);
  int32_t* __restrict__ sup = B.exec_supplies + (size_t)env * L.J_cap;
  int A = h.n_active;
  uint32_t srck = h.curr_source;
  // num_committable_execs of the source pool: the load starts here and is only looked at in lane 0's tail
  // (SssPoolHdr::used | commit_from << 16; with active jobs the load goes out next to the first chunk's job records)
  uint32_t src_used_cf = 0;
  if (A == 0 && lane == 0 && srck != POOL_NONE) src_used_cf = *SSS_AS_HBM(uint32_t, &g_c.pool_hdr[pool_index(srck)].used);
  int src_job = (srck == POOL_NONE || srck == POOL_COMMON) ? -1 : key_job(srck);
  int src_idx = A;  // ENV:352
  uint64_t lt = bit64(lane) - 1;
  // The edge rows are a function of the active jobs, their order and their active-stage masks alone: when none of that has
  // changed since they were last written to this buffer, they are there already.
  const bool same_graph = h.obs_graph_version == h.graph_version && h.obs_bind_gen == B.gen;
  int base_e = same_graph ? h.obs_n_edges : 0;
  const int SPn = g_c.SP;
  uint32_t run = 0;  // node rows of the chunks before this one
  for (int a0 = 0; a0 < A; a0 += 64) {
    // pass 1 - lanes over the chunk's jobs, each record read once: dag_ptr (exclusive scan of active-stage counts),
    // exec_supplies, and the per-job scratch of the two passes below
    const int a = a0 + lane;
    uint32_t cnt = 0, nst = 0, ned = 0, loc = 0, eoff = 0;
    uint64_t act = 0;
    int j = -1, supply = 0;
    if (a < A) {
      j = lds_active()[a];
      const int s = lds_slot_of()[j];
      if (a == 0 && srck != POOL_NONE) src_used_cf = *SSS_AS_HBM(uint32_t, &g_c.pool_hdr[pool_index(srck)].used);
      // the LDS copy and the HBM copy on code paths of their own (ds_* / global_* instead of flat accesses)
      if (s != SLOT_NONE) {
        const auto* job = SSS_AS_LDS(SssJob, lds_cjobs()) + s;
        act = job->active_mask, supply = job->supply, nst = job->n_stages, ned = job->n_edges, eoff = (uint32_t)job->edge_off;
        loc = (uint32_t)s;
      } else {
        const auto* job = SSS_AS_HBM(SssJob, g_c.jobs) + j;
        act = job->active_mask, supply = job->supply, nst = job->n_stages, ned = job->n_edges, eoff = (uint32_t)job->edge_off;
        loc = OBS_LOC_HBM | (uint32_t)j;
      }
      cnt = (uint32_t)popc64(act);
    }
    // one scan for both counts: each sums to at most 64 * 64 over a chunk
    const uint32_t both = cnt << 16 | nst;
    const uint32_t excl = wave_scan_excl_u32(both);
    const uint32_t tot = wave_readlane_u32(excl + both, 63);
    uint32_t e_excl = 0, tot_e = 0;
    if (!same_graph) {  // (at most 64 * 255 edges in a chunk)
      e_excl = wave_scan_excl_u32(ned);
      tot_e = wave_readlane_u32(e_excl + ned, 63);
    }
    uint64_t is_src = wave_ballot(a < A && j == src_job);
    if (is_src) src_idx = a0 + ctz64(is_src);
    if (a < A) {
      OBS_ACT_LO[lane] = (uint32_t)act, OBS_ACT_HI[lane] = (uint32_t)(act >> 32);
      OBS_EOFF[lane] = eoff, OBS_LOC[lane] = loc;
      OBS_PREF[lane] = excl, OBS_EPREF[lane] = (uint16_t)e_excl;
    } else {
      OBS_PREF[lane] = OBS_PREF_END, OBS_EPREF[lane] = (uint16_t)OBS_PREF_END;
    }
    wave_sync();
    // pass 2 - lanes over the stage slots of the chunk's jobs: node rows. Four slots per lane at a time; a slot whose stage
    // is not active loads nothing. The loads from HBM of all four are issued first; the rows of jobs in the LDS cache are
    // written while those are in flight, then the rows that waited for them.
    const int tot_s = (int)(tot & 0xFFFFu);
    for (int i0 = 0; i0 < tot_s; i0 += 64 * 4) {
      uint32_t info[4], lc[4];  // info: OBS_NO_ROW, or the node row | stage << 20; lc: OBS_LOC of the job
      int32_t remaining[4];     // (the three only mean something where lc says HBM)
      float recent[4];
      uint32_t sched[4];
      SSS_UNROLL4 for (int u = 0; u < 4; u++) {
        const int i = i0 + 64 * u + lane;
        info[u] = OBS_NO_ROW, lc[u] = 0;
        if (i < tot_s) {
          const int al = obs_find_by_slot(i);
          const uint32_t pref = OBS_PREF[al];
          const int st = i - (int)(pref & 0xFFFFu);
          const uint64_t am = (uint64_t)OBS_ACT_HI[al] << 32 | OBS_ACT_LO[al];
          if (am & bit64(st)) {
            info[u] = (run + (pref >> 16) + (uint32_t)popc64(am & (bit64(st) - 1))) | (uint32_t)st << 20;
            lc[u] = OBS_LOC[al];
            if (lc[u] & OBS_LOC_HBM) {
              const int jj = (int)(lc[u] & ~OBS_LOC_HBM);
              remaining[u] = SSS_AS_HBM(SssStage, g_c.stages)[jj * SPn + st].remaining;
              recent[u] = SSS_AS_HBM(float, g_c.durations)[jj * SPn + st];
              sched[u] = SSS_AS_HBM(uint32_t, &g_c.jobs[jj].sched_mask)[st >> 5];
            }
          }
        }
      }
      // plain stores: non-temporal ones were measured to double the HBM write traffic (partial
      // lines are no longer combined in L2) for no gain in time
      SSS_UNROLL4 for (int u = 0; u < 4; u++) {
        if (info[u] != OBS_NO_ROW && !(lc[u] & OBS_LOC_HBM)) {
          const int row = (int)(info[u] & 0xFFFFFu), st = (int)(info[u] >> 20), s = (int)lc[u];
          nodes[row * 3 + 0] = (float)SSS_AS_LDS(SssStage, lds_cstages())[s * SPn + st].remaining;
          nodes[row * 3 + 1] = SSS_AS_LDS(float, lds_cdur())[s * SPn + st];
          nodes[row * 3 + 2] = (SSS_AS_LDS(uint32_t, &lds_cjobs()[s].sched_mask)[st >> 5] >> (st & 31) & 1u) ? 1.0f : 0.0f;
        }
      }
      // (one wait for all of them here, where every lane passes: inside the branches below each row would wait on its own,
      // and for the stores before it as well)
      SSS_UNROLL4 for (int u = 0; u < 4; u++) {
        SSS_USE_HERE(remaining[u]);
        SSS_USE_HERE(recent[u]);
        SSS_USE_HERE(sched[u]);
      }
      SSS_UNROLL4 for (int u = 0; u < 4; u++) {
        if (info[u] != OBS_NO_ROW && (lc[u] & OBS_LOC_HBM)) {
          const int row = (int)(info[u] & 0xFFFFFu), st = (int)(info[u] >> 20);
          nodes[row * 3 + 0] = (float)remaining[u];
          nodes[row * 3 + 1] = recent[u];
          nodes[row * 3 + 2] = (sched[u] >> (st & 31) & 1u) ? 1.0f : 0.0f;
        }
      }
    }
    // pass 3 - lanes over the template edges of the chunk's jobs: the active subgraph, compacted in (job, edge) order.
    // Four groups of 64 edges at a time: the pack's edges of all four are fetched together; the job's mask and first row
    // come from pass 1.
    for (int i0 = 0; i0 < (int)tot_e; i0 += 64 * 4) {
      int al[4], uu[4], vv[4];
      SSS_UNROLL4 for (int u = 0; u < 4; u++) {
        const int i = i0 + 64 * u + lane;
        al[u] = -1, uu[u] = 0, vv[u] = 0;
        if (i < (int)tot_e) {
          al[u] = obs_find_by_edge(i);
          const int eo = (int)OBS_EOFF[al[u]] + (i - (int)OBS_EPREF[al[u]]);
          uu[u] = g_c.pk.edges[2 * eo], vv[u] = g_c.pk.edges[2 * eo + 1];
        }
      }
      SSS_UNROLL4 for (int u = 0; u < 4; u++) {
        if (i0 + 64 * u >= (int)tot_e) break;
        uint64_t am = 0;
        int nb = 0;
        if (al[u] >= 0) am = (uint64_t)OBS_ACT_HI[al[u]] << 32 | OBS_ACT_LO[al[u]], nb = (int)(run + (OBS_PREF[al[u]] >> 16));
        const bool keep = (am & bit64(uu[u])) && (am & bit64(vv[u]));
        const uint64_t bal = wave_ballot(keep);
        if (keep) {
          const int pos = base_e + popc64(bal & lt);
          el[2 * pos + 0] = nb + popc64(am & (bit64(uu[u]) - 1));
          el[2 * pos + 1] = nb + popc64(am & (bit64(vv[u]) - 1));
        }
        base_e += popc64(bal);
      }
    }
    // (after the two passes: stores in flight ahead of them would be waited for along with their loads)
    if (a < A) {
      dag_ptr[a] = (int32_t)(run + (excl >> 16));
      sup[a] = supply;
    }
    run += tot >> 16;
    if (a0 + 64 < A) wave_sync();  // the next chunk's pass 1 overwrites the scratch
  }
  int base_n = (int)run;
  if (lane == 0) {
    dag_ptr[A] = base_n;
    int32_t* oi = B.obs_i32 + (size_t)env * SSS_OBS_I32;
    double* of = B.obs_f64 + (size_t)env * SSS_OBS_F64;
    SSS_USE_HERE(src_used_cf);
    const int ncommit = (int)(uint16_t)src_used_cf - (int)(int16_t)(src_used_cf >> 16);
    oi[OBS_N_NODES] = base_n, oi[OBS_N_EDGES] = base_e, oi[OBS_N_JOBS] = A, oi[OBS_N_SCHED] = h.n_sched;
    oi[OBS_NUM_COMMITTABLE] = ncommit, oi[OBS_SOURCE_JOB_IDX] = src_idx;
    oi[OBS_TERMINATED] = h.terminated, oi[OBS_ERR] = h.err;
    of[OBS_REWARD] = reward, of[OBS_WALL_TIME] = h.wall_time;
    g_hot.h.prof[4] += wave_clock() - t_obs0;
    g_hot.h.obs_n_nodes = base_n;
    g_hot.h.obs_graph_version = h.graph_version, g_hot.h.obs_n_edges = base_e, g_hot.h.obs_bind_gen = B.gen;
    g_hot.h.obs_n_sched = h.n_sched;
    g_hot.h.last_reward = reward;
    // SURVEY 8(d) algorithmic bytes of this step: k*140 + 12N + (12N + 4(A+1) + 4A + 8Ed + 12) + 26
    g_hot.h.model_bytes += (uint64_t)g_sc.events_this_step * 140u + 24u * (uint64_t)base_n + 4u * (uint64_t)(A + 1) +
                            4u * (uint64_t)A + 8u * (uint64_t)base_e + 12u + 26u;
  }
}
