/* include/sss.h - C ABI of the MI355X-native batched Spark-scheduling simulator.
 *
 * This is the drop-in boundary for the reference's hot path: everything below
 * `SparkSchedSimEnv.reset()/step()` (reference spark_sched_sim/spark_sched_sim.py:127-221),
 * batched over `num_envs` independent environments, one wavefront per environment.
 * The reference is pure Python with no FFI of its own; these entry points are what a binding
 * for this path binds (INTEGRATION.md shows the ctypes stub the reference would add, and
 * spark_sched_sim_amd/binding.py is that stub in this repo).
 *
 * Conventions: plain C types only; every pointer named *_dev is a device pointer owned by the
 * caller (torch tensors in the Python host); calls are asynchronous on the HIP stream passed
 * as `void* stream` (NULL = default stream); return 0 on success, otherwise a negative code
 * and sss_last_error() describes it. A handle is not re-entrant.
 */
#ifndef SSS_H
#define SSS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sss_handle sss_handle;

/* env_cfg of the reference (spark_sched_sim.py:34-52, data_samplers/tpch.py:19-26) */
typedef struct sss_cfg {
  int32_t num_executors;   /* env_cfg["num_executors"], 1..128 (65..128: the wide instantiation of the kernels) */
  int32_t job_arrival_cap; /* env_cfg.get("job_arrival_cap"); <= 0 means None */
  int32_t max_jobs;        /* arena capacity in jobs; 0 = job_arrival_cap (required when cap is None) */
  int32_t reserved;
  double job_arrival_rate; /* tpch.py:21,42 (jobs per ms) */
  double moving_delay;     /* spark_sched_sim.py:40 */
  double warmup_delay;     /* tpch.py:24,43 */
  double beta;             /* spark_sched_sim.py:44 */
} sss_cfg;

/* sizes the caller needs to allocate the buffers below (all per env unless noted) */
typedef struct sss_dims {
  int32_t num_envs, num_executors, job_cap, stage_stride;
  int32_t node_cap;    /* rows of nodes[env]            */
  int32_t edge_cap;    /* rows of edge_links[env]       */
  int32_t obs_i32;     /* ints per env in obs_i32       */
  int32_t obs_f64;     /* doubles per env in obs_f64    */
  int64_t state_bytes; /* whole arena, all envs; must be zero-initialised */
  int64_t env_stride;  /* bytes per env inside the arena */
  /* byte offsets inside one env's arena block of arrays the host may view zero-copy
   * (replaces the attribute reads of reference metrics.py:4-23, rollout_worker.py:122-129) */
  int64_t off_t_arrival, off_t_completed, off_jobs, off_active, off_dur_ring;
  int32_t job_rec_bytes, hdr_bytes;
} sss_dims;

/* raw device pointers of caller-allocated buffers (observation = reference spark_sched_sim.py:345-406) */
typedef struct sss_buffers {
  void* state_dev;            /* uint8 [state_bytes]                                   */
  float* nodes_dev;           /* f32  [num_envs][node_cap][3]  dag_batch.nodes          */
  int32_t* edge_links_dev;    /* i32  [num_envs][edge_cap][2]  dag_batch.edge_links     */
  int32_t* dag_ptr_dev;       /* i32  [num_envs][job_cap + 1]  dag_ptr                  */
  int32_t* exec_supplies_dev; /* i32  [num_envs][job_cap]      exec_supplies            */
  int32_t* obs_i32_dev;       /* i32  [num_envs][8]: n_nodes, n_edges, n_active_jobs, n_schedulable,
                                 num_committable_execs, source_job_idx, terminated, err */
  double* obs_f64_dev;        /* f64  [num_envs][2]: reward, wall_time                  */
} sss_buffers;

/* per-env error codes reported in obs_i32[..][7] (reference exceptions they stand for) */
enum {
  SSS_E_OK = 0,
  SSS_E_ACTION_SPACE = 1, /* ValueError spark_sched_sim.py:276-277 */
  SSS_E_STAGE_IDX = 2,    /* KeyError   spark_sched_sim.py:284     */
  SSS_E_TOO_MANY = 4,     /* ValueError spark_sched_sim.py:294-295 */
  SSS_E_STALLED = 5,      /* AssertionError "[step]" spark_sched_sim.py:212-215 */
  SSS_E_NO_DURATION = 6,  /* KeyError/ValueError out of tpch.py:88-106 */
  SSS_E_INVARIANT = 7,    /* any other reference assert */
  SSS_E_NEED_RESET = 8,   /* step() on a finished / failed episode */
  SSS_E_NO_LIMIT = 9,     /* ValueError spark_sched_sim.py:137-138 */
  SSS_E_CAPACITY = 10     /* more jobs than max_jobs (time-limit mode) */
};

/* Host-only: validates cfg + workload pack (spark_sched_sim_amd/workload.py format) and reports
 * buffer sizes. Replaces nothing in the reference (Python allocates as it goes). */
int sss_query_dims(const sss_cfg* cfg, const void* pack, size_t pack_bytes, int num_envs, sss_dims* out);

/* Replaces SparkSchedSimEnv.__init__ (spark_sched_sim.py:34-125) + TPCHDataSampler.__init__
 * (tpch.py:19-52): copies the pack and the derived constants to device `device`. */
int sss_create(const sss_cfg* cfg, const void* pack, size_t pack_bytes, int num_envs, int device, sss_handle** out);

int sss_bind_buffers(sss_handle* h, const sss_buffers* buffers);

/* Replaces SparkSchedSimEnv.reset(seed, options) (spark_sched_sim.py:127-186) for every env whose
 * mask byte is non-zero (mask_dev NULL = all). seeds_dev: u64[num_envs]; time_limits_dev:
 * f64[num_envs] or NULL (= inf, options["time_limit"]). Writes the first observation. */
int sss_reset(sss_handle* h, const uint64_t* seeds_dev, const double* time_limits_dev, const uint8_t* mask_dev, void* stream);

/* Replaces SparkSchedSimEnv.step(action) (spark_sched_sim.py:188-221) for all envs:
 * action = {"stage_idx": stage_idx_dev[i], "num_exec": num_exec_dev[i]}. Writes reward, wall_time,
 * terminated, err and the next observation. auto_reset != 0: an env found terminated at entry
 * starts its next episode instead (seed = previous seed + seed_stride), reward 0.
 * stage_idx_dev[i] == SSS_SKIP_ENV leaves env i completely untouched (state, outputs, counters):
 * how a rollout collector freezes envs whose episode was truncated by a wrapper
 * (wrappers/stochastic_time_limit.py:26-31) while the rest of the batch keeps stepping. */
#define SSS_SKIP_ENV (-2147483647 - 1)
int sss_step(sss_handle* h, const int32_t* stage_idx_dev, const int32_t* num_exec_dev, int auto_reset, uint64_t seed_stride, void* stream);

/* sss_step with an event budget per launch - the reference's envs run in worker processes of their own, one step() never waits
 * for another env's (trainers/rollout_worker.py:133-206); a launch of sss_step ends with its slowest env. Here an env whose step
 * has taken max_events events (>= 1; batches of events are not cut, so it may overshoot by one batch) stops between two events:
 * ready_dev[i] = 0, its outputs (observation, reward, terminated, err) are NOT written, and the next sss_step_bounded / sss_step
 * call continues that step - its action arguments for env i are then not looked at. ready_dev[i] = 1: the step is complete, the
 * outputs are the ones sss_step writes. SSS_SKIP_ENV envs: ready_dev[i] is left alone. Every env goes through the states and
 * outputs it goes through under sss_step, bit for bit; only the launch in which its k-th step completes differs. */
int sss_step_bounded(sss_handle* h, const int32_t* stage_idx_dev, const int32_t* num_exec_dev, int auto_reset, uint64_t seed_stride, int max_events,
                     uint8_t* ready_dev, void* stream);

/* On-device counterparts of the reference's heuristic Scheduler plugins; they fill one action per
 * env for the next sss_step. policy: 0 = fair (RoundRobinScheduler(dynamic_partition=True),
 * schedulers/heuristics/round_robin.py:7-49), 1 = FIFO (dynamic_partition=False), 2 = the build's
 * counter-based uniform-random policy (param = per-mille probability of stage_idx = -1), 3 = weighted
 * fair (the Decima paper's baseline: per-job executor caps in proportion to job work^alpha; param = alpha,
 * an integer in [-4, 4], anything else fails with -23), 4 = SJF-CP (shortest job first, inside it the
 * schedulable stage at the head of the critical path; param unused). 3 and 4 are defined on the observation
 * and match the host plugins WeightedFairScheduler / SJFCPScheduler (schedulers.py) bit for bit. */
int sss_policy(sss_handle* h, int policy, int param, int32_t* stage_idx_dev, int32_t* num_exec_dev, void* stream);

/* n_steps x (policy -> step -> observe) per env in ONE launch: the episode loop of reference
 * examples.py:84-102 / trainers/rollout_worker.py:135-157 with an on-device policy. Per-step
 * semantics are exactly those of sss_policy + sss_step; only the last observation survives. */
int sss_rollout(sss_handle* h, int policy, int param, int n_steps, int auto_reset, uint64_t seed_stride, void* stream);

/* Decima's view of the current observations, for all envs in one launch: replaces
 * DecimaObsWrapper.observation (schedulers/decima/env_wrapper.py:69-143), the DAG-layer edge masks
 * (schedulers/decima/utils.py:238-267) and the PyG batch collation (utils.py:117-204). Reads the
 * bound observation buffers only. The envs' nodes / jobs / edges are written back to back into flat
 * arrays at the offsets the caller supplies (exclusive prefix sums of n_nodes / n_jobs / n_edges over
 * the envs with active != 0); M, J, Ed below are the totals.
 *   x f32[M,5]             node features [commit cap / E, +-1 source-job flag, supply / E,
 *                          remaining / num_tasks_scale, remaining * duration / work_scale]
 *   node_obs/loc/job i64[M] env, row inside the env's observation, flat job id
 *   sched_rank i64[M]      index among the env's schedulable stages (what stage_idx means), or -1
 *   gen i32[M]             topological generation inside the active subgraph
 *   node_recv u32[M]       bit l: the node is the source end of an edge of DAG layer l
 *   stage_mask u8[M]
 *   src/dst/edge_obs i64[Ed]  flat node ids of the edge's ends, env
 *   edge_layers u32[Ed]    bit l: the edge is in the reference's edge_masks[l]
 *   job_obs/cap/first i64[J]  env, number of allowed executor counts, flat id of the job's first node
 *   obs_depth i32[num_envs]   number of DAG layers (rows of the reference's edge_masks) per env */
typedef struct sss_decima_graph {
  const uint8_t* active_dev; /* u8[num_envs] or NULL (= all) */
  const int64_t* node_off_dev;
  const int64_t* job_off_dev;
  const int64_t* edge_off_dev;
  float num_tasks_scale; /* 200 in the reference (env_wrapper.py:48) */
  float work_scale;      /* 1e5 (env_wrapper.py:49) */
  float* x_dev;
  int64_t* node_obs_dev;
  int64_t* node_loc_dev;
  int64_t* node_job_dev;
  int64_t* sched_rank_dev;
  int32_t* gen_dev;
  uint32_t* node_recv_dev;
  uint8_t* stage_mask_dev;
  int64_t* src_dev;
  int64_t* dst_dev;
  int64_t* edge_obs_dev;
  uint32_t* edge_layers_dev;
  int64_t* job_obs_dev;
  int64_t* job_cap_dev;
  int64_t* job_first_dev;
  int32_t* obs_depth_dev;
  int64_t* job_nodes_dev; /* i64[J] number of nodes of the job (they follow job_first back to back) */
  int64_t* out_start_dev; /* i64[M] flat id of the node's first out-edge; a node's out-edges are contiguous */
  int32_t* out_deg_dev;   /* i32[M] number of out-edges */
  int32_t* layer_cnt_dev; /* i32[32][num_envs]: [l][b] = nodes of env b that are sources of layer-l edges */
  /* optional (both or neither): sched_off_dev i64[num_envs] = exclusive prefix sums of the envs' schedulable-stage counts
   * (obs_i32[OBS_N_SCHED], 0 for inactive envs); sched_list_dev then receives the flat ids of the schedulable nodes, env by
   * env in node order - the row list of the stage-score launch (sss_gnn_launch STAGE), with no padding */
  const int64_t* sched_off_dev;
  int64_t* sched_list_dev;
  /* optional (all or none): the layers' lists of receiving nodes written by this launch itself. An env reserves its share of
   * a list with a fetch-add on a counter it shares with its BLOCK of envs only - SSS_LIST_SETS = 32 blocks of
   * q = ceil(num_envs / 32) consecutive envs (4096 envs adding to the same addresses: 35 us of a 78 us launch,
   * profiles/r05_graph_kernel.txt) - so layer l's list is up to 32 dense pieces: block s's piece starts at
   * recv_lists_dev[l * recv_stride + node_off_dev[s * q]] and has layer_totals_dev[l * 32 + s] entries (i64[33][32], ZERO on
   * entry; recv_stride >= the total node count; a block's receivers are among its own nodes, so pieces never overlap; row 32
   * receives the largest node count of an env of block s - sss_gnn_encode_args.max_obs_nodes_hint is made of it). The
   * order of the envs inside a piece is not fixed (the layer launches treat rows independently). sss_gnn_encode takes the
   * pieces as they are (recv_stride there): no scan, no list kernel */
  int64_t* layer_totals_dev;
  int64_t* recv_lists_dev;
  int64_t recv_stride;
  /* optional: ANOTHER set of list counters (i64[33][32]) that this launch sets to zero - a caller that builds a graph per step
   * keeps two sets and passes them in turn (this step's zeroed by the previous launch, the previous step's - its consumers are
   * behind this launch in the stream - cleared now), which saves the clearing launch in between */
  int64_t* layer_totals_clear_dev;
  /* number of i64 entries behind layer_totals_dev (and behind layer_totals_clear_dev): must be 33 * 32 = 1056 whenever either is
   * passed. The counters grew from i64[32] to i64[33][32] in round 5; a caller built against the older layout now gets -1 and a
   * message instead of fetch-adds past the end of its 32-entry buffer. */
  int64_t layer_totals_len;
} sss_decima_graph;
int sss_decima_graph_build(sss_handle* h, const sss_decima_graph* g, void* stream);

/* sizeof() of an argument structure of this header as the LIBRARY was compiled with ("sss_cfg", "sss_decima_graph", ...; -1: unknown
 * name): a binding checks its mirrors against it once (spark_sched_sim_amd/binding.py: check_abi; tests/test_abi.py), so that a
 * stale binding fails loudly instead of handing the library a structure of another layout. No reference counterpart (the reference
 * has no native boundary). */
int sss_abi_sizeof(const char* struct_name);

/* The nodes each DAG layer updates, as index lists (what nonzero((node_recv >> l) & 1) returns), for
 * all layers in one launch: layer l's list starts at recv_dev[layer_base[l]]; env_off_dev = exclusive
 * prefix sums of layer_cnt along the env axis. */
typedef struct sss_decima_lists {
  const int64_t* node_off_dev;
  const int64_t* obs_nodes_dev;
  const uint32_t* node_recv_dev;
  const int64_t* env_off_dev; /* i64[32][num_envs] */
  int64_t layer_base[32];
  int64_t* recv_dev;
  int n_layers;
} sss_decima_lists;
int sss_decima_layer_lists(int num_envs, const sss_decima_lists* a, void* stream);

/* The DAG layers' index lists of a batch graph from its per-edge / per-node layer masks (sss_decima_graph_build's edge_layers /
 * node_recv; the reference's `edge_masks[l]` as index lists, decima/utils.py:249-267): for every bit l < n_layers the ascending
 * positions e with bit l of bits_dev[e] set - what torch.nonzero over (bits >> l) & 1 returns, for all layers in two launches.
 *   pass 0: cnt_dev[c * n_layers + l] (i32[n_chunks][n_layers]) = such positions in chunk c = [c * chunk, (c + 1) * chunk);
 *           chunk a multiple of 64, n_chunks = ceil(n / chunk). The caller scans the counts along the chunks (sss_prefix_rows with
 *           src_row_stride 1, src_col_stride n_layers) into off_dev i64[n_layers][n_chunks] and reads the totals;
 *   pass 1: out_dev[base[l] + off_dev[l][c] + rank] = e  (base[l]: where layer l's list starts in out_dev; host values). */
typedef struct sss_bit_list_args {
  const int32_t* bits_dev;
  int64_t n;
  int32_t n_layers, chunk;
  int32_t n_chunks, phase; /* phase: 0 = count, 1 = write ("pass" above) */
  int32_t* cnt_dev;
  const int64_t* off_dev;
  int64_t base[32];
  int64_t* out_dev;
} sss_bit_list_args;
int sss_bit_lists(const sss_bit_list_args* a, void* stream);

/* Exclusive prefix sums and totals of n_rows rows of n_cols non-negative counts, one launch (the offsets the two
 * kernels above are fed: per-env node / edge / job offsets of the compact graph, per-env offsets into each DAG
 * layer's receiver list; what utils.collate_obsns does with torch.cumsum on the host, decima/utils.py:117-204).
 * src_dev[row * src_row_stride + col * src_col_stride] (i32; strides in elements, so that columns of the env's
 * obs_i32 rows can be scanned in place), mask_dev (u8[n_cols], nullable): masked-out columns count as 0.
 * off_dev: i64[n_rows][n_cols] exclusive prefix along the columns, cnt_dev (nullable): i64[n_rows][n_cols] the
 * (masked) counts themselves, totals_dev: i64[n_rows]. */
int sss_prefix_rows(const int32_t* src_dev, int64_t src_row_stride, int64_t src_col_stride, const uint8_t* mask_dev, int n_rows, int n_cols,
                    int64_t* off_dev, int64_t* cnt_dev, int64_t* totals_dev, void* stream);

/* Decima's GNN forward pass for inference (schedulers/decima/scheduler.py:142-385) on a compact graph
 * written by sss_decima_graph_build: one launch per stage of the pass, each evaluating one whole MLP
 * per row with its gather / scatter fused in. Supports the published architecture
 * (config/decima_tpch.yaml:66-78: embed_dim 16, GNN MLPs [32,16] + LeakyReLU, policy MLPs [64,64] +
 * Tanh). `w_dev` = that stage's MLP parameters packed [W1, b1, W2^T, b2, W3, b3] (W1, W3 in torch.nn.Linear's
 * [out,in] layout, the middle layer transposed to [in,out]).
 * kind: 0 PREP (rows = nodes: out = h_init[M,16] from x), 1 SINK (h = h_init where the node's
 * observation has depth 0 [obs_depth given], else 0 for nodes with out-edges, else update(h_init)),
 * 2 LAYER (rows = idx0, -1 = skip: tmp[n] = h_init[n] + update(sum over n's out-edges in DAG layer
 * `layer` of msg(h[dst])); w = msg, w2 = update), 3 COMMIT (h[n] = tmp[n] for the same rows),
 * 4 DAGSUM (rows = jobs: h_dag[j] = sum over its nodes of dag([x,h]), from the hidden vectors
 * 8 DAGHID left in tmp[M,16]), 5 GLOBSUM (rows = observations: h_glob[o] = sum over its jobs of
 * glob(h_dag), from the hidden vectors 9 GLOBHID left in tmp[J,16]), 6 STAGE (rows = idx0, -1 = skip:
 * out[node_obs*n_pad + node_loc] = score), 7 EXEC (rows = (b, c), c < E: out[b*E + c] = score of c+1
 * executors for job idx0[b], -inf where c >= job_cap). No atomics, fixed summation order. */
typedef struct sss_gnn_args {
  int64_t n_rows;
  const float* w_dev;
  const float* w2_dev;
  float slope;
  int num_executors;
  int layer;
  int64_t n_pad;
  const float* x_dev;
  const float* h_init_dev;
  float* h_dev;
  float* tmp_dev;
  float* h_dag_dev;
  float* h_glob_dev;
  float* out_dev;
  const int32_t* out_deg_dev;
  const int32_t* obs_depth_dev; /* SINK, nullable: batch semantics (no per-observation skip) when NULL */
  const int64_t* idx0_dev;
  const int64_t* dst_dev;
  const int64_t* out_start_dev;
  const uint32_t* edge_layers_dev;
  const int64_t* node_job_dev;
  const int64_t* node_obs_dev;
  const int64_t* node_loc_dev;
  const int64_t* job_obs_dev;
  const int64_t* job_first_dev;
  const int64_t* job_cap_dev;
  const int64_t* job_nodes_dev;
  const int64_t* obs_job_off_dev;
  const int64_t* obs_jobs_dev;
  /* LAYER, optional: the message / update MLPs once more, laid out for the 16-lanes-per-row kernel (csrc/sss_gnn16.h:
   * w1[i][g][q] = W1[g+16q][i], b1[g][q], w2[jj][q][g][r] = W2T[jj+16q][g+16r], b2[g][r], w3[k][g] = W3[g][k], b3[g]).
   * NULL: the kernel transposes w_dev / w2_dev while staging them (slower: strided reads in every workgroup). */
  const float* w16_dev;
  const float* w2_16_dev;
  /* LAYER, optional / MERGE (kind 10): i32 per node, bit l set = the node receives in DAG layer l (sss_decima_graph_build's
   * node_recv). With it a LAYER launch needs no COMMIT: each node's embedding alternates between h_dev and tmp_dev
   * (after v updates it is in buffer v & 1; layers run from the highest index down), a layer reads every child's
   * current buffer and writes the receiver's other one. MERGE (rows = nodes), once after the last layer: h = tmp
   * where the number of updates is odd; DAGHID (kind 8) does that on the fly when it is given node_recv_dev. */
  const int32_t* node_recv_dev;
  /* optional: the row count on the device (i64[1]) - for a Decima step without a device->host round trip (the graph's totals
   * stay where sss_prefix_rows left them). n_rows then only sizes the launch grid (any positive guess, e.g. last step's total);
   * every kernel strides over all *n_rows_dev rows. Not for LAYER (its list lengths come from layer_totals in sss_gnn_encode). */
  const int64_t* n_rows_dev;
} sss_gnn_args;
int sss_gnn_launch(int kind, const sss_gnn_args* args, void* stream);

/* Decima's whole decision for every env in ONE launch (one wavefront per env): observation transform,
 * GNN encoder, stage and executor-count scores and the two softmax draws of
 * DecimaScheduler.schedule (schedulers/decima/scheduler.py:71-99) - sss_decima_graph_build +
 * the sss_gnn_launch sequence + sampling, without the intermediate graph or any host round trip.
 * w_*_dev: the seven MLPs packed as for sss_gnn_launch. node_scratch_dev: f32[num_envs][node_cap][53],
 * job_scratch_dev: f32[num_envs][job_cap][32] (work space). Draws are Gumbel-max over a counter-based
 * uniform stream keyed by (rng_seed, rng_counter, env, candidate): pass a new rng_counter per call.
 * The stream's 24-bit uniforms lie strictly inside (0, 1), so its Gumbel values span [-2.85, 16.64]: a candidate scored more
 * than ~19.5 below the best is never drawn (its softmax probability is below ~3e-9) - the one way the draws differ from an
 * exact softmax sampler.
 * Outputs per env: stage_idx / num_exec (for sss_step; stage_idx -1 when nothing is schedulable),
 * Decima's action tuple (stage_sel, job_idx, exec_sel) and its log-probability; optional dense
 * scores (stage_scores_dev f32[num_envs][node_cap], exec_scores_dev f32[num_envs][E]; -inf = masked).
 * Any executor count the simulator takes (1..128: an executor count sits on lane c & 63, two per lane beyond 64). */
typedef struct sss_decima_policy_args {
  const uint8_t* active_dev; /* u8[num_envs] or NULL */
  float num_tasks_scale, work_scale, slope;
  const float* w_prep_dev;
  const float* w_msg_dev;
  const float* w_upd_dev;
  const float* w_dag_dev;
  const float* w_glob_dev;
  const float* w_stage_dev;
  const float* w_exec_dev;
  float* node_scratch_dev;
  float* job_scratch_dev;
  uint64_t rng_seed, rng_counter;
  int32_t* stage_idx_dev;
  int32_t* num_exec_dev;
  int32_t* stage_sel_dev;
  int32_t* job_idx_dev;
  int32_t* exec_sel_dev;
  float* lgprob_dev;
  float* stage_scores_dev; /* nullable */
  float* exec_scores_dev;  /* nullable */
  uint64_t* prof_dev;      /* nullable: u64[num_envs][8] shader cycles per phase + depth + node count */
} sss_decima_policy_args;
int sss_decima_policy(sss_handle* h, const sss_decima_policy_args* a, void* stream);
/* The same kernel with both decisions taken as the arg-max of its own scores instead of drawn (a second instantiation of the
 * device function; rng_seed / rng_counter are ignored): the stage with the largest score among the schedulable ones, then the
 * executor count with the largest score among the allowed ones - ties go to the lowest index, a NaN never wins. lgprob is the
 * log-softmax of the chosen entries, computed as the draw computes it. */
int sss_decima_policy_argmax(sss_handle* h, const sss_decima_policy_args* a, void* stream);

/* The two softmax draws of DecimaScheduler.schedule (schedulers/decima/scheduler.py:80-99) for the
 * sss_gnn_launch pipeline, one wavefront per observation, same Gumbel-max stream as sss_decima_policy.
 * which = 0: stage draw from stage_scores_dev (f32[n_obs][n_pad], -inf = masked) -> job_gid_dev (the
 * idx0 of the EXEC launch), stage_idx / stage_sel / job_idx, lgprob, any_stage. which = 1: executor
 * count draw from exec_scores_dev (f32[n_obs][E], any E >= 1: lanes stride over the counts) -> num_exec / exec_sel, lgprob += .
 * As in sss_decima_policy, a candidate scored more than ~19.5 below the best (probability below ~3e-9) is never drawn. */
typedef struct sss_decima_sample_args {
  int64_t n_pad;
  int num_executors;
  uint64_t rng_seed, rng_counter;
  const float* stage_scores_dev;
  const float* exec_scores_dev;
  const int64_t* obs_nodes_dev;
  const int64_t* obs_node_off_dev;
  const int64_t* obs_job_off_dev;
  const int64_t* sched_rank_dev;
  const int64_t* node_job_dev;
  int64_t* job_gid_dev;
  int32_t* stage_idx_dev;
  int32_t* num_exec_dev;
  int64_t* stage_sel_dev;
  int64_t* job_idx_dev;
  int64_t* exec_sel_dev;
  float* lgprob_dev;
  uint8_t* any_stage_dev;
} sss_decima_sample_args;
int sss_decima_sample(int n_obs, int which, const sss_decima_sample_args* a, void* stream);
/* The arg-max counterpart of the two draws (second instantiations of the same device functions; rng_seed / rng_counter are
 * ignored), same inputs, same outputs.
 * which = 0: the candidates are the slots i < obs_nodes[env] with sched_rank[i] >= 0 and a score other than -inf - the draw's own
 * filter: a stale finite score in a slot that is no schedulable stage loses. The largest score wins; TIES GO TO THE LOWEST i
 * (-0.0 and +0.0 tie); a NaN never wins. Writes any_stage, job_gid, stage_idx, stage_sel, job_idx as the draw does and
 * lgprob = s_sel - M - logf(S) from the draw's online log-sum-exp: for the same selection, the draw's bits. Nothing schedulable:
 * stage_idx = -1, zeros elsewhere, lgprob = 0.
 * which = 1: the candidates are the counts c < E with a score other than -inf (lanes stride over c, any E); the largest score wins,
 * ties go to the lowest c; lgprob += its log-softmax. No candidate, or any_stage == 0: exec_sel = 0, num_exec = 1, lgprob unchanged. */
int sss_decima_argmax(int n_obs, int which, const sss_decima_sample_args* a, void* stream);

/* Decima's encoder for one batch of observations in ONE call (scheduler.py:142-283: node embeddings by message passing over
 * the DAG layers, per-job and per-observation summaries): the launches sss_gnn_launch offers one by one - PREP, SINK, one LAYER
 * per DAG layer from max_depth - 1 down to 0, DAGHID (+ MERGE), DAGSUM, GLOBHID, GLOBSUM - preceded by the scan and the kernel
 * that build the layers' lists of receiving nodes. The lists' lengths never leave the device: a LAYER launch is sized by n_nodes
 * and reads its row count and list position from layer_totals_dev, so the call enqueues everything and returns (no device->host
 * round trip; with sss_gnn_launch the caller has to read the list sizes back between SINK and the first LAYER).
 * max_depth: an upper bound of the observations' DAG depth (e.g. the deepest template of the workload); layers beyond an
 * observation's own depth are empty. Graph arrays as written by sss_decima_graph_build (dst_dev / edge_layers_dev may be NULL
 * when the batch has no edge); layer_cnt_dev = its i32[32][n_obs] output. Parameters packed as for sss_gnn_launch (w_msg16_dev / w_update16_dev: the optional 16-lane images). Outputs:
 * h_dev f32[n_nodes,16] node embeddings, h_dag_dev f32[n_jobs,16], h_glob_dev f32[n_obs,16]; h_init_dev f32[n_nodes,16] and
 * tmp_dev f32[max(n_nodes, n_jobs),16] are work space, as are env_off_dev i64[32 * n_obs], layer_totals_dev i64[32] and
 * recv_dev i64[recv_cap] with recv_cap >= n_nodes * max_depth. Launches on the CURRENT device's stream (no handle). */
typedef struct sss_gnn_encode_args {
  int64_t n_nodes, n_jobs;
  int32_t n_obs, max_depth;
  float slope;
  int32_t layers_mode; /* the DAG layers: 1 = a launch per layer over the layer's receiving nodes of all observations; 2 = ONE launch,
                          a wave per observation walking its own layers (message passing never leaves an observation; the same
                          arithmetic per node - bit-identical embeddings; needs none of the lists); 0 = the library chooses: 2 for
                          batches of small observations (64 observations or more, max_obs_nodes_hint small: see there), where nine
                          launches at the launch floor cost more than a wave walking a handful of tiles alone, else 1 */
  const float* w_prep_dev;
  const float* w_update_dev;
  const float* w_msg_dev;
  const float* w_dag_dev;
  const float* w_glob_dev;
  const float* w_msg16_dev;     /* nullable */
  const float* w_update16_dev;  /* nullable */
  const float* x_dev;
  const int32_t* out_deg_dev;
  const int32_t* obs_depth_dev;
  const int64_t* node_obs_dev;
  const int64_t* dst_dev;
  const int64_t* out_start_dev;
  const uint32_t* edge_layers_dev;
  const int32_t* node_recv_dev;
  const int64_t* job_first_dev;
  const int64_t* job_nodes_dev;
  const int64_t* obs_job_off_dev;
  const int64_t* obs_jobs_dev;
  const int64_t* obs_node_off_dev;
  const int64_t* obs_nodes_dev;
  const int32_t* layer_cnt_dev;
  float* h_init_dev;
  float* h_dev;
  float* tmp_dev;
  float* h_dag_dev;
  float* h_glob_dev;
  int64_t* env_off_dev;
  int64_t* layer_totals_dev;
  int64_t* recv_dev;
  int64_t recv_cap;
  int64_t recv_stride;         /* 0: this call builds the lists (scan + list kernel into env_off_dev / layer_totals_dev / recv_dev);
                                  > 0: sss_decima_graph_build wrote them - layer l's pieces at recv_dev[l * recv_stride ..], their
                                  lengths in layer_totals_dev (then i64[33][32], see sss_decima_graph; env_off_dev unused, may be
                                  NULL) */
  int64_t layer_rows_hint[32]; /* host values: roughly how many nodes layer l updates (e.g. layer_totals of the previous step,
                                  read back lazily); only sizes the launch grids - every row is processed whatever it says.
                                  -1: no idea (the grid is sized by n_nodes) */
  /* optional, both or neither: the node / job totals on the device (i64[1] each, e.g. sss_prefix_rows' totals_dev) - n_nodes /
   * n_jobs above are then CAPACITIES (what the buffers hold; they also size the grids unless the hints say less) and nothing
   * on the host needs the real totals: the launches read them (sss_gnn_args::n_rows_dev) */
  const int64_t* n_nodes_dev;
  const int64_t* n_jobs_dev;
  int64_t n_nodes_hint, n_jobs_hint; /* with the pointers: roughly the real totals (grid sizes); <= 0: use the capacities */
  int64_t max_obs_nodes_hint;        /* roughly the node count of the LARGEST observation (e.g. row 32 of an earlier pass's
                                        sss_decima_graph counters, read back lazily); <= 0: unknown. layers_mode 0 takes the one
                                        launch while it is at most 192 (up to 2048 observations) / 64 (more): that launch ends
                                        with its largest observation */
} sss_gnn_encode_args;
int sss_gnn_encode(const sss_gnn_encode_args* a, void* stream);

/* The weight and bias gradient of a Linear layer over a minibatch (what autograd's AddmmBackward
 * computes inside the reference's loss.backward(), trainers/ppo.py:129-131 / schedulers/scheduler.py:44-54):
 *   gw[n][m] = sum_k dy[k][n] * x[k][m],  gb[n] = sum_k dy[k][n]   for x f32[K][ldx] (M columns used), dy f32[K][ldy]
 * (N columns used), M, N in 1..64. scratch_dev: f32 workspace of sss_linear_wgrad_scratch(M, N) floats. gb_dev may be
 * NULL. Launches on the CURRENT device's stream `stream` (no handle). fp32 throughout; the sum runs in a fixed order. */
int64_t sss_linear_wgrad_scratch(int M, int N);
int sss_linear_wgrad(const float* x_dev, int64_t ldx, const float* dy_dev, int64_t ldy, int64_t K, int M, int N, float* gw_dev, float* gb_dev,
                     float* scratch_dev, void* stream);

/* The per-step bookkeeping of the rollout workers for all envs at once (trainers/rollout_worker.py:133-159 sync, :162-206
 * async, with spark_sched_sim/wrappers StochasticTimeLimit's truncation rule), two launches around sss_step:
 *   phase 0: stage_idx[b] = active[b] ? stage_sel[b] : SSS_SKIP_ENV, num_exec[b] = max(1, 1 + exec_sel[b])
 *   phase 1: from the step's outputs (obs_f64 = [reward, wall_time], obs_i32[6] terminated, [7] error code) and time_limit:
 *            an env with an error code leaves the collection (pending_reset set, its step not recorded); row t of the
 *            [T][num_envs] record arrays (active, reward - 0 for frozen envs -, the sample, times, reset flag):
 *              sync:  t_before = the env's clock before the step, t_after = after it; the env stops when its episode ends
 *              async: t_before / t_after = simulated time collected before / after; resets = the episode ended (the caller
 *                     resets those envs; their clock restarts at 0); the env stops when `duration` is reached
 *            wall / elapsed / step_counts / active are updated in place;
 *            flags (i32[8], zero on entry, OR-ed): [0] an env failed, [1] an episode ended, [2] an env goes on,
 *            [3] 1 + index of a failed env, [4] an env was recorded.
 * Launches on the CURRENT device's stream `stream` (no handle). */
typedef struct sss_collect_args {
  int32_t num_envs;
  int32_t asynchronous;
  int64_t t;
  double duration;
  const double* obs_f64_dev;
  const int32_t* obs_i32_dev;
  int64_t obs_i32_stride;
  const double* time_limit_dev;
  uint8_t* active_dev;
  double* wall_dev;
  double* elapsed_dev;
  int64_t* step_counts_dev;
  uint8_t* pending_reset_dev;
  const int64_t* stage_sel_dev;
  const int64_t* job_idx_dev;
  const int64_t* exec_sel_dev;
  const float* lgprob_dev;
  int32_t* stage_idx_dev;
  int32_t* num_exec_dev;
  uint8_t* rec_active_dev;
  double* rec_t_before_dev;
  double* rec_t_after_dev;
  double* rec_rewards_dev;
  int64_t* rec_stage_sel_dev;
  int64_t* rec_job_idx_dev;
  int64_t* rec_exec_sel_dev;
  float* rec_lgprobs_dev;
  uint8_t* rec_resets_dev;
  int32_t* flags_dev;
} sss_collect_args;
int sss_collect_step(const sss_collect_args* a, int phase, void* stream);

/* One MLP of Decima's networks (schedulers/decima/utils.py:44-64: Linear - act - Linear - act - Linear) over a minibatch of
 * rows, forward and backward, for the PPO update (trainers/ppo.py:104-138 -> scheduler.py:101-139 -> the nn.Sequential
 * forward / autograd backward of every MLP). All tensors f32, row-major, contiguous.
 *   forward:  a1 = act(W1 x + b1) [rows,h1], a2 = act(W2 a1 + b2) [rows,h2], y = W3 a2 + b3 [rows,out_dim]   (a1, a2, y written)
 *   backward: g2 = (W3^T dy) * act'(a2), g1 = (W2^T g2) * act'(a1), dx = W1^T g1 (dx_dev NULL: not computed) - g1 / g2 are the
 *             gradients w.r.t. the two hidden layers' pre-activations, so that the parameter gradients are
 *             sss_linear_wgrad(x = a2, dy = dy), (a1, g2), (x, g1).
 * w_dev: the MLP's parameters packed [W1 (h1 x in), b1, W2^T (h1 x h2), b2, W3 (out x h2), b3] as for sss_gnn_launch.
 * act: 0 LeakyReLU(slope), 1 Tanh. Shapes: the seven MLPs of config/decima_tpch.yaml:66-78 - (in, 32, 16, 16, LeakyReLU)
 * with in = 5 / 16 / 21 and (in, 64, 64, 1, Tanh) with in = 53 / 36; sss_mlp_supported says whether a shape is one of them
 * (anything else: error). Launches on the CURRENT device's stream `stream` (no handle). fp32 FMAs in a fixed order. */
typedef struct sss_mlp_args {
  int64_t rows;
  int32_t in_dim, h1, h2, out_dim;
  int32_t act;
  float slope;
  const float* w_dev;
  const float* x_dev;  /* forward */
  float* a1_dev;
  float* a2_dev;
  float* y_dev;        /* forward */
  const float* dy_dev; /* backward */
  float* g1_dev;       /* backward */
  float* g2_dev;       /* backward */
  float* dx_dev;       /* backward, nullable */
  /* the input rows in two pieces (sss_mlp_split_supported(in_dim); NULL otherwise): columns 0 .. in_dim - 17 from x_dev (rows of
   * in_dim - 16 floats), the last 16 columns from x2_dev (rows of 16 floats) - the DAG encoder's torch.cat([x, h_node], -1)
   * (schedulers/decima/scheduler.py:246-262) is never built; the first Linear then adds the x2 features first (the MLP on the
   * concatenation up to the order of fp32 additions). sss_mlp_forward and sss_mlp_backward_wgrad without stored activations
   * only; dx2_dev (sss_mlp_backward_wgrad, instead of dx_dev): the gradient w.r.t. the x2 piece, f32[rows][16] */
  const float* x2_dev;
  float* dx2_dev;
} sss_mlp_args;
int sss_mlp_supported(int in_dim, int h1, int h2, int out_dim, int act);
/* 1: for the (in_dim) -> 32 -> 16 -> 16 LeakyReLU MLP sss_mlp_forward may be called with a1_dev == a2_dev == NULL (the hidden
 * activations are not stored) and sss_mlp_backward_wgrad with the same two NULL: it then computes them again from x_dev - same
 * instructions, same bits as the stored ones. Stored activations are two thirds of these kernels' memory traffic and 48 floats
 * per row of the update's memory (what autograd keeps alive for nn.Sequential in the reference, ppo.py:104-138). 0: this build keeps them. */
int sss_mlp_recompute_supported(int in_dim);
/* 1: sss_mlp_forward / sss_mlp_backward_wgrad of the (in_dim) -> 32 -> 16 -> 16 MLP take x2_dev / dx2_dev (see sss_mlp_args) */
int sss_mlp_split_supported(int in_dim);
int sss_mlp_forward(const sss_mlp_args* a, void* stream);
int sss_mlp_backward(const sss_mlp_args* a, void* stream);
/* sss_mlp_backward with the six parameter gradients in the same pass, for the (5 | 16 | 21) -> 32 -> 16 -> 16 LeakyReLU MLPs and
 * (sss_mlp_wgrad_scratch(in_dim) > 0 says whether this build does) the two policy heads (53 | 36) -> 64 -> 64 -> 1 Tanh:
 * x_dev, a1_dev, a2_dev (both NULL: recomputed from x_dev, see sss_mlp_recompute_supported - the GNN-shaped MLPs only), dy_dev in,
 * dx_dev out (nullable); g1 / g2 are not written. The weight / bias gradients are ADDED to
 * per-workgroup slots of acc_dev (f32[sss_mlp_wgrad_scratch(in_dim)], 0 for any other input width; zeroed by the caller before the
 * first call of a group of calls whose gradients belong together - the layers of the message passing); sss_mlp_wgrad_finish adds
 * the slots in a fixed order into gw1 [h1][in_dim], gb1 [h1], gw2 [h2][h1], gb2 [h2], gw3 [out][h2], gb3 [out]. Same inputs, same
 * bits. What the reference runs here: autograd's AddmmBackward / TanhBackward chain inside loss.backward() (trainers/ppo.py:129-131). */
int64_t sss_mlp_wgrad_scratch(int in_dim);
int sss_mlp_backward_wgrad(const sss_mlp_args* a, float* acc_dev, void* stream);
int sss_mlp_wgrad_finish(int in_dim, const float* acc_dev, float* gw1_dev, float* gb1_dev, float* gw2_dev, float* gb2_dev, float* gw3_dev, float* gb3_dev, void* stream);

/* The rollout workers' record of observations, built while collecting (trainers/rollout_worker.py:133-159 appends every
 * observation to its buffer; trainers/trainer.py:208-233 with schedulers/decima/utils.py:117-204 collates them into one batch graph
 * for the update): the compact graph of one step - the arrays sss_decima_graph_build wrote, `totals_dev` = sss_prefix_rows'
 * totals [nodes, edges, jobs, ..] - is appended to the arena's arrays at the cursors in `cursor_dev` (i64[8], on the device:
 * [0..3] rows appended so far of the node / edge / job / observation arrays, [4] steps appended, [5] set to 1 instead when
 * something would not fit `capacity` - nothing is written then). An array is copied as `per_row` elements of `elem_bytes`
 * (1, 4, 8) per row of its `kind` (0 nodes, 1 edges, 2 jobs, 3 observations = n_obs rows per step); 8-byte id arrays get the
 * cursor of what they name added (`shift`: 0 none, 1 node ids, 2 job ids, 3 observation ids). No device->host traffic.
 * `rows_hint`: roughly the largest number of elements an array has this step (grid size only; <= 0: a default). */
#define SSS_ARENA_MAX_ARRAYS 24
typedef struct sss_arena_array {
  const void* src_dev;
  void* dst_dev;
  int32_t elem_bytes, per_row, kind, shift;
} sss_arena_array;
typedef struct sss_arena_args {
  int32_t n_arrays, n_obs;
  const int64_t* totals_dev;
  int64_t* cursor_dev;
  int64_t capacity[4];
  int64_t rows_hint;
  sss_arena_array arrays[SSS_ARENA_MAX_ARRAYS];
} sss_arena_args;
int sss_arena_append(const sss_arena_args* a, void* stream);

/* What the trainer computes from the collected rollouts before the PPO epochs, over [T][B] records (row = step, column = env;
 * active_dev u8[T][B] marks the rows an env recorded - a prefix of its column), all f64, row-major, on the CURRENT device:
 *   sss_discounted_returns   R_k = r_k + exp(-beta * 1e-3 * (t_after_k - t_before_k)) * R_{k+1} per env from its last row
 *                            (trainers/utils/returns_calculator.py:67-76); out = 0 on rows that are not active
 *   sss_sequence_baselines   envs g*R .. g*R+R-1 are the rollouts of one job sequence: out[t][b] = mean over the sequence's
 *                            rollouts j of numpy.interp(times[t][b], times[:n_j][j], values[:n_j][j]) (trainers/utils/baselines.py:
 *                            12-37, trainer.py:206-207); n_dev i64[B] = recorded rows per env; skip_empty != 0: rollouts with
 *                            n = 0 are left out of the mean. The arithmetic is numpy's, operation by operation - the mean's sum in
 *                            numpy's pairwise order (sequential below 8 rollouts, eight partial sums from 8 on, halved above 128). */
typedef struct sss_returns_args {
  int64_t T, B;
  const uint8_t* active_dev;
  const double* t_before_dev;
  const double* t_after_dev;
  const double* rewards_dev;
  double beta;
  double* out_dev;
} sss_returns_args;
typedef struct sss_baseline_args {
  int64_t T, B;
  int32_t R, skip_empty;
  const uint8_t* active_dev;
  const double* times_dev;
  const double* values_dev;
  const int64_t* n_dev;
  double* out_dev;
} sss_baseline_args;
int sss_discounted_returns(const sss_returns_args* a, void* stream);
int sss_sequence_baselines(const sss_baseline_args* a, void* stream);

/* Differential (average-reward) returns over the same [T][B] record, in two calls so that several ranks can pool their sums
 * between them (one all-reduce of sums_dev). Everything is f64 on the CURRENT device; nothing comes back to the host.
 *   sss_reward_window_update  the moving window of (dt, reward) rows behind `avg_num_jobs` - the CircularArray of
 *                             trainers/utils/returns_calculator.py:6-22, fed as in :52-55 - as f64[cap][2], zero before the first
 *                             call. The record's rows (t_after - t_before, reward) with dt > 0 are taken env by env (env 0's active
 *                             steps in step order, then env 1's, ...: the reference's chain(*deltas_list)); of more than cap new
 *                             rows the last cap count; the window's last cap - n rows move to its front and the n new rows follow.
 *                             window_dev[current] is the window before the call and is left as it was; the window after the call
 *                             is window_dev[1 - current] (every row of it is written) - unless T == 0 or B == 0: then nothing
 *                             moves and the window stays window_dev[current]. The caller keeps count of which one is current.
 *                             sums_dev[0] = total time, sums_dev[1] = reward sum of the window after the call: each
 *                             0.0 + row[0] + row[1] + ... + row[cap - 1] in row order over all cap rows (numpy's axis-0 sum of the
 *                             (cap, 2) array adds in this order; the order is fixed, so the bits are).
 *                             scratch_dev: SSS_REWARD_WINDOW_SCRATCH(T, B) int64 of workspace, contents irrelevant.
 *   sss_differential_returns  avg = -sums_dev[1] / sums_dev[0] (nan for a window without rows, as in the reference), written to
 *                             avg_dev[0] (may be NULL); per env from its last row R = -(-r - dt * avg) + R
 *                             (returns_calculator.py:52-65, 78-89); out = 0 on rows that are not active. */
#define SSS_REWARD_WINDOW_CHUNK 64
#define SSS_REWARD_WINDOW_SCRATCH(T, B) ((((T) + SSS_REWARD_WINDOW_CHUNK - 1) / SSS_REWARD_WINDOW_CHUNK + 1) * (B) + 1)
struct sss_reward_window_args {
  int64_t T, B;
  const uint8_t* active_dev;
  const double* t_before_dev;
  const double* t_after_dev;
  const double* rewards_dev;
  int64_t cap;            /* rows of the window, >= 1 */
  double* window_dev[2];  /* f64[cap][2] each, 16-byte aligned (a row is read as one 16-byte load) */
  int32_t current;        /* 0 or 1 */
  int32_t pad_;
  int64_t* scratch_dev;
  double* sums_dev;       /* f64[2] */
};
typedef struct sss_reward_window_args sss_reward_window_args;
struct sss_diffret_args {
  int64_t T, B;
  const uint8_t* active_dev;
  const double* t_before_dev;
  const double* t_after_dev;
  const double* rewards_dev;
  const double* sums_dev; /* f64[2]: this rank's, or the ranks' sums added up */
  double* out_dev;        /* f64[T][B] */
  double* avg_dev;        /* f64[1] or NULL */
};
typedef struct sss_diffret_args sss_diffret_args;
int sss_reward_window_update(const sss_reward_window_args* a, void* stream);
int sss_differential_returns(const sss_diffret_args* a, void* stream);

/* Row gathers / scatters of the PPO update (what PyG's message passing, the score networks' `torch.cat([x[idx], h[idx], ..])`
 * inputs and the per-job / per-observation sums run as index_select / index_add_ under autograd in the reference:
 * schedulers/decima/scheduler.py:209-232, :246-283, :289-318, :337-385). `a` is the list side (row i, leading dimension ld_a
 * floats - it may be a column slice of a wider matrix), `b` / `c` the table side (row idx[i], contiguous rows of `width` floats):
 *   SSS_ROWS_GATHER       a[i] = b[idx[i]]
 *   SSS_ROWS_SCATTER_ADD  b[idx[i]] += a[i]                  (float atomics: the order of the additions into a row is not fixed;
 *                         SSS_ROWS_ORDERED_ADD is the same sum in a fixed order)
 *   SSS_ROWS_UPDATE       b[idx[i]] = a[i] + c[idx[i]]       (idx without repeats)
 *   SSS_ROWS_TAKE         a[i] = b[idx[i]], b[idx[i]] = 0, c[idx[i]] += a[i]     (idx without repeats)
 *   SSS_ROWS_SCATTER      b[idx[i]] = a[i]                   (idx without repeats)
 *   SSS_ROWS_SEGMENT_SUM  b[s] = sum of a[i], idx[s] <= i < idx[s + 1]  (idx: n + 1 non-decreasing row offsets of the n segments;
 *                         no atomics, the additions run in row order)
 *   SSS_ROWS_ORDERED_ADD  b[t] = (((b[t] + a[p(i0)]) + a[p(i0 + 1)]) + ...) + a[p(i1 - 1)] for every maximal run i0 .. i1 - 1 of
 *                         equal keys t = idx[i], p(i) = perm_dev[i] (perm_dev NULL: p(i) = i). PRECONDITION: idx is NON-DECREASING
 *                         (not checked; sort the keys stably and pass the sort's permutation as perm_dev). No atomics: one thread
 *                         group owns a run and adds in that fixed order, so every launch gives the same bits (the deterministic
 *                         mode's scatter-add, spark_sched_sim_amd/train_kernels.py)
 * idx entries must be valid rows of the tables (not checked). Launches on the CURRENT device's stream `stream` (no handle). */
#define SSS_ROWS_GATHER 0
#define SSS_ROWS_SCATTER_ADD 1
#define SSS_ROWS_UPDATE 2
#define SSS_ROWS_TAKE 3
#define SSS_ROWS_SCATTER 4
#define SSS_ROWS_SEGMENT_SUM 5
#define SSS_ROWS_ORDERED_ADD 6
typedef struct sss_rows_args {
  int64_t n;              /* rows of the list */
  int64_t ld_a;           /* floats between rows of a (>= width) */
  int32_t width;          /* floats per row, 1..64 */
  int32_t op;             /* SSS_ROWS_* */
  const int64_t* idx_dev; /* i64[n] (SEGMENT_SUM: i64[n + 1]) */
  float* a_dev;
  float* b_dev;
  float* c_dev;           /* UPDATE / TAKE only */
  const int64_t* perm_dev; /* ORDERED_ADD only: i64[n] or NULL */
} sss_rows_args;
int sss_rows_op(const sss_rows_args* a, void* stream);

/* Several tables side by side - the score networks' input rows torch.cat([t_0[idx_0], t_1[idx_1], ...], -1) of
 * schedulers/decima/scheduler.py:289-318 / :337-385 - in ONE launch that walks `out` as a flat array (csrc/sss_rows.h):
 *   op 0  out[i][off_k + j] = table_k[idx_k[i]][j]       for every part k (idx_k NULL: row i itself)
 *   op 1  table_k[idx_k[i]][j] += out[i][off_k + j]      (the backward pass; float atomics; parts with table_dev NULL are skipped)
 * off_k = the widths of the parts before k; out_dev f32[n][sum of widths <= 64] contiguous, table_k f32[rows_k][width_k] contiguous. */
typedef struct sss_concat_part {
  float* table_dev;
  const int64_t* idx_dev; /* i64[n], nullable */
  int32_t width;          /* floats per row of the table, 1..64 */
  int32_t pad_;
} sss_concat_part;
typedef struct sss_concat_args {
  int64_t n;       /* rows */
  int32_t n_parts; /* 1..4 */
  int32_t op;
  float* out_dev;
  sss_concat_part parts[4];
} sss_concat_args;
int sss_rows_concat(const sss_concat_args* a, void* stream);

/* Log-probability of the recorded action and entropy of a categorical distribution per SEGMENT of a flat score array - the PPO
 * update's evaluate_actions (schedulers/decima/utils.py:26-41 `evaluate`: segment softmax, torch.distributions' clamp of the
 * probabilities to [eps, 1 - eps], log, the chosen entry, -sum p log p; scheduler.py:101-139 the same over the executor counts
 * a job allows), forward (backward = 0: lg_dev, ent_dev written) and backward (backward = 1: g_scores_dev written from g_lg_dev,
 * g_ent_dev). Segment s = rows ptr[s] .. ptr[s + 1] - 1 of scores_dev; chosen[s] counts inside the segment; an empty segment
 * gives lg = ent = 0. den_eps is added to the sum of exponentials (1e-16 in decima/utils.py:35, 0 for torch.softmax). */
typedef struct sss_segcat_args {
  int64_t n_seg;
  const float* scores_dev;   /* f32[rows] */
  const int64_t* ptr_dev;    /* i64[n_seg + 1], non-decreasing */
  const int64_t* chosen_dev; /* i64[n_seg] */
  float den_eps;
  int32_t pad_;
  float* lg_dev;             /* forward out f32[n_seg] */
  float* ent_dev;            /* forward out f32[n_seg] */
  const float* g_lg_dev;     /* backward in f32[n_seg] */
  const float* g_ent_dev;    /* backward in f32[n_seg] */
  float* g_scores_dev;       /* backward out f32[rows] */
} sss_segcat_args;
int sss_segment_categorical(const sss_segcat_args* a, int backward, void* stream);

/* Executor timelines: the reference's `Executor.history` (spark_sched_sim/components/executor.py:21-44 - per executor the list of
 * [t, job_id] pairs, t = the wall time at which the executor was released from job_id, None while it has not been; job_id -1 = the
 * common pool), recorded by the simulator kernels themselves into caller-allocated rows OUTSIDE the state arena:
 *   t_dev f64[num_envs][E][cap], job_dev i32[num_envs][E][cap], count_dev i32[num_envs][E]        (E = num_executors)
 * Entry k < count - 1 holds its release time, the open (last) entry's time slot holds NaN. An episode initialisation (sss_reset
 * for the envs of its mask, an auto-reset inside a step / rollout launch) restarts the env's rows at one open entry [NaN, -1]; an executor
 * arriving at a job (spark_sched_sim.py:444-445) and a release to the common pool (:778-782) each close the open entry with the
 * time of the event being handled and open the next one; a send (:627-629) writes nothing. count is the TRUE number of entries and
 * may exceed cap: entries from index cap on are not stored (the release time of entry cap - 1 still is). Nothing outside the three
 * arrays is ever written; envs skipped with SSS_SKIP_ENV keep their rows. (The two structures below have no typedef: C callers
 * write `struct sss_timeline`.) Binding does not touch the rows: they describe an episode
 * from its reset on (or from a caller's own [NaN, -1] / count 1 initialisation). tl == NULL unbinds; with nothing bound every
 * output and the whole arena are byte for byte what they are without this feature. */
struct sss_timeline {
  double* t_dev;
  int32_t* job_dev;
  int32_t* count_dev;
  int32_t cap; /* entries stored per executor, >= 1 */
  int32_t pad_;
};
int sss_bind_timeline(sss_handle* h, const struct sss_timeline* tl);

/* The bound timelines of n envs as Gantt frames (what the reference's renderer draws from the histories, components/renderer.py,
 * spark_sched_sim.py:408-424; "rgb_array"): rgb_dev u8[n][height][width][3], env_ids_dev i32[n] or NULL (= envs 0 .. n - 1; an id
 * outside [0, num_envs) leaves its frame untouched). A frame is defined by these rules, all in fp64, T = the env's wall time, J = the
 * episode's job count: executor i owns pixel rows [i * rh, min((i + 1) * rh, height)), rh = ceil(height / E); column x shows the
 * entry in force at tx = (x + 0.5) * (T / width) - the first entry k with tx < release_k, the open entry's release being +inf (so
 * entries of zero length are never chosen); T <= 0: the open entry everywhere. Job j >= 0 is drawn in trunc(c1 + p * (c2 - c1)) per
 * channel, p = (j + 1) / J, c1 = (0, 100, 255), c2 = (2, 247, 112); -1 is black. A row with count > cap is mid-grey (128, 128, 128)
 * from the release time of its last stored entry on. Then every job with t_completed < T draws a red (255, 0, 0) column over the whole
 * height at x = min(width - 1, floor(width * t_completed / T)). width, height in 1..16384. */
struct sss_timeline_render_args {
  const int32_t* env_ids_dev;
  int32_t n, width, height, pad_;
  uint8_t* rgb_dev;
};
int sss_timeline_render(sss_handle* h, const struct sss_timeline_render_args* a, void* stream);

/* The episode metrics of every env in one launch, one wavefront per env, from the env's block of the state arena (t_arrival,
 * t_completed, the duration ring, and wall_time, next_arrival, n_completed, n_active, dur_n, dur_head of its header). Nothing is
 * written to the arena. The definitions are those of the reference's host functions (spark_sched_sim/metrics.py:4-23,
 * spark_sched_sim.py:243-245), every sum in the ORDER the host takes - the order is the definition, the results carry the host's bits:
 *   n = next_arrival; d_j = min(t_completed[j], wall_time) - t_arrival[j] for j < n, in job-id order
 *   stats[0] = n
 *   stats[1] = ((0.0 + d_0) + d_1) + ...                                        (Python's sum)
 *   stats[2] = numpy.mean(d): numpy's pairwise summation order, then one division by n; NaN for n = 0
 *   stats[3] = stats[1] / wall_time                                             (IEEE division: NaN at wall_time == 0 with no jobs)
 *   stats[4] = numpy.mean(the ring's dur_n entries from dur_head on, i.e. in deque order) * 1e-3; NaN for an empty ring
 *   stats[5], [6], [7] = n_completed, n_active, wall_time
 *   pct[k] = numpy.percentile(d, q[k]), default method: d sorted ascending, quant = q / 100,
 *            vi = (n - 1) * quant (numpy's own index of its "linear" method), lo = floor(vi), hi = lo + 1, both n - 1 where
 *            vi >= n - 1 and 0 where vi < 0, g = vi - lo, result a + (b - a) * g, replaced by b - (b - a) * (1 - g) where g >= 0.5
 *            (a, b = the sorted values at lo, hi); NaN for n = 0
 * q_dev f64[n_q], n_q in 0..16, every value in [0, 100] (the caller's duty - the values live on the device; the kernel gives NaN
 * for any other). stats_dev f64[num_envs][8], pct_dev f64[num_envs][n_q]; sorted_dev (nullable) f64[num_envs][job_cap] receives
 * the sorted durations, the rest of a row NaN; active_dev (nullable) u8[num_envs]: the rows of envs with 0 are left untouched.
 * job_cap <= 1024. (Plain parameters, like sss_prefix_rows: there is no argument structure to keep in step with the binding.) */
int sss_job_stats(sss_handle* h, int n_q, const double* q_dev, double* stats_dev, double* pct_dev, double* sorted_dev, const uint8_t* active_dev,
                  void* stream);

/* Copies of running environments: what `copy.deepcopy(env)` is for the reference's SparkSchedSimEnv (every field that
 * spark_sched_sim/spark_sched_sim.py:34-125 sets up and an episode changes - the clock, the event queue, executors with their
 * histories, jobs, the executor tracker's pools and commitments, the sampler's generator, the duration deque - plus the last
 * observation). n env IMAGES go from a source STORE to a destination store in one launch, one workgroup per pair
 * (src_ids_dev[k] -> dst_ids_dev[k], i32[n] each). A store is the set of per-env buffers an env lives in: a state arena of
 * env_stride-byte blocks, the six observation buffers of sss_buffers and, optionally, the three timeline arrays of sss_timeline,
 * each with num_slots rows. A NULL store stands for the buffers bound to the handle (with its bound timeline, if any), so the
 * same call is
 *   fork      src_store = dst_store = NULL: env -> env in one handle
 *   snapshot  dst_store = slots the caller allocated (sized by sss_dims; state_dev 256-byte aligned)
 *   restore   src_store = such slots - also ones filled from ANOTHER handle of the same layout
 * layout_id is the sss_env_layout_id of the handle a caller's store was filled by (or sized for): the layout of an env's block -
 * executor, job, stage, level, node and edge capacities, every offset, the block size, the kernel instantiation - and the workload
 * pack (job records hold indices into it), hashed; num_envs is not part of it. A store whose id differs from the handle's is refused with -51: images only exist between equal layouts.
 * An image is
 *   - the block of the arena except (a) the table slots, in the pool overflow area, of pools whose record says the table has 8
 *     entries - those slots are never interpreted - and (b) the destination's lifetime counters n_steps, n_events, model_bytes,
 *     prof[5], n_fast, n_batched, n_rounds, which stay the destination's (sums over a store do not change). Everything else
 *     is the source's: a step cut at its event budget (sss_step_bounded) goes on in the copy, err / err_line, the episode counters
 *     and the episode's seed (an auto-reset of the copy therefore continues the SOURCE's seed schedule) come along;
 *   - the live prefix of the observation rows: n_nodes node rows, n_edges edge rows, n_jobs + 1 entries of dag_ptr, n_jobs of
 *     exec_supplies (counts: the source's obs_i32 row), the obs_i32 and obs_f64 rows; the copy's next observation relies on the
 *     edge rows exactly as the source's would;
 *   - when BOTH stores have timeline arrays, per executor min(count, cap of either) entries and count; else no timeline row is
 *     read or written.
 * reseed_dev (nullable, u64[n]): after the copy the destination's generator is numpy's Generator(PCG64(SeedSequence(seed))) afresh.
 * Job arrivals are all drawn at reset, so such a copy keeps the job sequence and draws its own task durations from there on.
 * A pair with an id outside its store is skipped. Destination ids must be distinct and, when both stores are the same buffers,
 * disjoint from the source ids - the caller's duty, the ids live on the device: otherwise an image may be garbage, but nothing
 * outside the two stores is read or written. Nothing outside the destination images is written. n == 0 does nothing. The launch
 * is asynchronous on `stream`. (The two structures have no typedef, like sss_timeline's.) */
struct sss_env_store
{
  void* state_dev;            /* u8[num_slots][env_stride] */
  float* nodes_dev;           /* f32[num_slots][node_cap][3] */
  int32_t* edge_links_dev;    /* i32[num_slots][edge_cap][2] */
  int32_t* dag_ptr_dev;       /* i32[num_slots][job_cap + 1] */
  int32_t* exec_supplies_dev; /* i32[num_slots][job_cap] */
  int32_t* obs_i32_dev;       /* i32[num_slots][obs_i32] */
  double* obs_f64_dev;        /* f64[num_slots][obs_f64] */
  double* tl_t_dev;           /* f64[num_slots][E][tl_cap], or all three NULL: no timeline rows */
  int32_t* tl_job_dev;        /* i32[num_slots][E][tl_cap] */
  int32_t* tl_count_dev;      /* i32[num_slots][E] */
  int32_t tl_cap;
  int32_t num_slots;
  uint64_t layout_id;
};
struct sss_env_copy_args
{
  const struct sss_env_store* src_store; /* NULL: the handle's bound buffers */
  const struct sss_env_store* dst_store;
  const int32_t* src_ids_dev;
  const int32_t* dst_ids_dev;
  const uint64_t* reseed_dev;
  int32_t n, pad_;
};
uint64_t sss_env_layout_id(const sss_handle* h);
int sss_env_copy(sss_handle* h, const struct sss_env_copy_args* a, void* stream);

/* The fused rollout with a policy PER ENV: sss_rollout for the envs that take part, each under its own on-device policy, the others
 * untouched - what a lookahead needs of the fused kernel (children of one state under different policies in one launch while their
 * parents sit still; the reference has no counterpart: its schedulers are host objects, one env per process). Every array is per
 * env of the handle, i32[num_envs]:
 *   policy_dev        the policy id of the env's steps, the ids of sss_policy. -1: env i is left completely untouched - state,
 *                     observation rows, outputs and counters stay byte for byte, as under SSS_SKIP_ENV in sss_step - and none of
 *                     the outputs below is written for it
 *   param_dev         that policy's param
 *   first_policy_dev, first_param_dev   (both NULL, or both given) the policy and param of the env's FIRST step in this launch; a
 *                     negative first_policy entry, like NULL, means policy_dev / param_dev. "Child k plays candidate k throughout"
 *                     and "child k takes candidate k's action, then the base policy" are the same call
 *   n_steps           upper bound of steps per env, >= 0. There is NO auto-reset: an env stops at the end of its episode or at an
 *                     env error (as sss_rollout does with auto_reset == 0); an env that is over at entry takes no step and no byte
 *                     of it is written
 *   steps_dev         (nullable) out: steps the env took in this launch
 *   first_stage_dev, first_exec_dev   (nullable) out: the action (stage_idx, num_exec) of the first step taken; left alone when
 *                     the env took none
 * Per-step semantics are exactly those of sss_policy + sss_step, bit for bit; only the last observation survives.
 * The arrays live on the device and no sync is spent on reading them, so their CONTENTS are the caller's duty: for a policy id
 * outside the table (other than -1) or a weighted-fair alpha outside [-4, 4] - in either pair - the kernel leaves env i untouched and
 * reports steps_dev[i] = -1. Refused on the host with -52, before any launch: NULL policy_dev or param_dev, one of the first_* pair
 * without the other, n_steps < 0, and a bound timeline ("not available while a timeline is recorded": this kernel has no recording
 * form - unbind, or use sss_policy + sss_step). */
int sss_rollout_each(sss_handle* h, const int32_t* policy_dev, const int32_t* param_dev, const int32_t* first_policy_dev, const int32_t* first_param_dev,
                     int n_steps, int32_t* steps_dev, int32_t* first_stage_dev, int32_t* first_exec_dev, void* stream);

/* From the children of a lookahead to its decision, in one launch (one wavefront per parent; the arena is only read). Parent i
 * (parent_dev i32[n_parents], env ids) has n_candidates x n_samples children, child_dev i32[n_parents][n_candidates][n_samples]: env
 * ids of copies of the parent (sss_env_copy) that were played to the end of their episodes, candidate k's under the policies
 * cand_first_policy_dev[k], cand_first_param_dev[k] (first step) and cand_policy_dev[k], cand_param_dev[k] (after it), i32[n_candidates]
 * each - the kernel does not interpret these four, it hands them on.
 *   cost of a child   stats[1] of sss_job_stats for that env, the same bits: ((0.0 + d_0) + d_1) + ... with
 *                     d_j = min(t_completed[j], wall_time) - t_arrival[j] over the arrived jobs in job-id order
 *   a child is valid  when its episode is over without an env error (terminated != 0 and err == 0). Only then are the costs of two
 *                     children comparable: they cover the same jobs from arrival to completion. An id outside [0, num_envs) is invalid
 *   score of k        ((0.0 + cost[k][0]) + cost[k][1]) + ... in sample order, then ONE division by n_samples; NaN when any of k's
 *                     samples is invalid
 *   winner            the lowest score; ties go to the lowest k; a NaN never wins
 * Outputs: best_dev i32[n_parents] the winner, -1 when no candidate is valid; score_dev f64[n_parents][n_candidates]; and the
 * winner's quadruple - candidate 0's when there is no winner - written to env_first_policy_dev, env_first_param_dev, env_policy_dev,
 * env_param_dev (i32[num_envs] each) at index parent_dev[i]: arrays that are -1 elsewhere are the arguments of the sss_rollout_each
 * launch that steps the parents by the decision. A parent id outside [0, num_envs) gets its best / score rows and nothing else.
 * n_candidates, n_samples >= 1, n_candidates * n_samples <= 1024 (the kernel's LDS cost table), n_parents >= 0 (0 does nothing);
 * anything else, or a NULL array, fails with -53. (Plain parameters, like sss_job_stats.) */
int sss_lookahead_pick(sss_handle* h, int n_parents, int n_candidates, int n_samples, const int32_t* parent_dev, const int32_t* child_dev,
                       const int32_t* cand_first_policy_dev, const int32_t* cand_first_param_dev, const int32_t* cand_policy_dev,
                       const int32_t* cand_param_dev, int32_t* best_dev, double* score_dev, int32_t* env_first_policy_dev, int32_t* env_first_param_dev,
                       int32_t* env_policy_dev, int32_t* env_param_dev, void* stream);

/* sss_rollout_each with a STOP TIME, for a lookahead whose children do not play to the end of the episode. Everything said of
 * sss_rollout_each holds per env (policy -1 sits out untouched, a bad policy gives steps = -1, an env over at entry is not staged in,
 * no auto-reset, the first step's policy), with max_steps in the place of n_steps, and on top of it:
 *   horizon        a span of simulated time in the simulator's unit, > 0, +inf allowed. T = the env's wall_time at entry + horizon is
 *                  ONE f64 addition. Before each step the env stops if it is terminated, needs a reset, has taken max_steps, or its
 *                  wall_time >= T; so the first step is taken (unless rounding swallowed the horizon), and the env stops at the
 *                  first step boundary at or behind T: it can overshoot T by the length of its last step
 *   t_stop_dev     out, REQUIRED, f64[num_envs]: T, for every env that takes part - an env that is over at entry included
 *   rem_work_dev   (nullable) out, f64[num_envs][job_cap]: the env's row is written at exit - zero everywhere, then for every active
 *                  job j the work it still holds, rem_work[env][j] = sum from 0.0 over j's active stages in ascending stage id of
 *                  (double)(float)remaining_tasks * (double)most_recent_duration: the value the weighted-fair and SJF-CP policies
 *                  compute, bit for bit. An env that is over at entry gets a zero row
 * With horizon = +inf the env's bytes, steps and first action are those of sss_rollout_each(.., n_steps = max_steps, ..).
 * Refused on the host with -54, before any launch: NULL policy_dev, param_dev or t_stop_dev, one of the first_* pair without the
 * other, horizon NaN or <= 0, max_steps < 0, and a bound timeline ("not available while a timeline is recorded"). */
int sss_rollout_until(sss_handle* h, const int32_t* policy_dev, const int32_t* param_dev, const int32_t* first_policy_dev, const int32_t* first_param_dev,
                      double horizon, int max_steps, int32_t* steps_dev, int32_t* first_stage_dev, int32_t* first_exec_dev, double* t_stop_dev,
                      double* rem_work_dev, void* stream);

/* sss_lookahead_pick for children that stopped at a time horizon (sss_rollout_until, whose t_stop_dev and rem_work_dev it takes):
 * the same arguments, scores, winner, fallback and per-env arrays - only a child's validity and cost differ. For child c let w be its
 * wall_time, T = t_stop_dev[c], n its number of arrived jobs, N = num_executors. The order of every sum is part of the definition.
 *   valid          err == 0 and (terminated != 0 or w >= T), the id inside [0, num_envs). A child that max_steps stopped short of
 *                  its horizon is invalid: its cost is NaN and its candidate cannot win
 *   counted jobs   j < n with t_arrival[j] < T. Arrival times are drawn at reset and are the same in every child of a parent (a
 *                  reseeded child draws other task durations, not other arrivals), and every valid child has reached T or its end:
 *                  all children of a parent count the SAME jobs, which is what makes their costs comparable
 *   tail == 0      (none) cost = ((0.0 + d_0) + d_1) + ... over the counted jobs in id order with
 *                  d_j = min(t_completed[j], min(T, w)) - t_arrival[j]: every child is charged up to the common time T, nothing beyond
 *   tail == 1      (srpt) d_j = min(t_completed[j], w) - t_arrival[j], summed the same way: charged up to the child's own stop. Unless
 *                  the child is terminated a tail is added: W_j = rem_work_dev[c][j] of the counted jobs with t_completed[j] > w,
 *                  sorted ascending W_(1) <= W_(2) <= ...; p_0 = 0.0, p_i = p_(i-1) + W_(i); tail = ((0.0 + p_1 / N) + p_2 / N) + ...;
 *                  cost = sum + tail. It is the flow time those jobs would still accrue if the N executors served them as one
 *                  machine, shortest remaining work first - an estimate that, unlike the total remaining work, tells orderings apart
 * Knowingly ignored: jobs that arrive in [T, w] compete for executors in a child that overshot T but are not charged; the overshoot
 * w - T itself is charged under srpt and clipped under none; the tail knows no precedence, no moving delay and no future arrival.
 * With T = +inf every job counts and every valid child is terminated: both forms give sss_lookahead_pick's cost, bit for bit.
 * A finite horizon carries NO guarantee: the lookahead may end above its candidates.
 * Errors as sss_lookahead_pick (-53), plus a NULL t_stop_dev / rem_work_dev and a tail other than 0 or 1. */
int sss_lookahead_pick_horizon(sss_handle* h, int n_parents, int n_candidates, int n_samples, const int32_t* parent_dev, const int32_t* child_dev,
                               const int32_t* cand_first_policy_dev, const int32_t* cand_first_param_dev, const int32_t* cand_policy_dev,
                               const int32_t* cand_param_dev, const double* t_stop_dev, const double* rem_work_dev, int tail, int32_t* best_dev,
                               double* score_dev, int32_t* env_first_policy_dev, int32_t* env_first_param_dev, int32_t* env_policy_dev,
                               int32_t* env_param_dev, void* stream);

/* sss_rollout_each with DECIMA among the policies: whole episodes of the learned scheduler in one launch, every env at its own pace,
 * and Decima as a candidate or base policy of a lookahead. Everything said of sss_rollout_each holds per env (policy -1 sits out
 * untouched, a bad id gives steps = -1, an env over at entry is not staged in, no auto-reset, the first step's policy, the three
 * outputs), with one more policy id:
 *   5 (Decima)     legal in policy_dev and in first_policy_dev; its param is ignored. A Decima step is the decision of
 *                  sss_decima_policy (greedy == 0) or sss_decima_policy_argmax (greedy != 0) on the env's current observation rows,
 *                  bit for bit, followed by the step of sss_step
 *   a              the policy kernel's arguments: weights, scales, work space and its six per-env outputs, which serve as the
 *                  hand-over inside the kernel and hold the env's LAST decision afterwards (an env that took no Decima step keeps
 *                  what they held). active_dev, stage_scores_dev, exec_scores_dev and prof_dev must be NULL: an env sits out with
 *                  policy -1, and of per-step scores only the last would survive
 *   rng_counter    the decision of the env's it-th step IN THIS LAUNCH (it = 0, 1, ..; steps under a heuristic count too) draws
 *                  with rng_counter + it; rng_seed, env and candidate key the draws as in sss_decima_policy. A lock-step loop that
 *                  passes rng_counter = c0 + t at its t-th iteration draws the same numbers. Ignored when greedy != 0
 *   policy_dev, param_dev   both NULL: every env plays Decima; else i32[num_envs] each, as for sss_rollout_each
 *   first_policy_dev, first_param_dev, n_steps, steps_dev, first_stage_dev, first_exec_dev   as for sss_rollout_each
 * One workgroup holds the simulator's LDS working set and Decima's (20 bytes per node slot) at once, so env layouts with many node
 * slots that the two-launch route still takes are refused here.
 * Refused on the host with -55, before any launch: a NULL a, or a NULL weight, work-space or output pointer in it; a non-NULL
 * active_dev, stage_scores_dev, exec_scores_dev or prof_dev; one of policy_dev / param_dev or of the first_* pair without the
 * other; n_steps < 0; a bound timeline ("not available while a timeline is recorded"); an env layout whose LDS working set does
 * not fit the 160 KB of a workgroup. (Plain parameters, like sss_job_stats.) */
int sss_rollout_decima(sss_handle* h, const sss_decima_policy_args* a, int greedy, const int32_t* policy_dev, const int32_t* param_dev,
                       const int32_t* first_policy_dev, const int32_t* first_param_dev, int n_steps, int32_t* steps_dev, int32_t* first_stage_dev,
                       int32_t* first_exec_dev, void* stream);

/* The K BEST decisions of the arg-max policy for every env in one launch: what sss_decima_policy_argmax computes, with k winners of
 * the stage decision instead of one - the candidates of a lookahead over the ACTIONS of a state. The launch shape is the policy
 * kernel's; the encoder (DAG analysis, embeddings, summaries) and the stage scores run ONCE per env, only the executor-count block
 * runs per slot.
 *   a              the policy kernel's arguments: weights, scales, work space; active_dev is honoured. stage_scores_dev,
 *                  exec_scores_dev, prof_dev and the six single-decision outputs are ignored and may be NULL; so are the rng fields
 *   k              slots per env, 1..64
 *   stage_idx_dev  i32[num_envs][k]: slot r (r = 0, 1, ..) holds the schedulable stage with the r-th largest key, as its rank among
 *                  the env's schedulable rows (the env's action format). The key is score + 0.0f, equal keys go to the lower node
 *                  index, a NaN or -inf key never enters: the policy's rule, applied r + 1 times with the earlier winners excluded
 *   num_exec_dev   i32[num_envs][k]: the arg-max executor count for THAT stage's job - the policy's second decision unchanged (the
 *                  job's cap, the source job capped at the committable count, ties to the lowest count)
 *   lgprob_dev     f32[num_envs][k]: the policy's log-probability of the (stage, count) pair; the stage term uses the policy's ONE
 *                  log-sum-exp over all schedulable stages and is not renormalised over the slots
 *   count_dev      i32[num_envs]: max(1, min(k, number of stages that can enter)) slots are filled. With nothing schedulable, or an
 *                  empty observation, slot 0 is the policy's (-1, 1, 0.0f) and count is 1. The slots at or behind count hold
 *                  stage_idx -1, num_exec -1 (the mark of an empty slot, see sss_rollout_action) and lgprob -inf. An env with
 *                  active == 0 gets count 0 and empty slots only
 *   exec_scores_dev (nullable) f32[num_envs][k][E]: row r holds the count scores of slot r's job, -inf beyond its cap - the policy's
 *                  exec_scores row when that job is chosen; -inf throughout for an empty slot
 * Slot 0 equals sss_decima_policy_argmax's stage_idx, num_exec and lgprob bit for bit.
 * Refused on the host with -56, before any launch: a NULL a, a NULL weight or work-space pointer in it, a NULL stage_idx_dev,
 * num_exec_dev, lgprob_dev or count_dev, k outside [1, 64], num_executors > 128. (Plain parameters, like sss_job_stats.) */
int sss_decima_topk(sss_handle* h, const sss_decima_policy_args* a, int k, int32_t* stage_idx_dev, int32_t* num_exec_dev, float* lgprob_dev,
                    int32_t* count_dev, float* exec_scores_dev, void* stream);

/* The per-env fused rollouts with a first ACTION per env: "take action a in state s, then follow the policy" - Q(s, a) by Monte
 * Carlo - in one launch. With a given it is sss_rollout_decima per env (policy id 5 is legal, policy_dev / param_dev both NULL: every
 * env plays Decima, the 160 KB LDS refusal applies); with a NULL it is sss_rollout_each per env (policy_dev and param_dev required,
 * id 5 gives steps = -1, the LDS working set is the simulator's alone). Two arrays take the place of the first-policy pair, both
 * REQUIRED, i32[num_envs]:
 *   first_exec_in_dev[i] >= 1   the env's first step in this launch takes (first_stage_in_dev[i], first_exec_in_dev[i]) verbatim, as
 *                  sss_step would; no policy is evaluated. An action the env refuses leaves the env in the error state sss_step
 *                  leaves it in, ends the env's part in the launch and is not counted in steps_dev. The step is it = 0 of
 *                  Decima's draw counter: the first decision behind it draws with rng_counter + 1
 *   first_exec_in_dev[i] == 0   no forced action: the first step is the env's policy's, the call is the existing kernels' for it
 *   first_exec_in_dev[i] < 0    the env sits out untouched, byte for byte, exactly like policy -1: an empty slot of sss_decima_topk
 *                  can be handed over unread
 * Everything else is the two existing calls': -1 sits out, a bad id gives steps = -1, an env that is over at entry is not staged
 * in, no auto-reset, steps_dev / first_stage_dev / first_exec_dev (the action of the first step TAKEN - the forced one where there
 * is one) and Decima's hand-over arrays are written as before.
 * Refused on the host with -57, before any launch: a NULL first_stage_in_dev or first_exec_in_dev; n_steps < 0; a bound timeline
 * ("not available while a timeline is recorded"); with a NULL: a NULL policy_dev or param_dev; with a given: everything
 * sss_rollout_decima refuses of it. (Plain parameters, like sss_job_stats.) */
int sss_rollout_action(sss_handle* h, const sss_decima_policy_args* a, int greedy, const int32_t* policy_dev, const int32_t* param_dev,
                       const int32_t* first_stage_in_dev, const int32_t* first_exec_in_dev, int n_steps, int32_t* steps_dev, int32_t* first_stage_dev,
                       int32_t* first_exec_dev, void* stream);

const char* sss_last_error(void);
void sss_destroy(sss_handle* h);

#ifdef __cplusplus
}
#endif
#endif
