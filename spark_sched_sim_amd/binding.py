"""ctypes binding of the C ABI in include/sss.h (libsss_hip.so, built by spark_sched_sim_amd/build.py).

The product path is the HIP library and nothing else: `load_library()` raises if it is missing
or cannot be loaded - there is no CPU fallback. (The test-suite can inject another library
object that exports the same ABI - the CPU wave emulator under tests/emu - through the `lib`
argument of `Binding`; that is test plumbing, not a fallback: nothing in this package looks for it.)
"""
from __future__ import annotations

import ctypes as C
import os.path as osp

CSRC = osp.join(osp.dirname(osp.abspath(__file__)), "csrc")
LIB_NAME = "libsss_hip.so"


class SssCfg(C.Structure):
    _fields_ = [("num_executors", C.c_int32), ("job_arrival_cap", C.c_int32), ("max_jobs", C.c_int32),
                ("reserved", C.c_int32), ("job_arrival_rate", C.c_double), ("moving_delay", C.c_double),
                ("warmup_delay", C.c_double), ("beta", C.c_double)]


class SssDims(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("num_executors", C.c_int32), ("job_cap", C.c_int32),
                ("stage_stride", C.c_int32), ("node_cap", C.c_int32), ("edge_cap", C.c_int32),
                ("obs_i32", C.c_int32), ("obs_f64", C.c_int32), ("state_bytes", C.c_int64),
                ("env_stride", C.c_int64), ("off_t_arrival", C.c_int64), ("off_t_completed", C.c_int64),
                ("off_jobs", C.c_int64), ("off_active", C.c_int64), ("off_dur_ring", C.c_int64),
                ("job_rec_bytes", C.c_int32), ("hdr_bytes", C.c_int32)]


class SssBuffers(C.Structure):
    _fields_ = [("state_dev", C.c_void_p), ("nodes_dev", C.c_void_p), ("edge_links_dev", C.c_void_p),
                ("dag_ptr_dev", C.c_void_p), ("exec_supplies_dev", C.c_void_p), ("obs_i32_dev", C.c_void_p),
                ("obs_f64_dev", C.c_void_p)]


class SssDecimaGraph(C.Structure):
    _fields_ = [("active_dev", C.c_void_p), ("node_off_dev", C.c_void_p), ("job_off_dev", C.c_void_p), ("edge_off_dev", C.c_void_p),
                ("num_tasks_scale", C.c_float), ("work_scale", C.c_float), ("x_dev", C.c_void_p), ("node_obs_dev", C.c_void_p),
                ("node_loc_dev", C.c_void_p), ("node_job_dev", C.c_void_p), ("sched_rank_dev", C.c_void_p), ("gen_dev", C.c_void_p),
                ("node_recv_dev", C.c_void_p), ("stage_mask_dev", C.c_void_p), ("src_dev", C.c_void_p), ("dst_dev", C.c_void_p),
                ("edge_obs_dev", C.c_void_p), ("edge_layers_dev", C.c_void_p), ("job_obs_dev", C.c_void_p), ("job_cap_dev", C.c_void_p),
                ("job_first_dev", C.c_void_p), ("obs_depth_dev", C.c_void_p), ("job_nodes_dev", C.c_void_p), ("out_start_dev", C.c_void_p),
                ("out_deg_dev", C.c_void_p), ("layer_cnt_dev", C.c_void_p), ("sched_off_dev", C.c_void_p), ("sched_list_dev", C.c_void_p),
                ("layer_totals_dev", C.c_void_p), ("recv_lists_dev", C.c_void_p), ("recv_stride", C.c_int64), ("layer_totals_clear_dev", C.c_void_p),
                ("layer_totals_len", C.c_int64)]


class SssDecimaLists(C.Structure):
    _fields_ = [("node_off_dev", C.c_void_p), ("obs_nodes_dev", C.c_void_p), ("node_recv_dev", C.c_void_p), ("env_off_dev", C.c_void_p),
                ("layer_base", C.c_int64 * 32), ("recv_dev", C.c_void_p), ("n_layers", C.c_int)]


class SssDecimaPolicyArgs(C.Structure):
    _fields_ = [("active_dev", C.c_void_p), ("num_tasks_scale", C.c_float), ("work_scale", C.c_float), ("slope", C.c_float),
                ("w_prep_dev", C.c_void_p), ("w_msg_dev", C.c_void_p), ("w_upd_dev", C.c_void_p), ("w_dag_dev", C.c_void_p),
                ("w_glob_dev", C.c_void_p), ("w_stage_dev", C.c_void_p), ("w_exec_dev", C.c_void_p), ("node_scratch_dev", C.c_void_p),
                ("job_scratch_dev", C.c_void_p), ("rng_seed", C.c_uint64), ("rng_counter", C.c_uint64), ("stage_idx_dev", C.c_void_p),
                ("num_exec_dev", C.c_void_p), ("stage_sel_dev", C.c_void_p), ("job_idx_dev", C.c_void_p), ("exec_sel_dev", C.c_void_p),
                ("lgprob_dev", C.c_void_p), ("stage_scores_dev", C.c_void_p), ("exec_scores_dev", C.c_void_p), ("prof_dev", C.c_void_p)]


class SssDecimaSampleArgs(C.Structure):
    _fields_ = [("n_pad", C.c_int64), ("num_executors", C.c_int), ("rng_seed", C.c_uint64), ("rng_counter", C.c_uint64),
                ("stage_scores_dev", C.c_void_p), ("exec_scores_dev", C.c_void_p), ("obs_nodes_dev", C.c_void_p),
                ("obs_node_off_dev", C.c_void_p), ("obs_job_off_dev", C.c_void_p), ("sched_rank_dev", C.c_void_p),
                ("node_job_dev", C.c_void_p), ("job_gid_dev", C.c_void_p), ("stage_idx_dev", C.c_void_p), ("num_exec_dev", C.c_void_p),
                ("stage_sel_dev", C.c_void_p), ("job_idx_dev", C.c_void_p), ("exec_sel_dev", C.c_void_p), ("lgprob_dev", C.c_void_p),
                ("any_stage_dev", C.c_void_p)]


class SssGnnArgs(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("w_dev", C.c_void_p), ("w2_dev", C.c_void_p), ("slope", C.c_float), ("num_executors", C.c_int),
                ("layer", C.c_int), ("n_pad", C.c_int64), ("x_dev", C.c_void_p), ("h_init_dev", C.c_void_p), ("h_dev", C.c_void_p),
                ("tmp_dev", C.c_void_p), ("h_dag_dev", C.c_void_p), ("h_glob_dev", C.c_void_p), ("out_dev", C.c_void_p),
                ("out_deg_dev", C.c_void_p), ("obs_depth_dev", C.c_void_p), ("idx0_dev", C.c_void_p), ("dst_dev", C.c_void_p),
                ("out_start_dev", C.c_void_p), ("edge_layers_dev", C.c_void_p), ("node_job_dev", C.c_void_p), ("node_obs_dev", C.c_void_p),
                ("node_loc_dev", C.c_void_p), ("job_obs_dev", C.c_void_p), ("job_first_dev", C.c_void_p), ("job_cap_dev", C.c_void_p),
                ("job_nodes_dev", C.c_void_p), ("obs_job_off_dev", C.c_void_p), ("obs_jobs_dev", C.c_void_p),
                ("w16_dev", C.c_void_p), ("w2_16_dev", C.c_void_p), ("node_recv_dev", C.c_void_p), ("n_rows_dev", C.c_void_p)]


GNN_KINDS = {"prep": 0, "sink": 1, "layer": 2, "commit": 3, "dagsum": 4, "globsum": 5, "stage": 6, "exec": 7, "daghid": 8, "globhid": 9, "merge": 10}

ERROR_NAMES = {
    1: "invalid action: does not belong to the action space",
    2: "invalid action: stage_idx is not a schedulable stage",
    4: "invalid action: too many executors requested",
    5: "[step]: simulation stalled with no committable executors or schedulable stages",
    6: "no task-duration data for the sampled executor level",
    7: "internal invariant violated",
    8: "episode is over or failed: reset() required",
    9: "must either have a limit on job arrivals or time.",
    10: "more job arrivals than max_jobs",
}

class SssGnnEncodeArgs(C.Structure):  # include/sss.h sss_gnn_encode_args
    _fields_ = ([("n_nodes", C.c_int64), ("n_jobs", C.c_int64), ("n_obs", C.c_int32), ("max_depth", C.c_int32), ("slope", C.c_float), ("layers_mode", C.c_int32)]
                + [(k + "_dev", C.c_void_p) for k in ("w_prep", "w_update", "w_msg", "w_dag", "w_glob", "w_msg16", "w_update16", "x", "out_deg", "obs_depth", "node_obs", "dst",
                                                      "out_start", "edge_layers", "node_recv", "job_first", "job_nodes", "obs_job_off", "obs_jobs", "obs_node_off",
                                                      "obs_nodes", "layer_cnt", "h_init", "h", "tmp", "h_dag", "h_glob", "env_off", "layer_totals", "recv")]
                + [("recv_cap", C.c_int64), ("recv_stride", C.c_int64), ("layer_rows_hint", C.c_int64 * 32),
                   ("n_nodes_dev", C.c_void_p), ("n_jobs_dev", C.c_void_p), ("n_nodes_hint", C.c_int64), ("n_jobs_hint", C.c_int64), ("max_obs_nodes_hint", C.c_int64)])


class SssCollectArgs(C.Structure):  # include/sss.h sss_collect_args
    _fields_ = [("num_envs", C.c_int32), ("asynchronous", C.c_int32), ("t", C.c_int64), ("duration", C.c_double), ("obs_f64_dev", C.c_void_p), ("obs_i32_dev", C.c_void_p),
                ("obs_i32_stride", C.c_int64), ("time_limit_dev", C.c_void_p), ("active_dev", C.c_void_p), ("wall_dev", C.c_void_p), ("elapsed_dev", C.c_void_p),
                ("step_counts_dev", C.c_void_p), ("pending_reset_dev", C.c_void_p), ("stage_sel_dev", C.c_void_p), ("job_idx_dev", C.c_void_p), ("exec_sel_dev", C.c_void_p),
                ("lgprob_dev", C.c_void_p), ("stage_idx_dev", C.c_void_p), ("num_exec_dev", C.c_void_p), ("rec_active_dev", C.c_void_p), ("rec_t_before_dev", C.c_void_p),
                ("rec_t_after_dev", C.c_void_p), ("rec_rewards_dev", C.c_void_p), ("rec_stage_sel_dev", C.c_void_p), ("rec_job_idx_dev", C.c_void_p),
                ("rec_exec_sel_dev", C.c_void_p), ("rec_lgprobs_dev", C.c_void_p), ("rec_resets_dev", C.c_void_p), ("flags_dev", C.c_void_p)]


class SssMlpArgs(C.Structure):  # include/sss.h sss_mlp_args
    _fields_ = [("rows", C.c_int64), ("in_dim", C.c_int32), ("h1", C.c_int32), ("h2", C.c_int32), ("out_dim", C.c_int32), ("act", C.c_int32), ("slope", C.c_float),
                ("w_dev", C.c_void_p), ("x_dev", C.c_void_p), ("a1_dev", C.c_void_p), ("a2_dev", C.c_void_p), ("y_dev", C.c_void_p), ("dy_dev", C.c_void_p),
                ("g1_dev", C.c_void_p), ("g2_dev", C.c_void_p), ("dx_dev", C.c_void_p), ("x2_dev", C.c_void_p), ("dx2_dev", C.c_void_p)]


class SssRowsArgs(C.Structure):  # include/sss.h sss_rows_args
    _fields_ = [("n", C.c_int64), ("ld_a", C.c_int64), ("width", C.c_int32), ("op", C.c_int32), ("idx_dev", C.c_void_p), ("a_dev", C.c_void_p), ("b_dev", C.c_void_p),
                ("c_dev", C.c_void_p), ("perm_dev", C.c_void_p)]


class SssConcatPart(C.Structure):  # include/sss.h sss_concat_part
    _fields_ = [("table_dev", C.c_void_p), ("idx_dev", C.c_void_p), ("width", C.c_int32), ("pad_", C.c_int32)]


class SssConcatArgs(C.Structure):  # include/sss.h sss_concat_args
    _fields_ = [("n", C.c_int64), ("n_parts", C.c_int32), ("op", C.c_int32), ("out_dev", C.c_void_p), ("parts", SssConcatPart * 4)]


class SssSegcatArgs(C.Structure):  # include/sss.h sss_segcat_args
    _fields_ = [("n_seg", C.c_int64), ("scores_dev", C.c_void_p), ("ptr_dev", C.c_void_p), ("chosen_dev", C.c_void_p), ("den_eps", C.c_float), ("pad_", C.c_int32),
                ("lg_dev", C.c_void_p), ("ent_dev", C.c_void_p), ("g_lg_dev", C.c_void_p), ("g_ent_dev", C.c_void_p), ("g_scores_dev", C.c_void_p)]


class SssBitListArgs(C.Structure):  # include/sss.h sss_bit_list_args
    _fields_ = [("bits_dev", C.c_void_p), ("n", C.c_int64), ("n_layers", C.c_int32), ("chunk", C.c_int32), ("n_chunks", C.c_int32), ("phase", C.c_int32),
                ("cnt_dev", C.c_void_p), ("off_dev", C.c_void_p), ("base", C.c_int64 * 32), ("out_dev", C.c_void_p)]


class SssReturnsArgs(C.Structure):  # include/sss.h sss_returns_args
    _fields_ = [("T", C.c_int64), ("B", C.c_int64), ("active_dev", C.c_void_p), ("t_before_dev", C.c_void_p), ("t_after_dev", C.c_void_p), ("rewards_dev", C.c_void_p),
                ("beta", C.c_double), ("out_dev", C.c_void_p)]


class SssBaselineArgs(C.Structure):  # include/sss.h sss_baseline_args
    _fields_ = [("T", C.c_int64), ("B", C.c_int64), ("R", C.c_int32), ("skip_empty", C.c_int32), ("active_dev", C.c_void_p), ("times_dev", C.c_void_p),
                ("values_dev", C.c_void_p), ("n_dev", C.c_void_p), ("out_dev", C.c_void_p)]


class SssRewardWindowArgs(C.Structure):  # include/sss.h sss_reward_window_args
    _fields_ = [("T", C.c_int64), ("B", C.c_int64), ("active_dev", C.c_void_p), ("t_before_dev", C.c_void_p), ("t_after_dev", C.c_void_p), ("rewards_dev", C.c_void_p),
                ("cap", C.c_int64), ("window_dev", C.c_void_p * 2), ("current", C.c_int32), ("pad_", C.c_int32), ("scratch_dev", C.c_void_p), ("sums_dev", C.c_void_p)]


class SssDiffretArgs(C.Structure):  # include/sss.h sss_diffret_args
    _fields_ = [("T", C.c_int64), ("B", C.c_int64), ("active_dev", C.c_void_p), ("t_before_dev", C.c_void_p), ("t_after_dev", C.c_void_p), ("rewards_dev", C.c_void_p),
                ("sums_dev", C.c_void_p), ("out_dev", C.c_void_p), ("avg_dev", C.c_void_p)]


class SssTimeline(C.Structure):  # include/sss.h sss_timeline
    _fields_ = [("t_dev", C.c_void_p), ("job_dev", C.c_void_p), ("count_dev", C.c_void_p), ("cap", C.c_int32), ("pad_", C.c_int32)]


class SssTimelineRenderArgs(C.Structure):  # include/sss.h sss_timeline_render_args
    _fields_ = [("env_ids_dev", C.c_void_p), ("n", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("pad_", C.c_int32), ("rgb_dev", C.c_void_p)]


class SssEnvStore(C.Structure):  # include/sss.h sss_env_store
    _fields_ = [("state_dev", C.c_void_p), ("nodes_dev", C.c_void_p), ("edge_links_dev", C.c_void_p), ("dag_ptr_dev", C.c_void_p),
                ("exec_supplies_dev", C.c_void_p), ("obs_i32_dev", C.c_void_p), ("obs_f64_dev", C.c_void_p), ("tl_t_dev", C.c_void_p),
                ("tl_job_dev", C.c_void_p), ("tl_count_dev", C.c_void_p), ("tl_cap", C.c_int32), ("num_slots", C.c_int32), ("layout_id", C.c_uint64)]


class SssEnvCopyArgs(C.Structure):  # include/sss.h sss_env_copy_args
    _fields_ = [("src_store", C.POINTER(SssEnvStore)), ("dst_store", C.POINTER(SssEnvStore)), ("src_ids_dev", C.c_void_p), ("dst_ids_dev", C.c_void_p),
                ("reseed_dev", C.c_void_p), ("n", C.c_int32), ("pad_", C.c_int32)]


JOB_STATS_COLUMNS = ("num_jobs", "total_job_time", "avg_job_duration", "avg_num_jobs", "avg_completed_job_duration", "num_completed_jobs", "num_active_jobs",
                     "wall_time")  # include/sss.h sss_job_stats: stats[0..7]
JOB_STATS_MAX_Q = 16

REWARD_WINDOW_CHUNK = 64  # include/sss.h SSS_REWARD_WINDOW_CHUNK


def reward_window_scratch(T: int, B: int) -> int:
    """include/sss.h SSS_REWARD_WINDOW_SCRATCH(T, B): int64 elements of workspace of sss_reward_window_update"""
    return ((T + REWARD_WINDOW_CHUNK - 1) // REWARD_WINDOW_CHUNK + 1) * B + 1


class SssArenaArray(C.Structure):  # include/sss.h sss_arena_array
    _fields_ = [("src_dev", C.c_void_p), ("dst_dev", C.c_void_p), ("elem_bytes", C.c_int32), ("per_row", C.c_int32), ("kind", C.c_int32), ("shift", C.c_int32)]


class SssArenaArgs(C.Structure):  # include/sss.h sss_arena_args
    _fields_ = [("n_arrays", C.c_int32), ("n_obs", C.c_int32), ("totals_dev", C.c_void_p), ("cursor_dev", C.c_void_p), ("capacity", C.c_int64 * 4),
                ("rows_hint", C.c_int64), ("arrays", SssArenaArray * 24)]


EXPORTS = ["sss_query_dims", "sss_create", "sss_bind_buffers", "sss_reset", "sss_step", "sss_step_bounded", "sss_policy", "sss_rollout",
           "sss_decima_graph_build", "sss_decima_layer_lists", "sss_prefix_rows", "sss_decima_policy", "sss_decima_sample", "sss_gnn_launch",
           "sss_linear_wgrad_scratch", "sss_linear_wgrad", "sss_mlp_supported", "sss_mlp_recompute_supported", "sss_mlp_split_supported", "sss_mlp_forward", "sss_mlp_backward", "sss_mlp_wgrad_scratch", "sss_mlp_backward_wgrad", "sss_mlp_wgrad_finish", "sss_collect_step", "sss_gnn_encode", "sss_rows_op", "sss_rows_concat", "sss_segment_categorical", "sss_bit_lists", "sss_arena_append", "sss_discounted_returns", "sss_sequence_baselines", "sss_reward_window_update", "sss_differential_returns", "sss_bind_timeline", "sss_timeline_render", "sss_decima_argmax", "sss_decima_policy_argmax", "sss_job_stats", "sss_env_layout_id", "sss_env_copy", "sss_rollout_each", "sss_lookahead_pick", "sss_rollout_until", "sss_lookahead_pick_horizon", "sss_rollout_decima", "sss_decima_topk", "sss_rollout_action", "sss_last_error", "sss_destroy", "sss_abi_sizeof"]
POLICY_IDS = {"fair": 0, "fifo": 1, "hash": 2, "wfair": 3, "sjfcp": 4}
POLICY_DECIMA = 5  # sss_rollout_decima only: the learned policy in a per-env policy array (not in POLICY_IDS: sss_policy / sss_rollout / sss_rollout_each refuse it)
WFAIR_ALPHA_RANGE = (-4, 4)  # sss_policy / sss_rollout: the weighted-fair exponent (param of policy 3)
LOOKAHEAD_TAILS = {"none": 0, "srpt": 1}  # sss_lookahead_pick_horizon: what a child that stopped at its horizon is charged for the rest
# the argument structures of include/sss.h and their mirrors here (Binding.check_abi)
ABI_STRUCTS = {"sss_cfg": SssCfg, "sss_dims": SssDims, "sss_buffers": SssBuffers, "sss_decima_graph": SssDecimaGraph, "sss_decima_lists": SssDecimaLists,
               "sss_bit_list_args": SssBitListArgs, "sss_gnn_args": SssGnnArgs, "sss_decima_policy_args": SssDecimaPolicyArgs,
               "sss_decima_sample_args": SssDecimaSampleArgs, "sss_gnn_encode_args": SssGnnEncodeArgs, "sss_collect_args": SssCollectArgs,
               "sss_mlp_args": SssMlpArgs, "sss_arena_array": SssArenaArray, "sss_arena_args": SssArenaArgs, "sss_returns_args": SssReturnsArgs,
               "sss_baseline_args": SssBaselineArgs, "sss_rows_args": SssRowsArgs, "sss_concat_part": SssConcatPart, "sss_concat_args": SssConcatArgs, "sss_segcat_args": SssSegcatArgs}
# ... and the ones the header declares as `struct name { .. }; typedef struct name name;` (tests/test_abi.py pins the list of the
# `} name;` typedefs above against a list of its own): checked at load in the same way
ABI_TAGGED_STRUCTS = {"sss_reward_window_args": SssRewardWindowArgs, "sss_diffret_args": SssDiffretArgs}
# ... and the ones it declares as `struct name { .. };` alone, without a typedef (tests pin both lists above against lists of their own)
ABI_PLAIN_STRUCTS = {"sss_timeline": SssTimeline, "sss_timeline_render_args": SssTimelineRenderArgs}
# ... and the two of sss_env_copy (declared `struct name`, the brace on the next line; tests/fork_util.py pins this list and their fields)
ABI_STORE_STRUCTS = {"sss_env_store": SssEnvStore, "sss_env_copy_args": SssEnvCopyArgs}


def load_library(path: str | None = None) -> C.CDLL:
    path = path or osp.join(CSRC, LIB_NAME)
    if not osp.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or spark_sched_sim_amd/build.py). "
            "There is no CPU fallback.")
    return C.CDLL(path)


class Binding:
    def __init__(self, lib: C.CDLL | None = None):
        self.lib = lib if lib is not None else load_library()
        L = self.lib
        L.sss_query_dims.argtypes = [C.POINTER(SssCfg), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(SssDims)]
        L.sss_create.argtypes = [C.POINTER(SssCfg), C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.sss_bind_buffers.argtypes = [C.c_void_p, C.POINTER(SssBuffers)]
        L.sss_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sss_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
        L.sss_step_bounded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        L.sss_policy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sss_rollout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
        L.sss_decima_graph_build.argtypes = [C.c_void_p, C.POINTER(SssDecimaGraph), C.c_void_p]
        L.sss_decima_layer_lists.argtypes = [C.c_int, C.POINTER(SssDecimaLists), C.c_void_p]
        L.sss_prefix_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sss_decima_policy.argtypes = [C.c_void_p, C.POINTER(SssDecimaPolicyArgs), C.c_void_p]
        L.sss_decima_sample.argtypes = [C.c_int, C.c_int, C.POINTER(SssDecimaSampleArgs), C.c_void_p]
        L.sss_gnn_launch.argtypes = [C.c_int, C.POINTER(SssGnnArgs), C.c_void_p]
        L.sss_linear_wgrad_scratch.argtypes = [C.c_int, C.c_int]
        L.sss_linear_wgrad_scratch.restype = C.c_int64
        L.sss_linear_wgrad.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sss_gnn_encode.argtypes = [C.POINTER(SssGnnEncodeArgs), C.c_void_p]
        L.sss_collect_step.argtypes = [C.POINTER(SssCollectArgs), C.c_int, C.c_void_p]
        L.sss_mlp_supported.argtypes = [C.c_int] * 5
        L.sss_mlp_recompute_supported.argtypes = [C.c_int]
        L.sss_mlp_split_supported.argtypes = [C.c_int]
        L.sss_mlp_forward.argtypes = [C.POINTER(SssMlpArgs), C.c_void_p]
        L.sss_mlp_backward.argtypes = [C.POINTER(SssMlpArgs), C.c_void_p]
        L.sss_mlp_wgrad_scratch.argtypes = [C.c_int]
        L.sss_mlp_wgrad_scratch.restype = C.c_int64
        L.sss_mlp_backward_wgrad.argtypes = [C.POINTER(SssMlpArgs), C.c_void_p, C.c_void_p]
        L.sss_mlp_wgrad_finish.argtypes = [C.c_int] + [C.c_void_p] * 8
        L.sss_discounted_returns.argtypes = [C.POINTER(SssReturnsArgs), C.c_void_p]
        L.sss_sequence_baselines.argtypes = [C.POINTER(SssBaselineArgs), C.c_void_p]
        L.sss_reward_window_update.argtypes = [C.POINTER(SssRewardWindowArgs), C.c_void_p]
        L.sss_differential_returns.argtypes = [C.POINTER(SssDiffretArgs), C.c_void_p]
        L.sss_bind_timeline.argtypes = [C.c_void_p, C.POINTER(SssTimeline)]
        L.sss_timeline_render.argtypes = [C.c_void_p, C.POINTER(SssTimelineRenderArgs), C.c_void_p]
        L.sss_decima_argmax.argtypes = [C.c_int, C.c_int, C.POINTER(SssDecimaSampleArgs), C.c_void_p]
        L.sss_decima_policy_argmax.argtypes = [C.c_void_p, C.POINTER(SssDecimaPolicyArgs), C.c_void_p]
        L.sss_job_stats.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        L.sss_env_layout_id.argtypes = [C.c_void_p]
        L.sss_env_layout_id.restype = C.c_uint64
        L.sss_env_copy.argtypes = [C.c_void_p, C.POINTER(SssEnvCopyArgs), C.c_void_p]
        L.sss_rollout_each.argtypes = [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4
        L.sss_lookahead_pick.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 13
        L.sss_rollout_until.argtypes = [C.c_void_p] * 5 + [C.c_double, C.c_int] + [C.c_void_p] * 6
        L.sss_rollout_decima.argtypes = [C.c_void_p, C.POINTER(SssDecimaPolicyArgs), C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4
        L.sss_decima_topk.argtypes = [C.c_void_p, C.POINTER(SssDecimaPolicyArgs), C.c_int] + [C.c_void_p] * 6
        L.sss_rollout_action.argtypes = [C.c_void_p, C.POINTER(SssDecimaPolicyArgs), C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4
        L.sss_lookahead_pick_horizon.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 7
        L.sss_bit_lists.argtypes = [C.POINTER(SssBitListArgs), C.c_void_p]
        L.sss_arena_append.argtypes = [C.POINTER(SssArenaArgs), C.c_void_p]
        L.sss_rows_op.argtypes = [C.POINTER(SssRowsArgs), C.c_void_p]
        L.sss_rows_concat.argtypes = [C.POINTER(SssConcatArgs), C.c_void_p]
        L.sss_segment_categorical.argtypes = [C.POINTER(SssSegcatArgs), C.c_int, C.c_void_p]
        L.sss_last_error.restype = C.c_char_p
        L.sss_destroy.argtypes = [C.c_void_p]
        L.sss_abi_sizeof.argtypes = [C.c_char_p]
        self.check_abi()

    def check_abi(self) -> None:
        """every ctypes mirror above has the size the library was compiled with (include/sss.h sss_abi_sizeof): a binding and a
        library of different rounds fail here, not inside a kernel"""
        bad = [(name, C.sizeof(cls), self.lib.sss_abi_sizeof(name.encode())) for name, cls in {**ABI_STRUCTS, **ABI_TAGGED_STRUCTS, **ABI_PLAIN_STRUCTS, **ABI_STORE_STRUCTS}.items()
               if C.sizeof(cls) != self.lib.sss_abi_sizeof(name.encode())]
        if bad:
            raise RuntimeError("binding / library mismatch (struct, sizeof in binding.py, sizeof in the library): " + ", ".join(map(str, bad)))

    def check(self, rc: int) -> None:
        if rc != 0:
            raise ValueError(f"sss error {rc}: {self.lib.sss_last_error().decode()}")

    def query_dims(self, cfg: SssCfg, pack: bytes, num_envs: int) -> SssDims:
        d = SssDims()
        self.check(self.lib.sss_query_dims(C.byref(cfg), pack, len(pack), num_envs, C.byref(d)))
        return d

    def create(self, cfg: SssCfg, pack: bytes, num_envs: int, device: int) -> C.c_void_p:
        h = C.c_void_p()
        self.check(self.lib.sss_create(C.byref(cfg), pack, len(pack), num_envs, device, C.byref(h)))
        return h


def device_of(dev):
    """context manager: `dev` is the current device while inside (no-op for CPU tensors, i.e. the emulator
    tests). The entry points of include/sss.h that take no env handle (sss_prefix_rows, sss_gnn_launch,
    sss_decima_sample, sss_decima_layer_lists) launch on the CURRENT device's stream; their callers make
    the device of the tensors they pass current, so that a caller whose own current device is another GPU
    (several envs / policies in one process) still works."""
    import contextlib

    import torch
    dev = torch.device(dev)
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()
