"""ctypes binding of libspp_hip.so (the C ABI declared in include/spp.h).

There is no CPU fallback: if the library is missing or no HIP device is usable, the
product path raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libspp_hip.so")

SPP_MAX_HOPS = 8
SPP_MAX_PARTS = 64

p = C.c_void_p
i32 = C.c_int32
i64 = C.c_int64
u32 = C.c_uint32


class PartitionCfg(C.Structure):
    _fields_ = [("num_parts", i32), ("rank", i32), ("offsets", i64 * (SPP_MAX_PARTS + 1)),
                ("use_cache", i32), ("cache_map_dev", p), ("cache_map_len", i64)]


class SamplerOpts(C.Structure):
    """spp_sampler_opts: 0 = automatic, > 0 on, < 0 off (include/spp.h)."""
    _fields_ = [("col32", i32), ("deg_tags", i32), ("row_stubs", i32), ("rng_arena", i32), ("rng_arena_mb", i64),
                ("fuse_scatter", i32), ("flag_tiled", i32), ("rows_coalesced", i32), ("dedup_preread", i32),
                ("fuse_max_edges", i64), ("initial_edge_cap", i64), ("reserved", i64 * 4)]


class SamplerCfg(C.Structure):
    _fields_ = [("rowptr_dev", p), ("col_dev", p), ("num_nodes", i64), ("nnz", i64),
                ("num_hops", i32), ("sizes", i64 * SPP_MAX_HOPS), ("max_batch", i64),
                ("num_slots", i32), ("device", i32), ("replace", i32), ("part", PartitionCfg),
                ("graph_generation", i64), ("opts", SamplerOpts)]


class SamplerInfo(C.Structure):
    _fields_ = [("col32", i32), ("deg_tags", i32), ("row_stubs", i32), ("rng_arena", i32), ("idbits", i32),
                ("tag_cap", i32), ("num_hops", i32), ("dedup_buckets_log2", i32), ("dedup_table_slots", i32),
                ("generic", i32 * SPP_MAX_HOPS), ("fused_pick", i32 * SPP_MAX_HOPS), ("flag_tiled", i32 * SPP_MAX_HOPS),
                ("rows_coalesced", i32 * SPP_MAX_HOPS), ("bucket_log2", i32 * SPP_MAX_HOPS),
                ("col32_ms", C.c_double), ("row_stubs_ms", C.c_double), ("rng_arena_ms", C.c_double),
                ("col32_bytes", i64), ("row_stubs_bytes", i64), ("rng_arena_bytes", i64), ("rng_arena_batches", i64)]


class MfgCounts(C.Structure):
    _fields_ = [("num_nodes", i64), ("num_seeds", i64), ("num_hops", i32),
                ("T", i64 * SPP_MAX_HOPS), ("S", i64 * SPP_MAX_HOPS), ("E", i64 * SPP_MAX_HOPS),
                ("draws", i64), ("part_counts", i64 * (SPP_MAX_PARTS + 2))]


class MfgOut(C.Structure):
    _fields_ = [("n_id", p), ("rowptr", p * SPP_MAX_HOPS), ("col", p * SPP_MAX_HOPS),
                ("parts", p), ("cached", p), ("perm", p), ("row_addr", p), ("x_remote", p)]


# spp_elem and the aggregation descriptor's codes (include/spp.h)
SPP_ELEM_F32, SPP_ELEM_F16, SPP_ELEM_BF16 = 0, 1, 2
SPP_BN_ACT_NONE, SPP_BN_ACT_RELU, SPP_BN_ACT_LEAKY_RELU = 0, 1, 2
SPP_ELEM_FP8_E4M3 = 3            # spp_agg_forward_fp8, spp_graph_agg_*_forward_fp8, spp_exchange_cfg.x_elem
SPP_AGG_DENSE, SPP_AGG_TABLE, SPP_AGG_ROWS = 0, 1, 2
SPP_AGG_MEAN, SPP_AGG_OPERAND, SPP_AGG_OPERAND_ACT, SPP_AGG_SUM = 0, 1, 2, 3
SPP_AGG_SCATTER, SPP_AGG_GATHER = 0, 1
SPP_AGG_MAX, SPP_AGG_MAX_OPERAND = 4, 5   # spp_graph_agg_forward / _fp8 only (spp_agg_max_forward has its own descriptor)


class AggFwdDesc(C.Structure):
    _fields_ = [("source", i32), ("epilogue", i32), ("x_elem", i32), ("out_elem", i32), ("rowptr_dev", p),
                ("col_dev", p), ("num_targets", i64), ("x_dev", p), ("x_stride_elems", i64), ("x_rows", i64),
                ("n_id_dev", p), ("F", i64), ("out_dev", p), ("out_stride_elems", i64), ("self_scale", C.c_float),
                ("p", C.c_float), ("training", i32), ("reserved", i32), ("seed", C.c_uint64)]


class AggBwdDesc(C.Structure):
    _fields_ = [("form", i32), ("epilogue", i32), ("grad_elem", i32), ("out_elem", i32), ("z_elem", i32),
                ("reserved", i32), ("rowptr_dev", p), ("col_dev", p), ("num_targets", i64), ("num_sources", i64),
                ("num_edges", i64), ("grad_out_dev", p), ("grad_out_stride_elems", i64), ("F", i64),
                ("grad_x_dev", p), ("z_dev", p), ("self_scale", C.c_float), ("p", C.c_float), ("training", i32),
                ("reserved2", i32), ("seed", C.c_uint64)]


class AggMaxFwdDesc(C.Structure):
    """spp_agg_max_fwd_desc: out = max over the row (first occurrence in arg), optionally [max | x_target]"""
    _fields_ = [("source", i32), ("x_elem", i32), ("out_elem", i32), ("concat_target", i32), ("rowptr_dev", p),
                ("col_dev", p), ("num_targets", i64), ("x_dev", p), ("x_stride_elems", i64), ("x_rows", i64),
                ("n_id_dev", p), ("scale_log2_dev", p), ("F", i64), ("out_dev", p), ("out_stride_elems", i64),
                ("arg_dev", p)]


class AggMaxBwdDesc(C.Structure):
    """spp_agg_max_bwd_desc: grad_x[arg[t, c], c] += g[t, c] (+ the target half with concat_target)"""
    _fields_ = [("grad_elem", i32), ("out_elem", i32), ("concat_target", i32), ("reserved", i32), ("arg_dev", p),
                ("num_targets", i64), ("num_sources", i64), ("grad_out_dev", p), ("grad_out_stride_elems", i64),
                ("F", i64), ("grad_x_dev", p), ("workspace_dev", p), ("workspace_bytes", i64)]


class AggWeightedFwdDesc(C.Structure):
    """spp_agg_weighted_fwd_desc: out[t] = sum_k w[k] * x[col[k]] (+ self_w[t] * x[t], last), one fmaf per entry"""
    _fields_ = [("source", i32), ("x_elem", i32), ("out_elem", i32), ("reserved", i32), ("rowptr_dev", p),
                ("col_dev", p), ("num_targets", i64), ("num_edges", i64), ("x_dev", p), ("x_stride_elems", i64),
                ("x_rows", i64), ("n_id_dev", p), ("F", i64), ("w_dev", p), ("self_w_dev", p), ("out_dev", p),
                ("out_stride_elems", i64)]


class AggWeightedBwdDesc(C.Structure):
    """spp_agg_weighted_bwd_desc: grad_x[s] = sum_{k = (t, s)} w[k] * g[t] (+ self_w[s] * g[s]), a gather"""
    _fields_ = [("grad_elem", i32), ("out_elem", i32), ("rowptr_dev", p), ("col_dev", p), ("num_targets", i64),
                ("num_sources", i64), ("num_edges", i64), ("grad_out_dev", p), ("grad_out_stride_elems", i64), ("F", i64),
                ("w_dev", p), ("self_w_dev", p), ("grad_x_dev", p)]


class AggWeightedWgradDesc(C.Structure):
    """spp_agg_weighted_wgrad_desc: grad_w[k] = <g[t], x[col[k]]>, grad_self_w[t] = <g[t], x[t]>"""
    _fields_ = [("source", i32), ("x_elem", i32), ("grad_elem", i32), ("reserved", i32), ("rowptr_dev", p),
                ("col_dev", p), ("num_targets", i64), ("num_edges", i64), ("x_dev", p), ("x_stride_elems", i64),
                ("x_rows", i64), ("n_id_dev", p), ("F", i64), ("grad_out_dev", p), ("grad_out_stride_elems", i64),
                ("grad_w_dev", p), ("grad_self_w_dev", p)]


class GcnNormDesc(C.Structure):
    """spp_gcn_norm_desc: PyG's gcn_norm of a hop padded to [S, S]"""
    _fields_ = [("fill", i32), ("reserved", i32), ("rowptr_dev", p), ("col_dev", p), ("num_targets", i64),
                ("num_sources", i64), ("num_edges", i64), ("w_dev", p), ("dinv_dev", p), ("coef_dev", p),
                ("self_coef_dev", p)]


class Gatv2Desc(C.Structure):
    """spp_gatv2_desc: GATv2Conv over a hop on projected rows x_l [S, H*C], x_r [T, H*C]; forward and backward"""
    _fields_ = [("heads", i32), ("x_elem", i32), ("negative_slope", C.c_float), ("reserved", i32), ("rowptr_dev", p),
                ("col_dev", p), ("num_targets", i64), ("num_sources", i64), ("C", i64), ("x_l_dev", p),
                ("x_l_stride_elems", i64), ("x_r_dev", p), ("x_r_stride_elems", i64), ("att_dev", p), ("out_dev", p),
                ("row_max_dev", p), ("row_sum_dev", p), ("grad_out_dev", p), ("grad_x_l_dev", p), ("grad_x_r_dev", p),
                ("grad_att_dev", p)]


class TransformerDesc(C.Structure):
    """spp_transformer_desc: TransformerConv over a hop on projected rows q [T, H*C], k and v [S, H*C]; forward and
    backward"""
    _fields_ = [("heads", i32), ("x_elem", i32), ("scale", C.c_float), ("reserved", i32), ("rowptr_dev", p),
                ("col_dev", p), ("num_targets", i64), ("num_sources", i64), ("C", i64), ("q_dev", p),
                ("q_stride_elems", i64), ("k_dev", p), ("k_stride_elems", i64), ("v_dev", p), ("v_stride_elems", i64),
                ("out_dev", p), ("row_max_dev", p), ("row_sum_dev", p), ("grad_out_dev", p), ("grad_q_dev", p),
                ("grad_k_dev", p), ("grad_v_dev", p)]


class GcnDinvDesc(C.Structure):
    """spp_gcn_dinv_desc: gcn_norm's first pass alone, dinv [num_nodes] over a whole graph"""
    _fields_ = [("fill", i32), ("reserved", i32), ("rowptr_dev", p), ("num_nodes", i64), ("w_dev", p), ("dinv_dev", p)]


class GraphAggWeightedDesc(C.Structure):
    """spp_graph_agg_weighted_desc: GraphAggDesc's graph, x, targets and output; the weights explicit (w_dev, self_w_dev)
    or formed in the kernel from dinv_dev and fill"""
    _fields_ = [("x_elem", i32), ("out_elem", i32), ("fill", i32), ("reserved", i32), ("rowptr_dev", p), ("col_dev", p),
                ("x_dev", p), ("x_stride_elems", i64), ("x_rows", i64), ("F", i64), ("target_row0", i64),
                ("target_ids_dev", p), ("num_targets", i64), ("out_dev", p), ("out_stride_elems", i64), ("w_dev", p),
                ("dinv_dev", p), ("self_w_dev", p)]


class GraphAggDesc(C.Structure):
    """spp_graph_agg_desc: targets as a slab (target_row0 >= 0) or a list (target_ids_dev, target_row0 < 0)"""
    _fields_ = [("epilogue", i32), ("x_elem", i32), ("out_elem", i32), ("reserved", i32), ("rowptr_dev", p),
                ("col_dev", p), ("x_dev", p), ("x_stride_elems", i64), ("x_rows", i64), ("F", i64),
                ("target_row0", i64), ("target_ids_dev", p), ("num_targets", i64), ("out_dev", p),
                ("out_stride_elems", i64), ("self_scale", C.c_float), ("reserved2", i32)]


SPP_GRAPH_AGG_MAX_PARTS = 16


class GraphAggPartsDesc(C.Structure):
    """spp_graph_agg_parts_desc: GraphAggDesc with x as num_parts row ranges (part_offsets, one base address each)"""
    _fields_ = [("epilogue", i32), ("x_elem", i32), ("out_elem", i32), ("num_parts", i32), ("rowptr_dev", p),
                ("col_dev", p), ("part_offsets", i64 * (SPP_GRAPH_AGG_MAX_PARTS + 1)),
                ("x_parts_dev", p * SPP_GRAPH_AGG_MAX_PARTS), ("x_stride_elems", i64), ("F", i64), ("target_row0", i64),
                ("target_ids_dev", p), ("num_targets", i64), ("out_dev", p), ("out_stride_elems", i64),
                ("self_scale", C.c_float), ("reserved", i32)]


class GraphGatDesc(C.Structure):
    """spp_graph_gat_desc: projected rows h with their logits; targets as in GraphAggDesc"""
    _fields_ = [("x_elem", i32), ("out_elem", i32), ("heads", i32), ("relu", i32), ("rowptr_dev", p), ("col_dev", p),
                ("x_dev", p), ("x_stride_elems", i64), ("x_rows", i64), ("F", i64), ("a_src_dev", p), ("a_dst_dev", p),
                ("target_row0", i64), ("target_ids_dev", p), ("num_targets", i64), ("out_dev", p),
                ("out_stride_elems", i64), ("negative_slope", C.c_float), ("reserved", i32)]


class GraphGatv2Desc(C.Structure):
    """spp_graph_gatv2_desc: projected rows x_l and x_r [x_rows, heads * C] by global id and att; targets as in
    GraphAggDesc"""
    _fields_ = [("x_elem", i32), ("out_elem", i32), ("heads", i32), ("relu", i32), ("rowptr_dev", p), ("col_dev", p),
                ("x_l_dev", p), ("x_l_stride_elems", i64), ("x_r_dev", p), ("x_r_stride_elems", i64), ("x_rows", i64),
                ("C", i64), ("att_dev", p), ("target_row0", i64), ("target_ids_dev", p), ("num_targets", i64),
                ("out_dev", p), ("out_stride_elems", i64), ("negative_slope", C.c_float), ("reserved", i32)]


class GraphTransformerDesc(C.Structure):
    """spp_graph_transformer_desc: projected rows q, k, v (and optionally skip) [x_rows, heads * C] by global id; targets
    as in GraphAggDesc"""
    _fields_ = [("x_elem", i32), ("out_elem", i32), ("heads", i32), ("relu", i32), ("rowptr_dev", p), ("col_dev", p),
                ("q_dev", p), ("q_stride_elems", i64), ("k_dev", p), ("k_stride_elems", i64), ("v_dev", p),
                ("v_stride_elems", i64), ("x_rows", i64), ("C", i64), ("target_row0", i64), ("target_ids_dev", p),
                ("num_targets", i64), ("out_dev", p), ("out_stride_elems", i64), ("skip_dev", p),
                ("skip_stride_elems", i64), ("scale", C.c_float), ("reserved", i32)]


class GraphGatPartsDesc(C.Structure):
    """spp_graph_gat_parts_desc: GraphGatDesc with h and its logits as num_parts row ranges (part_offsets, one h base and
    one [a_src | a_dst] base each)"""
    _fields_ = [("x_elem", i32), ("out_elem", i32), ("heads", i32), ("relu", i32), ("num_parts", i32), ("reserved", i32),
                ("rowptr_dev", p), ("col_dev", p), ("part_offsets", i64 * (SPP_GRAPH_AGG_MAX_PARTS + 1)),
                ("h_parts_dev", p * SPP_GRAPH_AGG_MAX_PARTS), ("a_parts_dev", p * SPP_GRAPH_AGG_MAX_PARTS),
                ("x_stride_elems", i64), ("a_stride_elems", i64), ("F", i64), ("target_row0", i64), ("target_ids_dev", p),
                ("num_targets", i64), ("out_dev", p), ("out_stride_elems", i64), ("negative_slope", C.c_float),
                ("reserved2", i32)]


class ResincEpilogueDesc(C.Structure):
    """spp_resinc_epilogue_desc: out = leaky_relu(a * z + b) + r[row]; rows of r as a slab (r_row0 >= 0) or a list"""
    _fields_ = [("z_elem", i32), ("r_elem", i32), ("out_elem", i32), ("negative_slope", C.c_float), ("z_dev", p),
                ("z_stride_elems", i64), ("a_dev", p), ("b_dev", p), ("r_dev", p), ("r_stride_elems", i64),
                ("r_rows", i64), ("r_row0", i64), ("r_ids_dev", p), ("n", i64), ("C", i64), ("out_dev", p),
                ("out_stride_elems", i64)]


class BnActDesc(C.Structure):
    """spp_bn_act_desc: y = dropout(act(BatchNorm(z))) [+ r] on batch statistics, and its backward"""
    _fields_ = [("z_elem", i32), ("r_elem", i32), ("y_elem", i32), ("g_elem", i32), ("act", i32), ("training", i32),
                ("negative_slope", C.c_float), ("p", C.c_float), ("eps", C.c_float), ("reserved", i32),
                ("momentum", C.c_double), ("seed", C.c_uint64), ("n", i64), ("C", i64), ("z_dev", p), ("gamma_dev", p),
                ("beta_dev", p), ("running_mean_dev", p), ("running_var_dev", p), ("num_batches_tracked_dev", p),
                ("r_dev", p), ("y_dev", p), ("mean_dev", p), ("invstd_dev", p), ("g_dev", p), ("dz_dev", p),
                ("dgamma_dev", p), ("dbeta_dev", p), ("workspace_dev", p), ("workspace_bytes", i64)]


class ClassifyDesc(C.Structure):
    """spp_classify_desc: pred = argmax z, nll = logsumexp(z) - z[y]; labels as a slab (y_row0 >= 0) or a list"""
    _fields_ = [("z_elem", i32), ("reserved", i32), ("z_dev", p), ("z_stride_elems", i64), ("n", i64), ("C", i64),
                ("y_dev", p), ("y_rows", i64), ("y_row0", i64), ("row_ids_dev", p), ("pred_dev", p), ("nll_dev", p)]


class FieldDesc(C.Structure):
    """spp_field_desc: the frontier (spp_field_mark) or the field's rows by slot (spp_field_rows) over the graph, with the
    slot map, the flags (mark) and the field's CSR (rows)"""
    _fields_ = [("rowptr_dev", p), ("col_dev", p), ("num_nodes", i64), ("ids_dev", p), ("num_ids", i64), ("slot_dev", p),
                ("flag_dev", p), ("frowptr_dev", p), ("fcol_dev", p), ("fcol_len", i64)]


class GroupOut(C.Structure):
    _fields_ = [("mfg", MfgOut), ("x_out", p), ("y_out", p)]


class ExchangeCfg(C.Structure):
    _fields_ = [("comm", p), ("x_local_dev", p), ("x_local_rows", i64), ("row_bytes", i64),
                ("cache_feats_dev", p), ("cache_rows", i64), ("x_local_stride_bytes", i64),
                ("cache_stride_bytes", i64), ("peer_x_dev", C.POINTER(p)), ("peer_x_stride_bytes", i64),
                ("issue_on_consumer", i32),
                # appended for fp8 partitions; all zero = rows are opaque bytes, as before
                ("x_elem", i32), ("scale_log2_dev", p), ("scales_tag", C.c_uint64)]


class SessionCfg(C.Structure):
    _fields_ = [("rowptr_dev", p), ("col_dev", p), ("num_nodes", i64), ("nnz", i64),
                ("idx_dev", p), ("n_idx", i64), ("batch_size", i64), ("num_hops", i32),
                ("sizes", i64 * SPP_MAX_HOPS), ("skip_nonfull_batch", i32),
                ("force_exact_num_batches", i32), ("exact_num_batches", i64),
                ("max_items_in_queue", i32), ("group_size", i32), ("device", i32), ("sampler", p),
                ("part", C.POINTER(PartitionCfg)), ("exchange", C.POINTER(ExchangeCfg)),
                ("input_stream", p), ("order_after_input_stream", i32)]


class BatchDesc(C.Structure):
    _fields_ = [("batch_index", i64), ("start", i32), ("stop", i32), ("slot", i32),
                ("counts", MfgCounts)]


# name -> (restype, argtypes); every symbol include/spp.h declares
SIGNATURES = {
    "spp_abi_version": (C.c_int, []),
    "spp_last_error": (C.c_char_p, []),
    "spp_device_count": (C.c_int, []),
    "spp_async_errors": (C.c_int, [C.c_int, C.c_int]),
    "spp_profile_enable": (None, [C.c_int]),
    "spp_tune": (C.c_int, [C.c_char_p, C.c_int]),
    "spp_profile_read": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64)]),
    "spp_mt19937_fill": (C.c_int, [u32, i64, i64, p, p]),
    "spp_batch_seed": (u32, [i32]),
    "spp_gather_rows": (C.c_int, [p, i64, i64, p, C.c_int, i64, i64, p, p]),
    "spp_gather_rows_strided": (C.c_int, [p, i64, i64, i64, p, C.c_int, i64, i64, p, p]),
    "spp_to_row_major": (C.c_int, [p, i64, i64, C.c_int, p, p]),
    "spp_sampler_create": (C.c_int, [C.POINTER(SamplerCfg), C.POINTER(p)]),
    "spp_sampler_destroy": (None, [p]),
    "spp_sampler_workspace_bytes": (i64, [p]),
    "spp_sampler_deliver_stream": (p, [p]),
    "spp_sampler_get_cfg": (C.c_int, [p, C.POINTER(SamplerCfg)]),
    "spp_sampler_get_info": (C.c_int, [p, C.POINTER(SamplerInfo)]),
    "spp_sampler_sample": (C.c_int, [p, i32, p, i64, u32, i64, p]),
    "spp_sampler_wait": (C.c_int, [p, i32, C.POINTER(MfgCounts)]),
    "spp_sampler_export": (C.c_int, [p, i32, C.POINTER(MfgOut), p]),
    "spp_sampler_gather": (C.c_int, [p, i32, p, i64, i64, i64, i64, p, p]),
    "spp_nid2partid": (C.c_int, [p, i32, p, i64, p, p]),
    "spp_cache_build_map": (C.c_int, [p, i64, p, i64, p]),
    "spp_cache_lookup": (C.c_int, [p, i64, p, i64, p, p, p]),
    "spp_partition_workspace_bytes": (i64, [i64]),
    "spp_partition_batch": (C.c_int, [p, i64, p, i32, i32, i32, p, i64, i64, p, p, p, p, p, p, i64, p]),
    "spp_assemble_features": (C.c_int, [p, p, i64, p, i32, i32, i64, p, i64, p, p, p, i64, i64, i64, p, p, p]),
    "spp_session_create": (C.c_int, [C.POINTER(SessionCfg), C.POINTER(p)]),
    "spp_session_destroy": (None, [p]),
    "spp_session_num_total_batches": (i64, [p]),
    "spp_session_num_consumed_batches": (i64, [p]),
    "spp_session_batch_ranges": (C.c_int, [p, p]),
    "spp_session_next": (C.c_int, [p, C.POINTER(BatchDesc)]),
    "spp_session_export": (C.c_int, [p, C.POINTER(MfgOut), p, i64, i64, i64, p, p, i64, i64, p, p]),
    "spp_session_next_group": (C.c_int, [p, i32, C.POINTER(BatchDesc), C.POINTER(i32)]),
    "spp_session_export_group": (C.c_int, [p, i32, C.POINTER(GroupOut), p, i64, i64, i64, p, i64, i64, p]),
    "spp_session_blocked_us": (i64, [p]),
    "spp_session_blocked_occasions": (i64, [p]),
    "spp_session_sampler": (p, [p]),
    "spp_session_group_size": (i32, [p]),
    "spp_comm_unique_id": (C.c_int, [p]),
    "spp_comm_create": (C.c_int, [p, i32, i32, i32, C.POINTER(p)]),
    "spp_comm_create_local": (C.c_int, [i32, i32, C.POINTER(p)]),
    "spp_comm_destroy": (None, [p]),
    "spp_comm_rank": (i32, [p]),
    "spp_comm_world": (i32, [p]),
    "spp_vip_frequencies": (C.c_int, [p, p, i64, p, i64, i64, p, i32, p, p, p]),
    "spp_csr_mean_forward": (C.c_int, [p, p, i64, p, i32, i64, i64, p, i64, p]),
    "spp_csr_mean_backward": (C.c_int, [p, p, i64, p, i64, i64, p, p]),
    "spp_sage_operand_forward": (C.c_int, [p, p, i64, p, i32, i64, i64, p, i64, p]),
    "spp_sage_operand_forward_table": (C.c_int, [p, p, i64, p, i32, i64, i64, p, i64, p, i64, p]),
    "spp_sage_operand_backward": (C.c_int, [p, p, i64, i64, p, i64, i64, p, p]),
    "spp_sage_operand_backward_workspace_bytes": (i64, [i64, i64, i64]),
    "spp_sage_operand_backward_gather": (C.c_int, [p, p, i64, i64, i64, p, i64, i64, p, p, i64, p]),
    "spp_relu_dropout_forward": (C.c_int, [p, i64, C.c_float, i32, C.c_uint64, p, p]),
    "spp_relu_dropout_backward": (C.c_int, [p, p, i64, C.c_float, p, p]),
    "spp_sage_operand_forward_act": (C.c_int, [p, p, i64, p, i64, p, i64, C.c_float, i32, C.c_uint64, p]),
    "spp_relu_dropout_backward_pre": (C.c_int, [p, p, i64, C.c_float, i32, C.c_uint64, p, p]),
    "spp_sage_operand_backward_gather_act": (C.c_int, [p, p, i64, i64, i64, p, i64, i64, p, p, i64, p, C.c_float, i32,
                                                       C.c_uint64, p]),
    "spp_gat_forward": (C.c_int, [p, p, i64, p, i64, p, p, C.c_float, p, p, p, p]),
    "spp_gat_logits": (C.c_int, [p, i32, i64, i64, i64, i64, p, p, p, p, p]),
    "spp_gat_logits_backward": (C.c_int, [p, i32, i64, i64, i64, i64, p, p, p, p, p]),
    "spp_gat_aggregate_forward": (C.c_int, [p, p, i64, p, i32, i64, i64, p, p, C.c_float, p, p, p, p]),
    "spp_gat_aggregate_backward": (C.c_int, [p, p, i64, p, i32, i64, i64, p, p, C.c_float, p, p, p, p, p, p, p, p]),
    "spp_gat_backward": (C.c_int, [p, p, i64, p, i64, p, p, C.c_float, p, p, p, p, p, p, p, p]),
    "spp_gat_aggregate_backward_gather_workspace_bytes": (i64, [i64, i64, i64]),
    "spp_gat_aggregate_backward_gather": (C.c_int, [p, p, i64, i64, i64, p, i32, i64, i64, p, p, C.c_float, p, p, p, p,
                                                    p, p, p, p, p, p, i64, p]),
    "spp_gat_mh_logits": (C.c_int, [p, i32, i64, i64, i64, i64, i32, p, p, p, p, p]),
    "spp_gat_mh_logits_backward": (C.c_int, [p, i32, i64, i64, i64, i64, i32, p, p, p, p, p]),
    "spp_gat_mh_aggregate_forward": (C.c_int, [p, p, i64, p, i32, i64, i64, i32, p, p, C.c_float, p, p, p, p]),
    "spp_gat_mh_aggregate_backward": (C.c_int, [p, p, i64, p, i32, i64, i64, i32, p, p, C.c_float, p, p, p, p, p, p,
                                                p, p]),
    "spp_gat_mh_aggregate_backward_gather_workspace_bytes": (i64, [i64, i64, i64, i32]),
    "spp_gat_mh_aggregate_backward_gather": (C.c_int, [p, p, i64, i64, i64, p, i32, i64, i64, i32, p, p, C.c_float, p,
                                                       p, p, p, p, p, p, p, p, p, i64, p]),
    # attention dropout (spp.h f3t): the three entries above + (p, training, seed), and the mask they use
    "spp_gat_mh_aggregate_forward_drop": (C.c_int, [p, p, i64, p, i32, i64, i64, i32, p, p, C.c_float, p, p, p, p,
                                                    C.c_float, i32, C.c_uint64]),
    "spp_gat_mh_aggregate_backward_drop": (C.c_int, [p, p, i64, p, i32, i64, i64, i32, p, p, C.c_float, p, p, p, p, p,
                                                     p, p, p, C.c_float, i32, C.c_uint64]),
    "spp_gat_mh_aggregate_backward_gather_drop": (C.c_int, [p, p, i64, i64, i64, p, i32, i64, i64, i32, p, p, C.c_float,
                                                            p, p, p, p, p, p, p, p, p, p, i64, p, C.c_float, i32,
                                                            C.c_uint64]),
    "spp_gat_mh_attn_keep": (C.c_int, [i64, i64, i32, C.c_float, C.c_uint64, p, p]),
    "spp_sage_operand_forward_rows": (C.c_int, [p, p, i64, p, i32, i64, p, i64, p]),
    "spp_gather_row_refs": (C.c_int, [p, i64, i64, p, p]),
    "spp_ipc_export": (C.c_int, [p, p, C.POINTER(i64)]),
    "spp_ipc_open": (C.c_int, [p, i32, C.POINTER(p)]),
    "spp_ipc_close": (C.c_int, [p]),
    "spp_csr_sum_forward": (C.c_int, [p, p, i64, p, i32, i64, i64, C.c_float, p, i64, p]),
    "spp_csr_sum_forward_table": (C.c_int, [p, p, i64, p, i32, i64, i64, p, i64, C.c_float, p, i64, p]),
    "spp_csr_sum_forward_rows": (C.c_int, [p, p, i64, p, i32, i64, C.c_float, p, i64, p]),
    "spp_csr_sum_backward": (C.c_int, [p, p, i64, i64, p, i64, i64, C.c_float, p, p]),
    "spp_csr_sum_backward_gather": (C.c_int, [p, p, i64, i64, i64, p, i64, i64, C.c_float, p, p, i64, p]),
    "spp_session_try_next": (C.c_int, [p, C.POINTER(BatchDesc)]),
    "spp_session_quiesce": (C.c_int, [p]),
    "spp_session_exchange_stats": (C.c_int, [p, C.POINTER(i64), C.POINTER(i64)]),
    "spp_agg_forward": (C.c_int, [C.POINTER(AggFwdDesc), p]),
    "spp_agg_backward": (C.c_int, [C.POINTER(AggBwdDesc), p, i64, p]),
    "spp_gather_rows_fp8": (C.c_int, [p, i64, i64, p, p, i64, p, p]),
    "spp_agg_forward_fp8": (C.c_int, [C.POINTER(AggFwdDesc), p, p]),
    "spp_graph_agg_chunk": (i64, []),
    "spp_graph_agg_workspace_bytes": (i64, [i64]),
    "spp_graph_agg_forward": (C.c_int, [C.POINTER(GraphAggDesc), p, i64, p]),
    "spp_graph_agg_parts_forward": (C.c_int, [C.POINTER(GraphAggPartsDesc), p, i64, p]),
    "spp_graph_agg_forward_fp8": (C.c_int, [C.POINTER(GraphAggDesc), p, p, i64, p]),
    "spp_graph_agg_parts_forward_fp8": (C.c_int, [C.POINTER(GraphAggPartsDesc), p, p, i64, p]),
    "spp_fp8_rows_f32": (C.c_int, [p, i64, i64, p, i64, p, i64, p, p]),
    "spp_graph_gat_chunk": (i64, []),
    "spp_graph_gat_workspace_bytes": (i64, [i64]),
    "spp_graph_gat_forward": (C.c_int, [C.POINTER(GraphGatDesc), p, i64, p]),
    "spp_graph_gat_parts_forward": (C.c_int, [C.POINTER(GraphGatPartsDesc), p, i64, p]),
    "spp_resinc_epilogue": (C.c_int, [C.POINTER(ResincEpilogueDesc), p]),
    "spp_classify_rows": (C.c_int, [C.POINTER(ClassifyDesc), p]),
    "spp_field_chunk": (i64, []),
    "spp_field_workspace_bytes": (i64, [i64]),
    "spp_field_mark": (C.c_int, [C.POINTER(FieldDesc), p, i64, p]),
    "spp_field_rows": (C.c_int, [C.POINTER(FieldDesc), p, i64, p]),
    "spp_bn_act_slab_rows": (i64, []),
    "spp_bn_act_workspace_bytes": (i64, [i64, i64]),
    "spp_bn_act_forward": (C.c_int, [C.POINTER(BnActDesc), p]),
    "spp_bn_act_backward": (C.c_int, [C.POINTER(BnActDesc), p]),
    "spp_agg_max_forward": (C.c_int, [C.POINTER(AggMaxFwdDesc), p]),
    "spp_agg_max_backward": (C.c_int, [C.POINTER(AggMaxBwdDesc), p]),
    "spp_agg_weighted_forward": (C.c_int, [C.POINTER(AggWeightedFwdDesc), p]),
    "spp_agg_weighted_backward_workspace_bytes": (i64, [i64, i64, i64]),
    "spp_agg_weighted_backward": (C.c_int, [C.POINTER(AggWeightedBwdDesc), p, i64, p]),
    "spp_agg_weighted_wgrad": (C.c_int, [C.POINTER(AggWeightedWgradDesc), p]),
    "spp_gcn_norm": (C.c_int, [C.POINTER(GcnNormDesc), p]),
    "spp_graph_agg_weighted_forward": (C.c_int, [C.POINTER(GraphAggWeightedDesc), p, i64, p]),
    "spp_gcn_dinv": (C.c_int, [C.POINTER(GcnDinvDesc), p]),
    "spp_gatv2_forward": (C.c_int, [C.POINTER(Gatv2Desc), p]),
    "spp_gatv2_backward": (C.c_int, [C.POINTER(Gatv2Desc), p]),
    "spp_graph_gatv2_chunk": (i64, []),
    "spp_graph_gatv2_workspace_bytes": (i64, [i64]),
    "spp_graph_gatv2_forward": (C.c_int, [C.POINTER(GraphGatv2Desc), p, i64, p]),
    # attention dropout (spp.h f3x): the training pair + (p, training, seed); the mask is spp_gat_mh_attn_keep's
    "spp_gatv2_forward_drop": (C.c_int, [C.POINTER(Gatv2Desc), p, C.c_float, i32, C.c_uint64]),
    "spp_gatv2_backward_drop": (C.c_int, [C.POINTER(Gatv2Desc), p, C.c_float, i32, C.c_uint64]),
    # TransformerConv over a hop (spp.h f3y)
    "spp_transformer_forward": (C.c_int, [C.POINTER(TransformerDesc), p]),
    "spp_transformer_backward": (C.c_int, [C.POINTER(TransformerDesc), p]),
    # attention dropout (spp.h f4a): the training pair + (p, training, seed); the mask is the first E * H bytes of
    # spp_gat_mh_attn_keep's
    "spp_transformer_forward_drop": (C.c_int, [C.POINTER(TransformerDesc), p, C.c_float, i32, C.c_uint64]),
    "spp_transformer_backward_drop": (C.c_int, [C.POINTER(TransformerDesc), p, C.c_float, i32, C.c_uint64]),
    # TransformerConv over rows of the resident graph (spp.h f3z)
    "spp_graph_transformer_chunk": (i64, []),
    "spp_graph_transformer_workspace_bytes": (i64, [i64]),
    "spp_graph_transformer_forward": (C.c_int, [C.POINTER(GraphTransformerDesc), p, i64, p]),
}
SPP_COMM_ID_BYTES = 128
SPP_IPC_HANDLE_BYTES = 64

_lib = None


class SppError(RuntimeError):
    pass


def load():
    """Load libspp_hip.so and type every entry point.  Raises if the extension is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SppError(
                f"{LIB_PATH} is missing: build it with `python -m salient_plusplus_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, same SONAME as the
        # system one).  It must be resident BEFORE this library is loaded so both resolve to the same
        # runtime; loading /opt/rocm's copy first leaves torch without a usable device.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.spp_abi_version() != 6:
            raise SppError("libspp_hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(rc: int):
    if rc < 0:
        msg = load().spp_last_error()
        raise SppError(msg.decode() if msg else f"libspp_hip error {rc}")
    return rc


def require_device():
    n = load().spp_device_count()
    if n <= 0:
        msg = load().spp_last_error()
        raise SppError("no usable HIP device for the MI355X data path: "
                       + (msg.decode() if msg else "device count 0"))
    return n
