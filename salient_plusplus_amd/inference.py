"""Exact, layer-wise inference over the whole graph (reference: driver/models.py:441 ``layerwise_inference`` with
``SAGE.inference``): every node is scored from ALL its neighbours, one pass per layer over the graph's CSR, with no
sampling, no dedup and no exchange.  The message passing is the HIP kernel pair of csrc/graph_aggregate.hip for SAGE,
GIN and SAGEResInception and of csrc/graph_gat.hip for GAT; SAGEResInception's layer tail is csrc/resinc_epilogue.hip
(``spp_resinc_epilogue``); GCN's weighted sums are the pair of csrc/graph_agg_weighted.hip (``graph_weighted_aggregate``,
with ``gcn_dinv`` for the per-node factors of its normalisation; resident entries only).  The layers' own parameters run
through the library GEMMs torch dispatches to.  Forward only, fp16 / fp32 / bf16 inputs.  GATv2 (f3w): the long-row
pair of csrc/graph_gatv2.hip behind ``graph_gatv2_aggregate`` (``spp_graph_gatv2_forward``) and the recipe
``_gatv2_layer`` of the attention driver; resident entries only.  GraphTransformer (f3z): the long-row pair of
csrc/graph_transformer.hip behind ``graph_transformer_aggregate`` (``spp_graph_transformer_forward``) and the recipe
``_transformer_layer`` of the same driver, with lin_skip and the ReLU in the kernel's epilogue; resident entries only.

The kernels' wrappers: ``graph_aggregate`` (``spp_graph_agg_forward``) and ``graph_gat_aggregate``
(``spp_graph_gat_forward``) read one resident matrix, ``graph_aggregate_parts`` (``spp_graph_agg_parts_forward``) and
``graph_gat_aggregate_parts`` (``spp_graph_gat_parts_forward``) a row-PARTITIONED one (one range of nodes per rank, the
peers' partitions mapped into the process), ``resinc_epilogue`` is SAGEResInception's layer tail, ``classify_rows`` (``spp_classify_rows``, csrc/classify.hip) the
tail all models share: argmax and negative log-likelihood of a tile of logits.  Each wrapper checks its arguments
with the helpers they share and hands them to its kernel's launch function (``_agg_launch``, ``_gat_launch``,
``_agg_parts_launch``, ``_gat_parts_launch``), which the drivers call directly, slab by slab.

The drivers: ``_conv_layers`` (SAGE, GIN, GCN) and ``_attn_layers`` (GAT, GATv2, GraphTransformer), each one layer loop plus a recipe per
model, and ``_resinc_layers``, written against a placement that says where the table lives -- ``_Resident`` (one matrix,
the whole-table kernels, no waits) or ``_Partitioned`` (the parts kernels over buffers published through ``peers``, a
synchronise and a barrier at every layer boundary) -- inside one frame (``_score``).  ``layerwise_inference`` is the
resident entry for all seven models (behind the ``.inference`` of the six that have one; ``gatv2_inference`` and
``transformer_inference`` are its names for one model each), ``partitioned_inference`` the partitioned one for SAGE, GIN, GAT and SAGEResInception
(``partitioned_layerwise_inference`` is its older name), with ``LocalPeers`` (ranks as threads of one process) or
``IpcPeers`` (one process per rank on one node) between the ranks.  Every driver hands its last layer's logits, tile by
tile, to a sink: ``_LogProbs`` (log_softmax into the [rows, classes] matrix those entries return) or ``_Classify``
(``classify_rows`` into pred [rows] and nll [rows]), which is what ``evaluate`` and ``partitioned_evaluate`` run: the same
pass, predictions, per-split accuracy and loss out, and no [rows, classes] matrix anywhere.

A layer loop follows a plan, one ``_Step`` a layer: which rows it computes, over which graph.  The whole-graph entries'
plan is every row of every layer but the last; ``field_inference`` and ``field_evaluate`` score a few ``nodes`` with the
same loops over a plan built from their receptive field -- the nodes within L - 1 hops, numbered and copied into a compact
CSR by ``ReceptiveFields`` (csrc/field.hip: ``spp_field_mark``, ``spp_field_rows``) -- and return the same bits."""
import ctypes as C
import threading

import torch

from . import _native as nat
from .fast_sampler import P2PPeers, RowRefs, TableRows, _common_stride, _row_stride_elems, _table_stride_bytes, \
    p2p_open_peers
from .fp8 import Fp8Features
from .models import GAT, GATv2, GCN, GIN, SAGE, GraphTransformer, SAGEResInception, _ELEM, _gcn_fill, _p, _stream

_EPILOGUES = {"mean": nat.SPP_AGG_MEAN, "operand": nat.SPP_AGG_OPERAND, "sum": nat.SPP_AGG_SUM,
              "max": nat.SPP_AGG_MAX, "max_operand": nat.SPP_AGG_MAX_OPERAND}
_MAX_EPILOGUES = ("max", "max_operand")                  # one resident matrix only: the entries over parts refuse them
_WIDE_EPILOGUES = ("operand", "max_operand")             # [T, 2F] = [reduction | x[target]]
_MAX_OVER_PARTS = ("max aggregation (aggr='max') is not built over a row-partitioned table: the parts kernels have no "
                   "max instantiation yet; score the model on one device (layerwise_inference, evaluate, field_inference)")
_OUT_DTYPES = (torch.float32, torch.bfloat16)


def graph_agg_chunk():
    """C of the summation contract (include/spp.h): rows of at most C entries are summed serially in CSR order, longer
    rows as chunks of C whose sums are added in chunk order"""
    return int(nat.load().spp_graph_agg_chunk())


def graph_agg_workspace_bytes(num_targets):
    return int(nat.load().spp_graph_agg_workspace_bytes(int(num_targets)))


def graph_gat_chunk():
    """C_g of the softmax contract (include/spp.h): a row of at most C_g raw entries is one online softmax in CSR order,
    a longer row is chunks of C_g whose softmax states are merged in chunk order"""
    return int(nat.load().spp_graph_gat_chunk())


def graph_gat_workspace_bytes(num_targets):
    return int(nat.load().spp_graph_gat_workspace_bytes(int(num_targets)))


def graph_gatv2_chunk():
    """C_g of GATv2's softmax contract (include/spp.h f3w): a row of at most C_g raw entries is one online softmax per
    head in CSR order, a longer row is chunks of C_g whose per-head states are merged in chunk order"""
    return int(nat.load().spp_graph_gatv2_chunk())


def graph_gatv2_workspace_bytes(num_targets):
    return int(nat.load().spp_graph_gatv2_workspace_bytes(int(num_targets)))


def graph_transformer_chunk():
    """C_g of TransformerConv's softmax contract (include/spp.h f3z): a row of at most C_g entries is one online softmax
    per head in CSR order from the empty state, a longer row is chunks of C_g, each from the empty state, whose per-head
    states are merged in chunk order"""
    return int(nat.load().spp_graph_transformer_chunk())


def graph_transformer_workspace_bytes(num_targets):
    return int(nat.load().spp_graph_transformer_workspace_bytes(int(num_targets)))


class Fp8Table:
    """``Fp8Table(features)``: "read this fp8 table in place" (f3o).  The wrapped ``Fp8Features`` (q e4m3 [N, F],
    scale_log2 int8 [F], on the GPU) is accepted as ``x`` by ``graph_aggregate``, as every element of ``parts`` by
    ``graph_aggregate_parts`` and as ``x`` by the resident drivers -- ``layerwise_inference`` (``SAGE.inference``,
    ``GIN.inference``), ``evaluate``, ``field_inference``, ``field_evaluate`` -- for all four models.  Layer 0's
    aggregation reads the e4m3 rows through ``spp_graph_agg_forward_fp8`` and the GEMM tiles of the table's own rows come
    from ``spp_fp8_rows_f32``; both yield v = float32(q) * 2^scale_log2 exactly, so every result is the bits of the same
    call on ``features.dequantize(torch.float32)`` -- without that matrix (4 bytes an element) or an fp16 copy (2) beside
    the table (1).  A bare ``Fp8Features`` keeps being refused everywhere: reading in place is asked for, never assumed.

    ``table[ids]`` (int64 1-D tensor on the table's device) names rows of the table without copying them."""
    __slots__ = ("features", "ids")

    def __init__(self, features):
        if not isinstance(features, Fp8Features):
            raise TypeError(f"Fp8Table: wraps an Fp8Features (fp8.quantize_e4m3, fp8.load), got {type(features).__name__}")
        self.features, self.ids = features, None

    q = property(lambda self: self.features.q)
    scale_log2 = property(lambda self: self.features.scale_log2)
    device = property(lambda self: self.features.q.device)
    is_cuda = property(lambda self: self.features.q.is_cuda)
    dtype = property(lambda self: self.features.dtype)
    requires_grad = False

    @property
    def shape(self):
        return torch.Size((self.size(0), self.size(1)))

    def size(self, dim=None):
        if dim is None:
            return self.shape
        return self.features.q.size(1) if dim in (1, -1) else self.ids.numel() if self.ids is not None else self.features.q.size(0)

    def dim(self):
        return 2

    def __getitem__(self, ids):
        if self.ids is not None or not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() != 1 \
                or ids.device != self.device:
            raise TypeError("Fp8Table: rows are named by one 1-D int64 tensor on the table's device")
        rows = Fp8Table(self.features)
        rows.ids = ids.contiguous()
        return rows

    def __repr__(self):
        return f"Fp8Table(shape={tuple(self.shape)}, device={self.device})"

    def rows_f32(self, out, row0=None):
        """``spp_fp8_rows_f32``: out[j] = v[row0 + j], or v[ids[j]] for ``table[ids]``; ``out`` contiguous fp32 [n, F]"""
        f = self.features
        if out.size(0):
            with torch.cuda.device(out.device):
                nat.check(nat.load().spp_fp8_rows_f32(_p(f.q), f.q.size(0), f.q.size(1), _p(f.scale_log2),
                                                      -1 if self.ids is not None else int(row0),
                                                      _p(self.ids[row0:row0 + out.size(0)]) if self.ids is not None else None,
                                                      out.size(0), _p(out), _stream()))
        return out


# ---- the argument checks the wrappers and the drivers share; ``what`` is the caller's name in the message -----------
_FP8_TABLE_READERS = ("an fp8 table is read in place only as x of graph_aggregate, in parts of graph_aggregate_parts and as "
                      "x of layerwise_inference, evaluate, field_inference and field_evaluate")


def _check_matrix(x, what, name="x", fp8_reason="this argument is a matrix of activations or projected rows (fp16 / fp32 / "
                                                  "bf16), which no fp8 table is"):
    """x as the kernels read it: a 2-D fp16 / fp32 / bf16 matrix with unit column stride that carries no gradient"""
    if isinstance(x, Fp8Features):
        raise TypeError(f"{what}: an fp8 feature table (Fp8Features) is not supported as inference input; pass "
                        "x.dequantize(torch.float16), or inference.Fp8Table(x) where the table is read in place")
    if isinstance(x, Fp8Table):
        raise TypeError(f"{what}: {name} is an Fp8Table; {_FP8_TABLE_READERS}: {fp8_reason}")
    if isinstance(x, (TableRows, RowRefs)):
        raise TypeError(f"{what}: {type(x).__name__} describes the rows of one sampled batch; inference reads the whole "
                        "feature matrix, one row per graph node")
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(x).__name__}")
    if x.dim() != 2 or x.dtype not in _ELEM or (x.size(1) > 1 and x.stride(1) != 1):
        raise ValueError(f"{what}: {name} must be a 2-D fp16 / fp32 / bf16 matrix with unit column stride, got "
                         f"{tuple(x.shape)} {x.dtype} strides {tuple(x.stride())}")
    if x.requires_grad:
        raise RuntimeError(f"{what}: {name} requires grad, and inference is forward only (detach it)")


def _check_table(x, what):
    """``x`` of the entries that read an fp8 table in place: an ``Fp8Table`` of whole rows, or ``_check_matrix``"""
    if not isinstance(x, Fp8Table):
        return _check_matrix(x, what)
    if x.ids is not None:
        raise TypeError(f"{what}: x must be the whole Fp8Table (one row per graph node), not rows of it")


def _check_graph(what, N, rowptr, col, parts=False):
    """the whole graph's CSR, one row for each of the N rows of the matrix (or of the parts together)"""
    for name, t in (("rowptr", rowptr), ("col", col)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous 1-D int64 tensor")
    if rowptr.numel() != N + 1:
        raise ValueError(f"{what}: {f'the parts hold {N} rows' if parts else f'x has {N} rows'}, the graph "
                         f"{rowptr.numel() - 1} nodes (one row per node)")


def _check_out_dtype(what, out_dtype):
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")


def _check_heads(what, heads, Fdim):
    if not isinstance(heads, int) or heads < 1 or Fdim % heads != 0:
        raise ValueError(f"{what}: heads must be a positive int that divides F = {Fdim}, got {heads!r}")


def _check_epilogue(what, epilogue, parts=False):
    if parts and epilogue in _MAX_EPILOGUES:
        raise NotImplementedError(f"{what}: epilogue {epilogue!r}: {_MAX_OVER_PARTS}")
    if epilogue not in _EPILOGUES:
        raise ValueError(f"{what}: epilogue must be 'mean', 'operand', 'sum'{'' if parts else ', max or max_operand'}, "
                         f"got {epilogue!r}")


def _refuse_max_over_parts(what, model):
    if getattr(model, "aggr", "mean") == "max":
        raise NotImplementedError(f"{what}: {_MAX_OVER_PARTS}")


def _check_fp32(what, name, t, shape, meaning):
    """a contiguous fp32 tensor of exactly ``shape`` that carries no gradient"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) \
            or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor of shape {list(shape)} ({meaning})")
    if t.requires_grad:
        raise RuntimeError(f"{what}: {name} requires grad, and inference is forward only (detach it)")


def _check_row_address(what, noun, n, row0, row_ids):
    """the rows that go with the n rows of z: a slab (``row0`` >= 0) xor a list (``row_ids``: contiguous int64 [n]).
    Returns row0 as an int, None with a list."""
    if (row0 is None) == (row_ids is None):
        raise ValueError(f"{what}: address {noun} either as a slab (row0) or as row_ids"
                         + (", not both" if row0 is not None else ""))
    if row_ids is None:
        row0 = int(row0)
        if row0 < 0:
            raise ValueError(f"{what}: row0 must not be negative, got {row0}")
    elif not isinstance(row_ids, torch.Tensor) or row_ids.dtype != torch.int64 or tuple(row_ids.shape) != (n,) \
            or not row_ids.is_contiguous():
        raise ValueError(f"{what}: row_ids must be a contiguous int64 tensor of shape [{n}] (one entry per row of z)")
    return row0


def _check_targets(what, N, row0, num_targets, target_ids):
    """(row0 or -1, target_ids or None, T) of the two target forms: a slab inside the graph's N nodes, or a contiguous
    int64 list"""
    slab = row0 is not None or num_targets is not None
    if slab == (target_ids is not None):
        raise ValueError(f"{what}: give the targets either as a slab (row0 and num_targets) or as target_ids"
                         + (", not both" if slab else ""))
    if slab:
        if row0 is None or num_targets is None:
            raise ValueError(f"{what}: a slab needs both row0 and num_targets")
        row0, T = int(row0), int(num_targets)
        if row0 < 0 or T < 0 or row0 + T > N:
            raise ValueError(f"{what}: the slab [{row0}, {row0 + T}) leaves the graph's {N} nodes")
        return row0, None, T
    if not isinstance(target_ids, torch.Tensor) or target_ids.dtype != torch.int64 or target_ids.dim() != 1 \
            or not target_ids.is_contiguous():
        raise ValueError(f"{what}: target_ids must be a contiguous 1-D int64 tensor")
    return -1, target_ids, target_ids.numel()


def _check_out(what, out, out_dtype, T, width):
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != out_dtype
                            or tuple(out.shape) != (T, width) or (width > 1 and out.stride(1) != 1) or out.requires_grad):
        raise ValueError(f"{what}: out must be a {out_dtype} matrix of shape [{T}, {width}] with unit column stride "
                         "that does not require grad")


def _on_device(what, names, dev, tensors, workspace, workspace_bytes, T):
    """what follows the argument checks: the device is required, every tensor given lives on ``dev``, and the workspace
    (returned; allocated when None) holds ``workspace_bytes(T)`` bytes"""
    nat.require_device()
    if dev.type != "cuda" or not all(t.is_cuda and t.device == dev for t in tensors + [workspace] if t is not None):
        raise ValueError(f"{what}: {names} must live on one CUDA device")
    nbytes = workspace_bytes(T)
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < nbytes:
        raise ValueError(f"{what}: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes")
    return workspace


def _check_offsets(part_offsets, what):
    """part_offsets as a list of P + 1 ints: P in 1..SPP_GRAPH_AGG_MAX_PARTS, first entry 0, non-decreasing"""
    if isinstance(part_offsets, torch.Tensor):
        part_offsets = part_offsets.detach().cpu().tolist()
    off = [int(v) for v in part_offsets]
    P = len(off) - 1
    if not 1 <= P <= nat.SPP_GRAPH_AGG_MAX_PARTS:
        raise ValueError(f"{what}: part_offsets must hold 2..{nat.SPP_GRAPH_AGG_MAX_PARTS + 1} entries (one part to "
                         f"{nat.SPP_GRAPH_AGG_MAX_PARTS}), got {len(off)}")
    if off[0] != 0 or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"{what}: part_offsets must start at 0 and never decrease, got {off}")
    return off


def _fp8_parts(parts, what):
    """(the parts' e4m3 matrices, the exponents) when ``parts`` is a list of ``Fp8Table``; (parts, None) otherwise.  One
    exponent vector serves all parts, the first non-empty part's: that every part was quantised against the same
    exponents is the caller's duty, as on the exchange path (comparing them here would wait for the device)."""
    if isinstance(parts, P2PPeers) or not any(isinstance(t, Fp8Table) for t in parts):
        return parts, None
    tabs = list(parts)
    if not all(t is None or (isinstance(t, Fp8Table) and t.ids is None) for t in tabs):
        raise TypeError(f"{what}: fp8 parts are read in place when EVERY part is a whole Fp8Table (None for an empty "
                        f"one), got {sorted({type(t).__name__ for t in tabs})}")
    live = [t for t in tabs if t is not None and t.size(0)]
    return [None if t is None else t.q for t in tabs], (live or [t for t in tabs if t is not None])[0].scale_log2


def _parts_source(parts, off, dtype, F, what, name="part", fp8=False):
    """(base addresses [P], row stride in elements, dtype, F, device or None) of the two forms of ``parts``; ``fp8``:
    the tensors are ``_fp8_parts``' e4m3 matrices (an element is a byte)"""
    P = len(off) - 1
    if isinstance(parts, P2PPeers):
        if dtype not in _ELEM or not isinstance(F, int) or F < 0:
            raise ValueError(f"{what}: a P2PPeers source needs dtype= (fp16 / fp32 / bf16) and F= (the row width)")
        if len(parts.ptrs) != P:
            raise ValueError(f"{what}: {len(parts.ptrs)} peer tables for {P} parts")
        esize = torch.empty(0, dtype=dtype).element_size()
        if parts.stride % esize:
            raise ValueError(f"{what}: the peers' row stride ({parts.stride} bytes) is no multiple of the element size")
        for p in range(P):
            if off[p + 1] > off[p] and not parts.ptrs[p]:
                raise ValueError(f"{what}: {name} {p} holds the rows [{off[p]}, {off[p + 1]}) and has no address")
        return list(parts.ptrs), parts.stride // esize, dtype, F, None
    if dtype is not None or F is not None:
        raise ValueError(f"{what}: dtype= and F= describe a P2PPeers source; tensors carry their own")
    tabs = list(parts)
    if len(tabs) != P:
        raise ValueError(f"{what}: {len(tabs)} parts for {P} ranges of part_offsets")
    live = []
    for p, t in enumerate(tabs):
        rows = off[p + 1] - off[p]
        if t is None:
            if rows:
                raise ValueError(f"{what}: {name} {p} holds the rows [{off[p]}, {off[p + 1]}) and is None")
            continue
        if not fp8:
            _check_matrix(t, what, f"{name} {p}")
        if t.size(0) != rows:
            raise ValueError(f"{what}: {name} {p} has {t.size(0)} rows, part_offsets gives it {rows}")
        if rows:
            live.append((p, t))
    if not live:
        raise ValueError(f"{what}: every part is empty")
    first = live[0][1]
    if any(t.dtype != first.dtype or t.size(1) != first.size(1) for _p, t in live):
        raise ValueError(f"{what}: the parts must share one dtype and one row width, got "
                         f"{sorted({(str(t.dtype), t.size(1)) for _p, t in live})}")
    if any(t.device != first.device for _p, t in live):
        raise ValueError(f"{what}: in-process parts on different devices "
                         f"({sorted({str(t.device) for _p, t in live})}); parts of other devices are mapped by their "
                         "owners' handles (p2p_open_peers), nothing here enables peer access")
    strides = sorted({t.stride(0) for _p, t in live if t.size(0) > 1})     # (a part of one row has no stride of its own)
    if len(strides) > 1:
        raise ValueError(f"{what}: the parts must share one row stride, got {strides} elements")
    stride = strides[0] if strides else first.size(1)
    ptrs = [0] * P
    for p, t in live:
        ptrs[p] = t.data_ptr()
    return ptrs, stride, first.dtype, first.size(1), first.device


# ---- the kernels' launch functions: checked arguments in, ``out`` [T, width] (rows of a larger matrix allowed) written
def _request(rowptr, col, row0, target_ids, T, out):
    """the descriptor fields all four kernels share: the graph, the targets and where their rows go"""
    return dict(rowptr_dev=_p(rowptr), col_dev=_p(col), target_row0=row0, target_ids_dev=_p(target_ids), num_targets=T,
                out_elem=_ELEM[out.dtype], out_dev=_p(out), out_stride_elems=out.stride(0) if T > 1 else 0)


def _launch(entry, d, workspace, out, scale_log2=None):
    """``scale_log2``: the exponents of an fp8 table, the _fp8 entries' second argument"""
    with torch.cuda.device(out.device):
        nat.check(entry(C.byref(d), *([] if scale_log2 is None else [_p(scale_log2)]),
                        C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream()))
    return out


def _agg_launch(x, rowptr, col, epilogue, self_scale, row0, target_ids, T, out, workspace):
    """spp_graph_agg_forward: x [N, F] is one matrix; spp_graph_agg_forward_fp8: an ``Fp8Table`` read in place"""
    N, Fdim = x.shape
    if isinstance(x, Fp8Table):
        d = nat.GraphAggDesc(epilogue=_EPILOGUES[epilogue], x_elem=nat.SPP_ELEM_FP8_E4M3, x_dev=_p(x.q), x_stride_elems=Fdim,
                             x_rows=N, F=Fdim, self_scale=float(self_scale), **_request(rowptr, col, row0, target_ids, T, out))
        return _launch(nat.load().spp_graph_agg_forward_fp8, d, workspace, out, x.scale_log2)
    d = nat.GraphAggDesc(epilogue=_EPILOGUES[epilogue], x_elem=_ELEM[x.dtype], x_dev=_p(x),
                         x_stride_elems=x.stride(0) if N > 1 else Fdim, x_rows=N, F=Fdim, self_scale=float(self_scale),
                         **_request(rowptr, col, row0, target_ids, T, out))
    return _launch(nat.load().spp_graph_agg_forward, d, workspace, out)


def _agg_weighted_launch(x, rowptr, col, weight, dinv, fill, self_weight, row0, target_ids, T, out, workspace):
    """spp_graph_agg_weighted_forward: x [N, F] is one matrix; the weights explicit (``weight`` [E] or None for ones,
    ``self_weight`` [N] or None) or, with ``dinv`` [N], formed in the kernel from it and ``fill``"""
    N, Fdim = x.shape
    d = nat.GraphAggWeightedDesc(x_elem=_ELEM[x.dtype], fill=int(fill), x_dev=_p(x),
                                 x_stride_elems=x.stride(0) if N > 1 else Fdim, x_rows=N, F=Fdim, w_dev=_p(weight),
                                 dinv_dev=_p(dinv), self_w_dev=_p(self_weight),
                                 **_request(rowptr, col, row0, target_ids, T, out))
    return _launch(nat.load().spp_graph_agg_weighted_forward, d, workspace, out)


def _agg_parts_launch(src, off, rowptr, col, epilogue, self_scale, row0, target_ids, T, out, workspace, scale_log2=None):
    """spp_graph_agg_parts_forward: ``src`` is ``_parts_source``'s (base addresses, row stride, dtype, F); with
    ``scale_log2`` spp_graph_agg_parts_forward_fp8 over e4m3 parts"""
    ptrs, stride, x_dtype, Fdim = src
    fp8 = scale_log2 is not None
    d = nat.GraphAggPartsDesc(epilogue=_EPILOGUES[epilogue], x_elem=nat.SPP_ELEM_FP8_E4M3 if fp8 else _ELEM[x_dtype],
                              num_parts=len(off) - 1,
                              x_stride_elems=stride, F=Fdim, self_scale=float(self_scale),
                              **_request(rowptr, col, row0, target_ids, T, out))
    for p, v in enumerate(off):
        d.part_offsets[p] = v
    for p, v in enumerate(ptrs):
        d.x_parts_dev[p] = v or None
    L = nat.load()
    return _launch(L.spp_graph_agg_parts_forward_fp8 if fp8 else L.spp_graph_agg_parts_forward, d, workspace, out, scale_log2)


def _gat_launch(h, a_src, a_dst, rowptr, col, heads, negative_slope, relu, row0, target_ids, T, out, workspace):
    """spp_graph_gat_forward: h [N, F] is one matrix, its logits two contiguous fp32 [N, heads]"""
    N, Fdim = h.shape
    d = nat.GraphGatDesc(x_elem=_ELEM[h.dtype], heads=heads, relu=int(bool(relu)), x_dev=_p(h),
                         x_stride_elems=h.stride(0) if N > 1 else Fdim, x_rows=N, F=Fdim, a_src_dev=_p(a_src),
                         a_dst_dev=_p(a_dst), negative_slope=float(negative_slope),
                         **_request(rowptr, col, row0, target_ids, T, out))
    return _launch(nat.load().spp_graph_gat_forward, d, workspace, out)


def _gatv2_launch(x_l, x_r, att, rowptr, col, negative_slope, relu, row0, target_ids, T, out, workspace):
    """spp_graph_gatv2_forward: x_l and x_r [N, H * C] by global id (x_r may be x_l), att contiguous fp32 [H, C]"""
    N, D = x_l.shape
    H, Cc = att.shape
    d = nat.GraphGatv2Desc(x_elem=_ELEM[x_l.dtype], heads=H, relu=int(bool(relu)), x_l_dev=_p(x_l),
                           x_l_stride_elems=x_l.stride(0) if N > 1 else D, x_r_dev=_p(x_r),
                           x_r_stride_elems=x_r.stride(0) if N > 1 else D, x_rows=N, C=Cc, att_dev=_p(att),
                           negative_slope=float(negative_slope), **_request(rowptr, col, row0, target_ids, T, out))
    return _launch(nat.load().spp_graph_gatv2_forward, d, workspace, out)


def _transformer_launch(q, k, v, skip, heads, scale, rowptr, col, relu, row0, target_ids, T, out, workspace):
    """spp_graph_transformer_forward: q, k, v [N, H * C] by global id (k and v may be the halves of one matrix), skip
    None or [N, H * C] of their dtype (it may be the matrix ``out`` is a slab of)"""
    N, D = q.shape
    stride = lambda t: t.stride(0) if N > 1 else D
    d = nat.GraphTransformerDesc(x_elem=_ELEM[q.dtype], heads=heads, relu=int(bool(relu)), q_dev=_p(q),
                                 q_stride_elems=stride(q), k_dev=_p(k), k_stride_elems=stride(k), v_dev=_p(v),
                                 v_stride_elems=stride(v), x_rows=N, C=D // heads, skip_dev=_p(skip),
                                 skip_stride_elems=stride(skip) if skip is not None else 0, scale=float(scale),
                                 **_request(rowptr, col, row0, target_ids, T, out))
    return _launch(nat.load().spp_graph_transformer_forward, d, workspace, out)


def _gat_parts_launch(src, a_src, off, rowptr, col, heads, negative_slope, relu, row0, target_ids, T, out, workspace):
    """spp_graph_gat_parts_forward: ``src`` as for ``_agg_parts_launch``, ``a_src`` the logits' (base addresses, row
    stride)"""
    ptrs, stride, x_dtype, Fdim = src
    a_ptrs, a_stride = a_src
    d = nat.GraphGatPartsDesc(x_elem=_ELEM[x_dtype], heads=heads, relu=int(bool(relu)), num_parts=len(off) - 1,
                              x_stride_elems=stride, a_stride_elems=a_stride, F=Fdim,
                              negative_slope=float(negative_slope), **_request(rowptr, col, row0, target_ids, T, out))
    for p, v in enumerate(off):
        d.part_offsets[p] = v
    for p, (hv, av) in enumerate(zip(ptrs, a_ptrs)):
        d.h_parts_dev[p], d.a_parts_dev[p] = hv or None, av or None
    return _launch(nat.load().spp_graph_gat_parts_forward, d, workspace, out)


# ---- the kernels' public wrappers ------------------------------------------------------------------------------------
def graph_aggregate(x, rowptr, col, *, row0=None, num_targets=None, target_ids=None, epilogue="mean", self_scale=0.0,
                    out_dtype=torch.float32, workspace=None):
    """Aggregation over whole rows of the resident graph (``spp_graph_agg_forward``, include/spp.h).

    ``x`` [N, F]: one row per graph node (fp16 / fp32 / bf16, possibly a strided view) -- or an ``Fp8Table``, read in
    place by ``spp_graph_agg_forward_fp8`` with the bits of the same call on its fp32 dequantisation; ``rowptr`` /
    ``col``: the graph's CSR (int64, global ids).  The targets are a slab, ``row0`` and ``num_targets`` (output row i is node
    row0 + i), or a list, ``target_ids`` (int64, any order, duplicates allowed).  ``epilogue``: "mean" [T, F],
    "operand" [T, 2F] = [mean | x[target]], "sum" [T, F] = self_scale * x[target] + sum, "max" [T, F] = the element-wise
    maximum over the row (the bits of ``models.max_aggregate`` for every row length; an empty row gives 0) or
    "max_operand" [T, 2F] = [max | x[target]].  fp32 sums; a bf16 output is rounded once.  A ``col`` entry outside the graph reads row 0, a target id outside it gives a row of zeros.

    Forward only: no autograd node is registered and an input that requires grad is refused.  ``workspace``: a uint8
    CUDA tensor of at least ``graph_agg_workspace_bytes(T)`` bytes, reusable between calls on one stream; allocated
    when None.  Nothing here waits for the device."""
    what = "graph_aggregate"
    _check_table(x, what)
    N, Fdim = x.shape
    _check_graph(what, N, rowptr, col)
    _check_epilogue(what, epilogue)
    _check_out_dtype(what, out_dtype)
    row0, target_ids, T = _check_targets(what, N, row0, num_targets, target_ids)
    workspace = _on_device(what, "x, rowptr, col, target_ids and workspace", x.device,
                           [x.q if isinstance(x, Fp8Table) else x, rowptr, col, target_ids],
                           workspace, graph_agg_workspace_bytes, T)
    out = torch.empty((T, 2 * Fdim if epilogue in _WIDE_EPILOGUES else Fdim), dtype=out_dtype, device=x.device)
    return _agg_launch(x, rowptr, col, epilogue, self_scale, row0, target_ids, T, out, workspace)


_WEIGHTS_NOT_BUILT = ("the weighted aggregation reads one resident fp16 / fp32 / bf16 matrix: a row-partitioned x, fp8 tables "
                      "and the receptive-field entries take no edge weights")


def _check_fill(what, fill):
    if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill <= 2:
        raise ValueError(f"{what}: fill must be 0 (no self loops), 1 or 2 (improved), got {fill!r}")


def graph_weighted_aggregate(x, rowptr, col, *, weight=None, dinv=None, fill=1, self_weight=None, row0=None,
                             num_targets=None, target_ids=None, out_dtype=torch.float32, out=None, workspace=None):
    """The edge-weighted sum over whole rows of the resident graph (``spp_graph_agg_weighted_forward``, include/spp.h
    f3s): ``out[i] = sum_k c_k * x[col[k]]`` over target i's row, plus a self term, [T, F] fp32 or bf16.

    ``x``, ``rowptr`` / ``col``, the targets (``row0`` and ``num_targets``, or ``target_ids``), ``out_dtype`` and
    ``workspace`` as ``graph_aggregate``; ``out``: an fp32 / bf16 [T, F] matrix to write into (rows of a larger one
    allowed).  The weights, all contiguous fp32 without gradient:

      ``weight`` [E]       one value per entry of ``col``; None: every entry weighs 1
      ``self_weight`` [N]  by global node id: ``self_weight[t] * x[t]`` is added last; None: no self term
      ``dinv`` [N]         (``gcn_dinv``) instead of ``self_weight``: the kernel forms PyG's gcn_norm itself,
                           ``c_k = dinv[t] * weight[k] * dinv[col[k]]`` and the self term ``dinv[t] * fill * dinv[t]``
                           (``fill`` 0, 1 or 2; none for 0) -- the bits of ``models.gcn_norm``'s coefficients over the
                           whole graph, without an [E] array.  ``fill`` is read only with ``dinv``.

    One fp32 fmaf per entry in CSR order from zero, the self term last: for a row of at most ``graph_agg_chunk()``
    entries the bits of ``models.weighted_aggregate``; a longer row is chunks of that many entries whose sums are added in
    chunk order.  An ``Fp8Table``, fp8 features and a row-partitioned ``x`` are refused.  Forward only; nothing here
    waits for the device."""
    what = "graph_weighted_aggregate"
    if isinstance(x, (list, tuple, P2PPeers)):
        raise NotImplementedError(f"{what}: x is row-partitioned ({type(x).__name__}); {_WEIGHTS_NOT_BUILT}")
    _check_matrix(x, what, fp8_reason=_WEIGHTS_NOT_BUILT)
    N, Fdim = x.shape
    _check_graph(what, N, rowptr, col)
    if weight is not None:
        _check_fp32(what, "weight", weight, (col.numel(),), "one value per entry of col")
    if dinv is not None:
        if self_weight is not None:
            raise ValueError(f"{what}: give dinv or self_weight, not both (with dinv the self term is "
                             "dinv[t] * fill * dinv[t])")
        _check_fp32(what, "dinv", dinv, (N,), "one value per graph node: gcn_dinv")
        _check_fill(what, fill)
    if self_weight is not None:
        _check_fp32(what, "self_weight", self_weight, (N,), "one value per graph node, by global id")
    _check_out_dtype(what, out_dtype)
    row0, target_ids, T = _check_targets(what, N, row0, num_targets, target_ids)
    _check_out(what, out, out_dtype, T, Fdim)
    workspace = _on_device(what, "x, rowptr, col, weight, dinv, self_weight, target_ids, workspace and out", x.device,
                           [x, rowptr, col, weight, dinv, self_weight, target_ids, out], workspace,
                           graph_agg_workspace_bytes, T)
    if out is None:
        out = torch.empty((T, Fdim), dtype=out_dtype, device=x.device)
    return _agg_weighted_launch(x, rowptr, col, weight, dinv, fill if dinv is not None else 0, self_weight, row0,
                                target_ids, T, out, workspace)


def gcn_dinv(rowptr, edge_weight=None, *, add_self_loops=True, improved=False):
    """``deg^-1/2`` of PyG's gcn_norm over the whole graph (``spp_gcn_dinv``): fp32 [N] with
    ``dinv[t] = (fill + sum of row t's edge_weight)^-1/2`` in CSR order -- the row length without ``edge_weight`` -- and 0
    where that is inf; ``fill`` = 1, 2 with ``improved``, 0 without self loops.  The first pass of ``models.gcn_norm``
    (the same kernel, the same bits) without its [E] coefficients: ``graph_weighted_aggregate(dinv=...)`` forms those.
    One thread walks a row, a hub's included; it runs once per evaluation."""
    what = "gcn_dinv"
    if not isinstance(rowptr, torch.Tensor) or rowptr.dtype != torch.int64 or rowptr.dim() != 1 or rowptr.numel() < 1 \
            or not rowptr.is_contiguous():
        raise ValueError(f"{what}: rowptr must be a contiguous 1-D int64 tensor of N + 1 entries")
    if edge_weight is not None:
        if not isinstance(edge_weight, torch.Tensor) or edge_weight.dtype != torch.float32 or edge_weight.dim() != 1 \
                or not edge_weight.is_contiguous():
            raise ValueError(f"{what}: edge_weight must be a contiguous 1-D fp32 tensor (one value per entry of col)")
        if edge_weight.requires_grad:
            raise RuntimeError(f"{what}: edge_weight requires grad, and inference is forward only (detach it)")
    nat.require_device()
    if not rowptr.is_cuda or (edge_weight is not None and edge_weight.device != rowptr.device):
        raise ValueError(f"{what}: rowptr and edge_weight must live on one CUDA device")
    N = rowptr.numel() - 1
    dinv = torch.empty(N, dtype=torch.float32, device=rowptr.device)
    d = nat.GcnDinvDesc(fill=_gcn_fill(add_self_loops, improved), rowptr_dev=_p(rowptr), num_nodes=N, w_dev=_p(edge_weight),
                        dinv_dev=_p(dinv))
    with torch.cuda.device(rowptr.device):
        nat.check(nat.load().spp_gcn_dinv(C.byref(d), _stream()))
    return dinv


def graph_aggregate_parts(parts, part_offsets, rowptr, col, *, row0=None, num_targets=None, target_ids=None,
                          epilogue="mean", self_scale=0.0, out_dtype=torch.float32, workspace=None, out=None,
                          dtype=None, F=None):
    """``graph_aggregate`` over a row-partitioned source (``spp_graph_agg_parts_forward``, include/spp.h): part p holds
    the global rows [part_offsets[p], part_offsets[p + 1]) of x, in an allocation of its own.  The result is the bits of
    ``graph_aggregate(torch.cat(parts), ...)``.

    ``parts``: a list of P CUDA tensors on one device (an empty part may be None or have 0 rows) that share dtype, width
    and row stride -- or a ``P2PPeers`` (the ranks' partitions as addresses in this process, ``p2p_open_peers``) with
    ``dtype=`` and ``F=`` -- or a list of ``Fp8Table`` (None for an empty part), read in place by
    ``spp_graph_agg_parts_forward_fp8`` with the first non-empty part's exponents for all of them (that the parts agree on
    the exponents is the caller's duty).  ``rowptr`` / ``col``: the WHOLE graph's CSR with global ids; the targets, ``epilogue``,
    ``self_scale``, ``out_dtype`` and ``workspace`` as ``graph_aggregate``, the ids global.  ``out``: an fp32 / bf16
    [T, F or 2F] matrix to write into (rows of a larger one allowed).  Nothing here maps memory or enables peer access,
    and nothing waits for the device."""
    what = "graph_aggregate_parts"
    if epilogue in _MAX_EPILOGUES:
        _check_epilogue(what, epilogue, parts=True)      # (refused whatever the parts are)
    off = _check_offsets(part_offsets, what)
    parts, scale_log2 = _fp8_parts(parts, what)
    *src, dev = _parts_source(parts, off, dtype, F, what, fp8=scale_log2 is not None)
    _check_graph(what, off[-1], rowptr, col, parts=True)
    _check_epilogue(what, epilogue, parts=True)
    _check_out_dtype(what, out_dtype)
    row0, target_ids, T = _check_targets(what, off[-1], row0, num_targets, target_ids)
    width = 2 * src[3] if epilogue == "operand" else src[3]
    _check_out(what, out, out_dtype, T, width)
    dev = rowptr.device if dev is None else dev
    workspace = _on_device(what, "the parts, rowptr, col, target_ids, workspace and out", dev,
                           [rowptr, col, target_ids, out, scale_log2], workspace, graph_agg_workspace_bytes, T)
    if out is None:
        out = torch.empty((T, width), dtype=out_dtype, device=dev)
    return _agg_parts_launch(src, off, rowptr, col, epilogue, self_scale, row0, target_ids, T, out, workspace, scale_log2)


def graph_gat_aggregate(h, a_src, a_dst, rowptr, col, *, heads, negative_slope=0.2, relu=False, row0=None,
                        num_targets=None, target_ids=None, out_dtype=torch.float32, workspace=None):
    """GATConv's attention over whole rows of the resident graph (``spp_graph_gat_forward``, include/spp.h).

    ``h`` [N, F]: one PROJECTED row per graph node (fp16 / fp32 / bf16, possibly a strided view), F = heads * C with
    head k in columns k*C .. (k+1)*C; ``a_src`` / ``a_dst``: contiguous fp32 [N, heads], the logits' two halves;
    ``rowptr`` / ``col``: the graph's CSR (int64, global ids).  The targets are a slab, ``row0`` and ``num_targets``,
    or a list, ``target_ids`` (int64, any order, duplicates allowed).  Output row i, head k: the softmax over node t's
    row without its diagonal entries plus one self loop, of leaky_relu(a_src[j, k] + a_dst[t, k]), applied to the rows
    h[j, k*C:(k+1)*C]; through a ReLU with ``relu=True``.  fp32 state; a bf16 output is rounded once.  A ``col`` entry
    outside the graph is node 0, a target id outside it gives a row of zeros.

    Forward only: no autograd node is registered and an input that requires grad is refused.  ``workspace``: a uint8
    CUDA tensor of at least ``graph_gat_workspace_bytes(T)`` bytes, reusable between calls on one stream; allocated
    when None.  Nothing here waits for the device."""
    what = "graph_gat_aggregate"
    _check_matrix(h, what)
    N, Fdim = h.shape
    _check_graph(what, N, rowptr, col)
    _check_heads(what, heads, Fdim)
    for name, t in (("a_src", a_src), ("a_dst", a_dst)):
        _check_fp32(what, name, t, (N, heads), "nodes, heads")
    _check_out_dtype(what, out_dtype)
    row0, target_ids, T = _check_targets(what, N, row0, num_targets, target_ids)
    workspace = _on_device(what, "h, a_src, a_dst, rowptr, col, target_ids and workspace", h.device,
                           [h, a_src, a_dst, rowptr, col, target_ids], workspace, graph_gat_workspace_bytes, T)
    out = torch.empty((T, Fdim), dtype=out_dtype, device=h.device)
    return _gat_launch(h, a_src, a_dst, rowptr, col, heads, negative_slope, relu, row0, target_ids, T, out, workspace)


_GATV2_HEADS = (1, 2, 4, 8)                              # the head counts the GATv2 kernels are built for
_GATV2_MAX_D = 1024                                      # ... and their widest row, heads * C


def _gatv2_pad(Cc):
    """the smallest Cp >= Cc with Cp % 4 == 0 and Cp / 4 a power of two: the channels per head the kernels take"""
    g = 1
    while 4 * g < Cc:
        g *= 2
    return 4 * g


def _check_gatv2_rows(what, name, t):
    if t.stride(0) % 4 != 0 or t.data_ptr() % (4 * t.element_size()) != 0:
        raise ValueError(f"{what}: the rows of {name} must be aligned to 4 elements, base and stride (the kernels move "
                         f"four columns per lane); got stride {t.stride(0)} elements, address % {4 * t.element_size()} = "
                         f"{t.data_ptr() % (4 * t.element_size())}")


def graph_gatv2_aggregate(x_l, x_r, att, rowptr, col, *, negative_slope=0.2, relu=False, row0=None, num_targets=None,
                          target_ids=None, out_dtype=torch.float32, out=None, workspace=None):
    """GATv2Conv's attention over whole rows of the resident graph (``spp_graph_gatv2_forward``, include/spp.h f3w).

    ``x_l`` / ``x_r`` [N, H * C]: the PROJECTED rows lin_l(x) and lin_r(x), one per graph node and both indexed by
    global node id (fp16 / fp32 / bf16, one dtype, possibly strided views with rows aligned to 4 elements); ``x_r`` may
    be ``x_l`` itself (share_weights).  ``att``: contiguous fp32 [H, C].  ``rowptr`` / ``col``: the graph's CSR (int64,
    global ids).  The targets are a slab, ``row0`` and ``num_targets``, or a list, ``target_ids`` (int64, any order,
    duplicates allowed).  Output row i, head h: the softmax over node t's row without its diagonal entries plus one self
    loop, of e_j = att[h] . leaky_relu(x_l[j, h] + x_r[t, h]), applied to the rows x_l[j, h*C:(h+1)*C]; through a ReLU
    with ``relu=True``.  fp32 state; a bf16 output is rounded once.  A ``col`` entry outside the graph is node 0, a
    target id outside it gives a row of zeros.  The kernels are built for H in {1, 2, 4, 8}, C % 4 == 0 with C / 4 a
    power of two and H * C <= 1024; any other shape is a ``ValueError`` (``gatv2_inference`` pads C itself).

    Forward only: no autograd node is registered and an input that requires grad is refused.  ``out``: where the rows
    go ([T, H * C] of ``out_dtype``, rows aligned to 4 elements; allocated when None).  ``workspace``: a uint8 CUDA
    tensor of at least ``graph_gatv2_workspace_bytes(T)`` bytes, reusable between calls on one stream; allocated when
    None.  Nothing here waits for the device."""
    what = "graph_gatv2_aggregate"
    _check_matrix(x_l, what, name="x_l")
    _check_matrix(x_r, what, name="x_r")
    N, D = x_l.shape
    if tuple(x_r.shape) != (N, D) or x_r.dtype != x_l.dtype:
        raise ValueError(f"{what}: x_r must have x_l's shape and dtype ({[N, D]} {x_l.dtype}: both are indexed by global "
                         f"node id), got {list(x_r.shape)} {x_r.dtype}")
    _check_graph(what, N, rowptr, col)
    if not isinstance(att, torch.Tensor) or att.dim() != 2:
        raise ValueError(f"{what}: att must be a contiguous fp32 tensor of shape [heads, C]")
    H, Cc = att.shape
    _check_fp32(what, "att", att, (H, Cc), "heads, channels per head")
    if H not in _GATV2_HEADS:
        raise ValueError(f"{what}: heads must be 1, 2, 4 or 8 (the kernels' head counts), got att of {H} rows")
    if Cc < 4 or _gatv2_pad(Cc) != Cc:
        raise ValueError(f"{what}: C must be a multiple of 4 with C / 4 a power of two (the per-head reduction is a "
                         f"butterfly over aligned lane segments), got C = {Cc}; zero-pad the channels to {_gatv2_pad(Cc)}")
    if H * Cc != D or D > _GATV2_MAX_D:
        raise ValueError(f"{what}: the rows must be heads * C = {H} * {Cc} = {H * Cc} <= {_GATV2_MAX_D} wide, got {D}")
    _check_gatv2_rows(what, "x_l", x_l)
    _check_gatv2_rows(what, "x_r", x_r)
    _check_out_dtype(what, out_dtype)
    row0, target_ids, T = _check_targets(what, N, row0, num_targets, target_ids)
    _check_out(what, out, out_dtype, T, D)
    if out is not None:
        _check_gatv2_rows(what, "out", out)
    workspace = _on_device(what, "x_l, x_r, att, rowptr, col, target_ids, out and workspace", x_l.device,
                           [x_l, x_r, att, rowptr, col, target_ids, out], workspace, graph_gatv2_workspace_bytes, T)
    if out is None:
        out = torch.empty((T, D), dtype=out_dtype, device=x_l.device)
    return _gatv2_launch(x_l, x_r, att, rowptr, col, negative_slope, relu, row0, target_ids, T, out, workspace)


def graph_transformer_aggregate(q, k, v, rowptr, col, *, heads, scale, skip=None, relu=False, row0=None,
                                num_targets=None, target_ids=None, out_dtype=torch.float32, out=None, workspace=None):
    """TransformerConv's attention over whole rows of the resident graph (``spp_graph_transformer_forward``,
    include/spp.h f3z).

    ``q`` / ``k`` / ``v`` [N, H * C]: the PROJECTED rows lin_query(x), lin_key(x) and lin_value(x), one per graph node
    and all indexed by global node id (fp16 / fp32 / bf16, one dtype, possibly strided views with rows aligned to 4
    elements: ``k`` and ``v`` may be the halves of one [N, 2 * H * C] matrix).  ``rowptr`` / ``col``: the graph's CSR
    (int64, global ids).  The targets are a slab, ``row0`` and ``num_targets``, or a list, ``target_ids`` (int64, any
    order, duplicates allowed).  Output row i, head h: the softmax over EVERY entry of node t's row -- no self loop,
    diagonal entries kept, repeats counted -- of e_j = ``scale`` * q[t, h] . k[j, h], applied to the rows
    v[j, h*C:(h+1)*C]; a row without entries gives zeros.  Then ``skip[t]`` is added (``skip``: [N, H * C] of the rows'
    dtype, by global id; None: nothing), then the ReLU with ``relu=True``, then one rounding to ``out_dtype``.  fp32
    state.  A ``col`` entry outside the graph is node 0, a target id outside it gives a row of zeros (no skip).
    ``skip`` may be the matrix ``out`` is a slab of (``out = skip[row0:row0 + num_targets]``): a lane reads its columns
    before it writes them.  The kernels are built for H in {1, 2, 4, 8}, C % 4 == 0 with C / 4 a power of two and
    H * C <= 1024; any other shape is a ``ValueError`` (``layerwise_inference`` pads C itself).

    Forward only: no autograd node is registered and an input that requires grad is refused.  ``out``: where the rows
    go ([T, H * C] of ``out_dtype``, rows aligned to 4 elements; allocated when None).  ``workspace``: a uint8 CUDA
    tensor of at least ``graph_transformer_workspace_bytes(T)`` bytes, reusable between calls on one stream; allocated
    when None.  Nothing here waits for the device."""
    what = "graph_transformer_aggregate"
    _check_matrix(q, what, name="q")
    N, D = q.shape
    rows = [("k", k), ("v", v)] + ([("skip", skip)] if skip is not None else [])
    for name, t in rows:
        _check_matrix(t, what, name=name)
        if tuple(t.shape) != (N, D) or t.dtype != q.dtype:
            raise ValueError(f"{what}: {name} must have q's shape and dtype ({[N, D]} {q.dtype}: all are indexed by global "
                             f"node id), got {list(t.shape)} {t.dtype}")
    _check_graph(what, N, rowptr, col)
    if isinstance(heads, bool) or not isinstance(heads, int) or heads not in _GATV2_HEADS:
        raise ValueError(f"{what}: heads must be 1, 2, 4 or 8 (the kernels' head counts), got {heads!r}")
    Cc = D // heads
    if D % heads != 0 or Cc < 4 or _gatv2_pad(Cc) != Cc:
        raise ValueError(f"{what}: C = D / heads must be a multiple of 4 with C / 4 a power of two (the per-head reduction "
                         f"is a butterfly over aligned lane segments), got D = {D} with heads = {heads}; zero-pad the "
                         f"channels to {_gatv2_pad(max(-(-D // heads), 1))}")
    if D > _GATV2_MAX_D:
        raise ValueError(f"{what}: the rows must be heads * C = {heads} * {Cc} = {D} <= {_GATV2_MAX_D} wide")
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not (0.0 < float(scale) < float("inf")):
        raise ValueError(f"{what}: scale must be a finite positive number (the layer's is 1 / sqrt(C)), got {scale!r}")
    for name, t in [("q", q)] + rows:
        _check_gatv2_rows(what, name, t)
    _check_out_dtype(what, out_dtype)
    row0, target_ids, T = _check_targets(what, N, row0, num_targets, target_ids)
    _check_out(what, out, out_dtype, T, D)
    if out is not None:
        _check_gatv2_rows(what, "out", out)
    workspace = _on_device(what, "q, k, v, skip, rowptr, col, target_ids, out and workspace", q.device,
                           [q, k, v, skip, rowptr, col, target_ids, out], workspace, graph_transformer_workspace_bytes, T)
    if out is None:
        out = torch.empty((T, D), dtype=out_dtype, device=q.device)
    return _transformer_launch(q, k, v, skip, heads, scale, rowptr, col, relu, row0, target_ids, T, out, workspace)


def graph_gat_aggregate_parts(h_parts, a_parts, part_offsets, rowptr, col, *, heads, negative_slope=0.2, relu=False,
                              row0=None, num_targets=None, target_ids=None, out_dtype=torch.float32, out=None,
                              workspace=None, dtype=None, F=None):
    """``graph_gat_aggregate`` over a row-partitioned h with its logits (``spp_graph_gat_parts_forward``, include/spp.h):
    part p holds the global rows [part_offsets[p], part_offsets[p + 1]) of h and of the logits, in allocations of its own.
    The result is the bits of ``graph_gat_aggregate(torch.cat(h_parts), a[:, :heads], a[:, heads:], ...)`` with
    ``a = torch.cat(a_parts)``.

    ``h_parts``: a list of P CUDA tensors on one device (an empty part may be None or have 0 rows) that share dtype,
    width F = heads * C and row stride -- or a ``P2PPeers`` with ``dtype=`` and ``F=`` (the width read, which may be less
    than the published buffer's).  ``a_parts``: each part's logits as ONE fp32 matrix [rows_p, 2 * heads] = [a_src | a_dst]
    (unit column stride, one row stride for all parts, which may exceed 2 * heads) -- or a ``P2PPeers``.  ``rowptr`` /
    ``col``: the WHOLE graph's CSR with global ids; ``heads``, ``negative_slope``, ``relu``, the targets (global ids),
    ``out_dtype`` and ``workspace`` as ``graph_gat_aggregate``.  ``out``: an fp32 / bf16 [T, F] matrix to write into (rows
    of a larger one allowed).  Nothing here maps memory or enables peer access, and nothing waits for the device."""
    what = "graph_gat_aggregate_parts"
    off = _check_offsets(part_offsets, what)
    *src, dev = _parts_source(h_parts, off, dtype, F, what)
    Fdim = src[3]
    _check_heads(what, heads, Fdim)
    peer_logits = isinstance(a_parts, P2PPeers)
    a_ptrs, a_stride, a_dtype, a_width, a_dev = _parts_source(
        a_parts, off, torch.float32 if peer_logits else None, 2 * heads if peer_logits else None, what, "logits part")
    if a_dtype != torch.float32 or a_width != 2 * heads:
        raise ValueError(f"{what}: every logits part must be an fp32 matrix [rows, 2 * heads = {2 * heads}] "
                         f"([a_src | a_dst]), got {a_dtype} of width {a_width}")
    if a_stride < 2 * heads:
        raise ValueError(f"{what}: the logits' row stride ({a_stride} elements) is smaller than 2 * heads = {2 * heads}")
    if dev is not None and a_dev is not None and dev != a_dev:
        raise ValueError(f"{what}: h_parts ({dev}) and a_parts ({a_dev}) live on different devices")
    dev = a_dev if dev is None else dev
    _check_graph(what, off[-1], rowptr, col, parts=True)
    _check_out_dtype(what, out_dtype)
    row0, target_ids, T = _check_targets(what, off[-1], row0, num_targets, target_ids)
    _check_out(what, out, out_dtype, T, Fdim)
    dev = rowptr.device if dev is None else dev
    workspace = _on_device(what, "the parts, rowptr, col, target_ids, workspace and out", dev,
                           [rowptr, col, target_ids, out], workspace, graph_gat_workspace_bytes, T)
    if out is None:
        out = torch.empty((T, Fdim), dtype=out_dtype, device=dev)
    return _gat_parts_launch(src, (a_ptrs, a_stride), off, rowptr, col, heads, negative_slope, relu, row0, target_ids, T,
                             out, workspace)


def resinc_epilogue(z, scale, shift, *, negative_slope, residual=None, row0=None, row_ids=None, out=None,
                    out_dtype=None):
    """SAGEResInception's layer tail in eval mode, one pass (``spp_resinc_epilogue``, include/spp.h):

        out[i, c] = leaky_relu(scale[c] * z[i, c] + shift[c], negative_slope) + residual[row(i), c]

    in fp32 (one fma, the slope, the add), rounded once when ``out`` is bf16.  ``z`` [n, C]: fp32 / bf16, possibly a
    strided view (the columns of a GEMM tile); ``scale`` / ``shift``: contiguous fp32 [C], BatchNorm's running
    statistics folded by the caller (scale = gamma / sqrt(var + eps), shift = beta - mean * scale).  ``residual``
    [R, C]: fp16 / fp32 / bf16, read in place, either as a slab, ``row0`` (row(i) = row0 + i), or by a list,
    ``row_ids`` (int64 [n], any order, duplicates allowed); a row index outside [0, R) gives an output row of zeros.
    ``out``: an fp32 / bf16 [n, C] matrix to write into (rows of a larger matrix allowed; must not overlap rows of
    ``z`` or ``residual`` that the call still reads); allocated in ``out_dtype`` (default fp32) when None.

    Forward only: no autograd node is registered and an input that requires grad is refused.  Nothing here waits for the
    device."""
    what = "resinc_epilogue"
    _check_matrix(z, what, "z")
    if z.dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: z must be fp32 or bf16, got {z.dtype}")
    n, Cdim = z.shape
    if Cdim < 1:
        raise ValueError(f"{what}: z needs at least one column, got {tuple(z.shape)}")
    for name, t in (("scale", scale), ("shift", shift)):
        _check_fp32(what, name, t, (Cdim,), "one entry per column")
    if residual is None:
        if row0 is not None or row_ids is not None:
            raise ValueError(f"{what}: row0 / row_ids address the residual's rows, and there is no residual")
    else:
        _check_matrix(residual, what, "residual")
        if residual.size(1) != Cdim or residual.size(0) < 1:
            raise ValueError(f"{what}: residual must have z's {Cdim} columns and at least one row, got "
                             f"{tuple(residual.shape)}")
        row0 = _check_row_address(what, "the residual's rows", n, row0, row_ids)
    if out is None:
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        _check_out_dtype(what, out_dtype)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype not in _OUT_DTYPES or tuple(out.shape) != (n, Cdim) \
                or (Cdim > 1 and out.stride(1) != 1) or out.requires_grad:
            raise ValueError(f"{what}: out must be an fp32 / bf16 matrix of shape [{n}, {Cdim}] with unit column stride "
                             "that does not require grad")
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError(f"{what}: out is {out.dtype}, out_dtype {out_dtype}")
    nat.require_device()
    tensors = [z, scale, shift] + [t for t in (residual, row_ids, out) if t is not None]
    if not all(t.is_cuda and t.device == z.device for t in tensors):
        raise ValueError(f"{what}: z, scale, shift, residual, row_ids and out must live on one CUDA device")
    if out is None:
        out = torch.empty((n, Cdim), dtype=out_dtype, device=z.device)
    d = nat.ResincEpilogueDesc(z_elem=_ELEM[z.dtype], out_elem=_ELEM[out.dtype], negative_slope=float(negative_slope),
                               z_dev=_p(z), z_stride_elems=z.stride(0) if n > 1 else Cdim, a_dev=_p(scale),
                               b_dev=_p(shift), n=n, C=Cdim, out_dev=_p(out),
                               out_stride_elems=out.stride(0) if n > 1 else Cdim)
    if residual is not None:
        R = residual.size(0)
        d.r_elem, d.r_dev, d.r_rows = _ELEM[residual.dtype], _p(residual), R
        d.r_stride_elems = residual.stride(0) if R > 1 else Cdim
        d.r_row0, d.r_ids_dev = (-1, _p(row_ids)) if row_ids is not None else (row0, None)
    if n:
        with torch.cuda.device(z.device):
            nat.check(nat.load().spp_resinc_epilogue(C.byref(d), _stream()))
    return out


def _check_vector(what, name, t, dtype, n):
    """a caller-provided output of ``classify_rows``: a contiguous 1-D ``dtype`` tensor of n entries, no gradient"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,) or not t.is_contiguous() \
            or t.requires_grad:
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor of shape [{n}] (one entry per row of z) "
                         "that does not require grad")


def classify_rows(z, y=None, *, row0=None, row_ids=None, pred=None, nll=None):
    """The predicted class and the negative log-likelihood of every row of logits, one pass over ``z`` and no
    [n, C] intermediate (``spp_classify_rows``, include/spp.h).  Returns ``(pred, nll)``:

        pred[i] = torch.argmax(z[i].float())                  exactly: smallest index on ties, the first NaN wins
        nll[i]  = logsumexp(z[i]) - z[i, y[row(i)]]           fp32; 0.0 where row i has no label in [0, C)

    ``z`` [n, C]: fp32 / bf16, possibly a strided view (the rows of a GEMM tile).  ``y``: contiguous int64 [R], read in
    place either as a slab, ``row0`` (row(i) = row0 + i), or by a list, ``row_ids`` (int64 [n], any order, duplicates
    allowed); an index outside [0, R) and a label outside [0, C) (-1: unlabelled) both mean "no label".  Without ``y``
    only ``pred`` is computed and ``nll`` is None.  ``pred`` (int64 [n]) / ``nll`` (fp32 [n]): contiguous vectors to write
    into (slices of longer ones allowed); allocated when None.  A row's two results are the same bits wherever the row
    stands in ``z``, whatever the stride, and from run to run.  |nll - exact| <= (C + 8) * 2^-24 * (1 + |z_y - max| +
    log C).

    Forward only: no autograd node is registered and an input that requires grad is refused.  Nothing here waits for the
    device."""
    what = "classify_rows"
    _check_matrix(z, what, "z")
    if z.dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: z must be fp32 or bf16, got {z.dtype}")
    n, Cdim = z.shape
    if Cdim < 1:
        raise ValueError(f"{what}: z needs at least one column, got {tuple(z.shape)}")
    if y is None:
        if row0 is not None or row_ids is not None:
            raise ValueError(f"{what}: row0 / row_ids address the labels y, and there is no y")
        if nll is not None:
            raise ValueError(f"{what}: nll needs the labels y")
    else:
        if not isinstance(y, torch.Tensor):
            raise TypeError(f"{what}: y must be a torch.Tensor, got {type(y).__name__}")
        if y.dtype != torch.int64 or y.dim() != 1 or not y.is_contiguous():
            raise ValueError(f"{what}: y must be a contiguous 1-D int64 tensor, got {tuple(y.shape)} {y.dtype}")
        row0 = _check_row_address(what, "the labels y", n, row0, row_ids)
    if pred is not None:
        _check_vector(what, "pred", pred, torch.int64, n)
    if nll is not None:
        _check_vector(what, "nll", nll, torch.float32, n)
    nat.require_device()
    if not all(t.is_cuda and t.device == z.device for t in (z, y, row_ids, pred, nll) if t is not None):
        raise ValueError(f"{what}: z, y, row_ids, pred and nll must live on one CUDA device")
    if pred is None:
        pred = torch.empty(n, dtype=torch.int64, device=z.device)
    if nll is None and y is not None:
        nll = torch.empty(n, dtype=torch.float32, device=z.device)
    d = nat.ClassifyDesc(z_elem=_ELEM[z.dtype], z_dev=_p(z), z_stride_elems=z.stride(0) if n > 1 else Cdim, n=n, C=Cdim,
                         y_row0=-1, pred_dev=_p(pred), nll_dev=_p(nll))
    if y is not None:
        d.y_dev, d.y_rows = _p(y), y.numel()
        d.y_row0, d.row_ids_dev = (-1, _p(row_ids)) if row_ids is not None else (row0, None)
    if n:
        with torch.cuda.device(z.device):
            nat.check(nat.load().spp_classify_rows(C.byref(d), _stream()))
    return pred, nll


_GEMM_ROWS = 1 << 16


def _row_tiles(A):
    """(first row, rows, tile) over A in tiles of exactly _GEMM_ROWS rows, the last one zero-padded.  The library picks
    a GEMM kernel -- and with it the order of the sum over K -- by the problem's shape, so the same operand row can
    come out with different last bits from a [600, K] and a [75, K] product.  With one shape for every call a node's
    result depends on its own row alone: not on the slab size, and not on whether ``nodes`` selected it.  The tiles of an
    ``Fp8Table`` (or of ``table[ids]``) are fp32, straight from ``spp_fp8_rows_f32``: the same shape, the same zero
    padding and exactly the values of the table dequantised to fp32."""
    T = A.size(0)
    for r in range(0, T, _GEMM_ROWS):
        n = min(_GEMM_ROWS, T - r)
        if isinstance(A, Fp8Table):
            tile = (torch.empty if n == _GEMM_ROWS else torch.zeros)((_GEMM_ROWS, A.size(1)), dtype=torch.float32,
                                                                      device=A.device)
            A.rows_f32(tile[:n], r)
            yield r, n, tile
            continue
        tile = A[r:r + n]
        if n < _GEMM_ROWS:
            tile = A.new_zeros((_GEMM_ROWS, A.size(1)))
            tile[:n] = A[r:r + n]
        yield r, n, tile


def _tiles_contiguous(A):
    """``_row_tiles`` with every tile contiguous: a full tile of a padded buffer is a strided view, and the GEMM's
    operand layout is part of its shape (the resident matrices the drivers allocate are contiguous)"""
    for r, n, tile in _row_tiles(A):
        yield r, n, tile.contiguous()


# ---- where the table lives: the two placements the drivers below are written against --------------------------------
class _Resident:
    """One rank owns the rows [0, N) of one matrix ``x``: the whole-table kernels, every layer in a matrix of its own
    that is dropped when the next layer is complete, nothing to publish and nothing to wait for at a layer boundary.
    ``x`` may be an ``Fp8Table``: layer 0's ``aggregate`` goes to the fp8 entry (``_agg_launch``), ``_row_tiles(x)`` and
    ``_row_tiles(x[ids])`` are fp32 tiles, and every later layer reads activations as before."""
    lo = 0
    head_tiles = staticmethod(_row_tiles)                 # the tiles of a block of SAGEResInception's head, as they are

    def __init__(self, x, rowptr, col, edge_weight=None):
        self.x, self.rowptr, self.col, self.edge_weight = x, rowptr, col, edge_weight      # (edge_weight: GCN only)
        self.n_local, self.dev = x.size(0), x.device

    def bind(self):
        pass

    abort = close = boundary = bind

    def local(self, ids):
        """global ids as rows of the rank's own matrices"""
        return ids

    def open(self, n_bufs, width, dtype):
        pass

    open_gat = open

    def layer_rows(self, i, last, rows, width, dtype):
        """where layer i's rows go: [rows, width], read back as ``cur`` (and as the residual) by layer i + 1"""
        return torch.empty((rows, width), dtype=dtype, device=self.dev)

    def aggregate(self, i, cur, epilogue, self_scale, s, ids, T, out, ws, graph=None):
        """layer i's input ``cur`` aggregated for the rank's local slab [s, s + T), or for the global ``ids``; over
        ``graph`` = (rowptr, col) whose ids are rows of ``cur`` when the layer's plan names one (a receptive field's)"""
        rowptr, col = graph or (self.rowptr, self.col)
        return _agg_launch(cur, rowptr, col, epilogue, self_scale, -1 if ids is not None else s, ids, T, out, ws)

    def aggregate_weighted(self, cur, dinv, fill, s, ids, T, out, ws):
        """GCN: ``cur`` summed with the placement's edge weights (ones without) for the slab [s, s + T) or the global
        ``ids``; with ``dinv`` the kernel forms gcn_norm's coefficients and the self term from it and ``fill``"""
        return _agg_weighted_launch(cur, self.rowptr, self.col, self.edge_weight, dinv, fill, None,
                                    -1 if ids is not None else s, ids, T, out, ws)

    def gat_rows(self, rows, H, Cc, dtype):
        """(h, logits) of a GAT layer over ``rows`` input rows: the projected rows [rows, H * Cc] and where
        ``put_logits`` writes"""
        h = torch.empty((rows, H * Cc), dtype=dtype, device=self.dev)
        return h, tuple(torch.empty((rows, H), dtype=torch.float32, device=self.dev) for _ in range(2))

    def put_logits(self, logits, r, n, a):
        H = a.size(1) // 2
        logits[0][r:r + n], logits[1][r:r + n] = a[:n, :H], a[:n, H:]

    def attend(self, h, logits, conv, relu, s, ids, T, out, ws, graph=None):
        rowptr, col = graph or (self.rowptr, self.col)
        return _gat_launch(h, logits[0], logits[1], rowptr, col, conv.heads, conv.negative_slope, relu,
                           -1 if ids is not None else s, ids, T, out, ws)


class _Partitioned:
    """Rank ``rank`` owns the rows [off[rank], off[rank + 1]) and reads the others' through ``peers``: the parts kernels
    over buffers that are allocated up front, laid out by the resident tables' row-stride rule (one stride on every rank
    whatever its row count: a one-row part has no stride of its own) and published once.  A layer boundary is a
    synchronise of the rank's stream and a barrier: what was written is complete before any rank reads it, and every rank
    has finished reading a buffer before it is written again (after the last layer: before anyone unmaps)."""
    head_tiles = staticmethod(_tiles_contiguous)          # a full tile of a padded buffer is strided: the GEMM gets a copy

    def __init__(self, what, x_local, rowptr, col, off, rank, peers):
        self.what, self.x, self.rowptr, self.col, self.off, self.rank, self.peers = what, x_local, rowptr, col, off, rank, peers
        self.lo, self.n_local, self.dev = off[rank], off[rank + 1] - off[rank], x_local.device
        self.shared = []

    def bind(self):
        if hasattr(self.peers, "bind"):
            self.peers.bind(self.rank)

    def abort(self):
        if hasattr(self.peers, "abort"):
            self.peers.abort()

    def close(self):
        for sh in self.shared:
            sh.close()

    def boundary(self):
        torch.cuda.current_stream(self.dev).synchronize()
        self.peers.barrier()

    def local(self, ids):
        return ids - self.lo

    def _buffer(self, width, dtype):
        stride = _row_stride_elems(width, torch.empty(0, dtype=dtype).element_size())
        return torch.empty((self.n_local, stride), dtype=dtype, device=self.dev)[:, :width]

    def _share(self, t, name="part"):
        """publish t (collective); its parts as the launch functions take them"""
        self.shared.append(self.peers.share(t))
        return _parts_source(self.shared[-1], self.off, t.dtype, t.size(1), self.what, name)[:4]

    def open(self, n_bufs, width, dtype):
        """SAGE, GIN, SAGEResInception: the table and the ping-pong activation buffers [n_local, width]"""
        self.bufs = [self._buffer(width, dtype) for _ in range(n_bufs)]
        self.sources = [self._share(t) for t in [self.x] + self.bufs]

    def layer_rows(self, i, last, rows, width, dtype):
        return torch.empty((rows, width), dtype=dtype, device=self.dev) if last else self.bufs[i % len(self.bufs)]

    def aggregate(self, i, cur, epilogue, self_scale, s, ids, T, out, ws, graph=None):
        src = self.sources[0] if i == 0 else self.sources[1 + (i - 1) % len(self.bufs)]      # (``cur``, as published)
        return _agg_parts_launch(src, self.off, self.rowptr, self.col, epilogue, self_scale,
                                 -1 if ids is not None else self.lo + s, ids, T, out, ws)

    def open_gat(self, Fmax, Hmax, dtype):
        """GAT: h [n_local, max H * C] and the logits [n_local, 2 * max H] fp32 = [a_src | a_dst]; a layer narrower than
        a buffer reads its leading columns at the buffer's stride.  Projection is local: the table is not published."""
        self.hbuf, self.abuf = self._buffer(Fmax, dtype), self._buffer(2 * Hmax, torch.float32)
        self.h_src, self.a_src = self._share(self.hbuf), self._share(self.abuf, "logits part")

    def gat_rows(self, rows, H, Cc, dtype):
        return self.hbuf[:, :H * Cc], self.abuf[:, :2 * H]

    def put_logits(self, logits, r, n, a):
        logits[r:r + n] = a[:n]

    def attend(self, h, logits, conv, relu, s, ids, T, out, ws, graph=None):
        return _gat_parts_launch(self.h_src[:2] + (h.dtype, h.size(1)), self.a_src[:2], self.off, self.rowptr, self.col,
                                 conv.heads, conv.negative_slope, relu, -1 if ids is not None else self.lo + s, ids, T,
                                 out, ws)


# ---- where the last layer's logits go: the two tails the drivers below end in ---------------------------------------
class _LogProbs:
    """fp32 log-probabilities, [rows, classes]: ``log_softmax(dtype=float32)`` per tile, copied into the matrix that
    ``layerwise_inference`` and ``partitioned_inference`` return"""

    def open(self, place, rows, classes):
        self.out = torch.empty((rows, classes), dtype=torch.float32, device=place.dev)

    def put(self, r, n, logits, ids):
        """output rows [r, r + n) from the first n rows of ``logits`` (fp32 / bf16); ``ids``: their global ids when the
        call scores ``nodes``, None when they are the rank's rows r .. r + n"""
        self.out[r:r + n] = torch.log_softmax(logits, dim=-1, dtype=torch.float32)[:n]

    def result(self):
        return self.out


class _Classify:
    """``classify_rows`` per tile, straight into pred [rows] and nll [rows]: nothing of [rows, classes] exists.  ``y``:
    the rank's labels by local id, or None"""

    def __init__(self, y):
        self.y = y

    def open(self, place, rows, classes):
        self.place, self.classes = place, classes
        self.pred = torch.empty(rows, dtype=torch.int64, device=place.dev)
        self.nll = torch.empty(rows, dtype=torch.float32, device=place.dev) if self.y is not None else None

    def put(self, r, n, logits, ids):
        if self.y is None:
            classify_rows(logits[:n], pred=self.pred[r:r + n])
        elif ids is None:
            classify_rows(logits[:n], self.y, row0=r, pred=self.pred[r:r + n], nll=self.nll[r:r + n])
        else:
            classify_rows(logits[:n], self.y, row_ids=self.place.local(ids), pred=self.pred[r:r + n],
                          nll=self.nll[r:r + n])

    def result(self):
        return self


class Evaluation:
    """What ``evaluate`` and ``partitioned_evaluate`` return.  ``pred`` int64 [rows] and ``nll`` fp32 [rows] (None
    without labels) stay on the device, in the order of the rows scored.  With labels: ``labelled`` (rows whose label
    lies in [0, classes)), ``correct`` (labelled rows with pred == label) and ``loss`` (the mean nll over the labelled
    rows, summed in float64 from ``nll``; nan when there are none) as Python numbers, and ``splits``: the same three per
    split name, as {name: {"labelled", "correct", "loss"}} (empty without ``splits=``).  ``accuracy`` is correct /
    labelled."""

    def __init__(self, pred, nll, labelled=None, correct=None, loss=None, splits=None):
        self.pred, self.nll, self.labelled, self.correct, self.loss = pred, nll, labelled, correct, loss
        self.splits = splits or {}

    @property
    def accuracy(self):
        return self.correct / self.labelled if self.labelled else float("nan")

    def __repr__(self):
        return (f"Evaluation(rows={self.pred.numel()}, labelled={self.labelled}, correct={self.correct}, "
                f"loss={self.loss}, splits={self.splits})")


def _evaluation(sink, y, label_rows, segments):
    """the counts of a finished ``_Classify``: ``label_rows`` are the scored rows' indices into ``y`` (None: the rows
    0 .. rows of y in order), ``segments`` {name: (first, end)} the splits' ranges of the scored rows.  Everything is
    reduced on the device and read back ONCE, as one float64 vector (counts below 2^53 are exact in it)."""
    pred, nll = sink.pred, sink.nll
    if y is None:
        return Evaluation(pred, None)
    yv = y if label_rows is None else y[label_rows]
    labelled = (yv >= 0) & (yv < sink.classes)
    correct = labelled & (pred == yv)
    nll64 = nll.to(torch.float64)                        # (0.0 on the unlabelled rows: the sums are over the labelled)
    ranges = [(0, pred.numel())] + list(segments.values())
    stats = torch.stack([torch.stack([labelled[a:b].sum().to(torch.float64), correct[a:b].sum().to(torch.float64),
                                      nll64[a:b].sum()]) for a, b in ranges]).cpu().tolist()
    rec = [dict(labelled=int(l), correct=int(c), loss=t / l if l else float("nan")) for l, c, t in stats]
    return Evaluation(pred, nll, splits=dict(zip(segments, rec[1:])), **rec[0])


# ---- the drivers: one layer loop per model, over a placement ---------------------------------------------------------
def _sage_layer(model, place, act_dtype):
    """SAGE's layers for ``_conv_layers``.  Every recipe returns ``layer(i, last)`` -> (aggregate, wide, fn, classes):
    ``aggregate(cur, s, ids, T, A, ws, graph)`` fills a slab's operand A [T, wide * K] from the layer's input ``cur``
    [n, K] through the placement, ``fn`` maps a fixed tile of A to the layer's output rows -- on the last layer the
    logits, ``classes`` wide"""
    def layer(i, last):
        conv = model.convs[i]
        W = torch.cat([conv.lin_l.weight, conv.lin_r.weight], dim=1).to(act_dtype)      # [N, 2K] = [W_l | W_r]
        bias = conv.lin_l.bias
        epilogue = "max_operand" if getattr(conv, "aggr", "mean") == "max" else "operand"

        def fn(A):
            Z = A @ W.t()
            if bias is not None:
                Z = Z + bias.to(Z.dtype)
            return Z if last else torch.relu_(Z)         # the inter-layer ReLU; dropout is the identity in eval mode
        return (lambda cur, *slab: place.aggregate(i, cur, epilogue, 0.0, *slab)), 2, fn, conv.lin_l.out_features
    return layer


def _gin_layer(model, place, act_dtype):
    amp = act_dtype == torch.bfloat16

    def layer(i, last):
        conv = model.convs[i]
        scale = conv._scale()

        def fn(h):
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                h = conv.nn(h)                           # Linear, BatchNorm1d (running statistics), ReLU, Linear, ReLU
            if last:                                     # what follows the last conv layer: the logits
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                    h = model.lin2(torch.relu(model.lin1(h)))
            return h
        return (lambda cur, *slab: place.aggregate(i, cur, "sum", scale, *slab)), 1, fn, model.lin2.out_features
    return layer


def _gcn_layer(model, place, act_dtype):
    """GCN over one resident matrix (f3s), in ``GCNConv.forward``'s order -- aggregate first, project second:

      aggregate  ``spp_graph_agg_weighted_forward`` over each node's whole row of the layer's input, [T, K] in
                 ``act_dtype``.  ``normalize=False`` (the reference's model): the entries weigh ``edge_weight`` (ones
                 without), no self term.  ``normalize=True``: PyG's gcn_norm of the whole graph, formed IN the kernel from
                 ``dinv`` = ``gcn_dinv(rowptr, edge_weight)`` -- fp32 [N], computed once per call and ``fill`` -- with
                 the self term ``fill * dinv[t]^2``.
      project    tile @ lin.weight^T (+ bias) over the fixed row tiles
      tail       every layer but the last: relu(BatchNorm) on the running statistics, under bf16 autocast when
                 ``act_dtype`` is bf16 (as GIN's ``conv.nn``); dropout is the identity.  The last layer's logits go to
                 the sink untouched.

    Memory, as arithmetic: two [N, hidden] matrices of ``act_dtype`` at a layer boundary, as for SAGE, plus a slab's
    [rows_per_slab, K] aggregate and, with ``normalize=True``, ``dinv``: 4 * N bytes (0.44 GB at N = 111 M).  NO [E]
    array is allocated on either path: the coefficients PyG would materialise are 4 * E bytes (12.8 GB at E = 3.2 G),
    and so are the ones of a valueless ``adj_t``; a caller's ``edge_weight`` is read in place."""
    amp = act_dtype == torch.bfloat16
    dinvs = {}                                           # fill -> dinv [N]: once per call (the convs share one setting)

    def layer(i, last):
        conv, bn = model.convs[i], model.bns[i]
        dinv, fill = None, 0
        if conv.normalize:
            fill = _gcn_fill(conv.add_self_loops, conv.improved)
            if fill not in dinvs:
                dinvs[fill] = gcn_dinv(place.rowptr, place.edge_weight, add_self_loops=conv.add_self_loops,
                                       improved=conv.improved)
            dinv = dinvs[fill]
        Wt = conv.lin.weight.to(act_dtype).t()
        bias = conv.bias.to(act_dtype) if conv.bias is not None else None

        def fn(tile):
            Z = torch.addmm(bias, tile, Wt) if bias is not None else tile @ Wt
            if last:
                return Z
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                return torch.relu(bn(Z))                 # (eval mode: the running statistics)
        return (lambda cur, s, ids, T, A, ws, _graph: place.aggregate_weighted(cur, dinv, fill, s, ids, T, A, ws)), 1, \
            fn, conv.lin.out_features
    return layer


def _slabs(rows, ids, rows_per_slab):
    """(first row, rows, the slab's ids or None) over the rows [0, rows), or over the ``rows`` entries of ``ids``"""
    for s in range(0, rows, rows_per_slab):
        e = min(rows, s + rows_per_slab)
        yield s, e - s, ids[s:e] if ids is not None else None


class _Step:
    """One conv layer of a plan: the layer computes ``rows`` output rows -- the targets ``ids`` (a list) or, with None,
    the slab [0, rows) -- over ``graph`` = (rowptr, col), None for the placement's own.  ``names``: the output rows'
    global ids as the sink of the last layer wants them, None when they are the rank's rows 0 .. rows in order."""

    def __init__(self, rows, ids=None, graph=None, names=None):
        self.rows, self.ids, self.graph, self.names = rows, ids, graph, names


def _whole_graph_plan(place, nodes, n_layers):
    """the plan of the whole-graph entries: every layer for all the rank's rows over the placement's graph, the last one
    for ``nodes`` only when they are given"""
    last = _Step(place.n_local) if nodes is None else _Step(nodes.numel(), ids=nodes, names=nodes)
    return [_Step(place.n_local) for _ in range(n_layers - 1)] + [last]


def _field_plan(field, n_layers):
    """the plan of ``field_inference`` over a field of h = n_layers - 1 hops: layer 0 reads the table in place over the
    ORIGINAL graph, for every node of the field (``target_ids=field.ids``); layer i >= 1 runs on the field's CSR as the
    slab [0, sizes[h - i]) and reads layer i - 1's rows, which are the slots below sizes[h - i + 1] that its rows name;
    the last layer leaves the distinct nodes' rows, which the sink labels by their global ids"""
    h = n_layers - 1
    if field.hops != h:
        raise ValueError(f"a model of {n_layers} conv layers is scored over a field of {h} hops, got one of {field.hops}")
    graph = (field.rowptr, field.col)
    steps = [_Step(field.sizes[h], ids=field.ids)] + [_Step(field.sizes[h - i], graph=graph) for i in range(1, n_layers)]
    steps[-1].names = field.ids[:field.sizes[0]]
    return steps


def _conv_layers(model, place, nodes, rows_per_slab, act_dtype, sink, plan=None):
    """SAGE, GIN and GCN (``_sage_layer``, ``_gin_layer``, ``_gcn_layer``: what a layer aggregates and what follows), as
    ``layerwise_inference`` describes them; the last layer's logits go to ``sink``, tile by tile.  Resident, layer i-1's
    matrix is dropped as soon as layer i is complete, so two [N, hidden] matrices are live at a boundary; partitioned,
    the layers alternate between the (at most two) published buffers.  ``plan``: one ``_Step`` a layer (rows, targets
    and graph); None is ``_whole_graph_plan``."""
    recipe = _gin_layer if isinstance(model, GIN) else _gcn_layer if isinstance(model, GCN) else _sage_layer
    layer = recipe(model, place, act_dtype)
    n_layers, dev = len(model.convs), place.dev
    plan = plan or _whole_graph_plan(place, nodes, n_layers)
    place.open(min(2, n_layers - 1), model.hidden_channels, act_dtype)
    ws = torch.empty(graph_agg_workspace_bytes(min(rows_per_slab, max([place.n_local] + [st.rows for st in plan]))),
                     dtype=torch.uint8, device=dev)
    cur = place.x
    for i, step in enumerate(plan):
        last = i == n_layers - 1
        aggregate, wide, fn, classes = layer(i, last)
        rows, names = step.rows, step.names
        nxt = None
        if last:
            sink.open(place, rows, classes)
        for s, T, tids in _slabs(rows, step.ids, rows_per_slab):
            A = torch.empty((T, cur.size(1) * wide), dtype=act_dtype, device=dev)
            aggregate(cur, s, tids, T, A, ws, step.graph)
            for r, n, tile in _row_tiles(A):
                h = fn(tile)
                if last:
                    sink.put(s + r, n, h, names[s + r:s + r + n] if names is not None else None)
                    continue
                if nxt is None:
                    nxt = place.layer_rows(i, last, rows, h.size(1), act_dtype)
                nxt[s + r:s + r + n] = h[:n]
        if nxt is None and not last:                     # no rows at all
            nxt = place.layer_rows(i, last, 0, model.hidden_channels, act_dtype)
        cur = nxt                                        # (resident: drops layer i-1's matrix)
        place.boundary()
    return sink.result()


def _gat_layer(model, place, act_dtype):
    """GAT's layers for ``_attn_layers``, in PyG's project-first order (training aggregates first, _GatLayer /
    _GatLayerMH, because an MFG hop has many sources per target; over the whole graph T = S = N, that saving is gone,
    and the aggregate-first intermediate would be [T, H, K] fp32 per slab):

      project    h = cur @ W^T for all the rank's rows, [n, H*C] in ``act_dtype``
      logits     [a_src | a_dst] = tile.float() @ V^T with V = W_h^T att (as _GatLayerMH builds it), fp32 [n, H] each:
                 taken from the layer's input rows, never from the rounded h
      attend     ``place.attend``: ``spp_graph_gat_forward``; partitioned, the parts kernel over h and the logits, the
                 two published buffers.  Projection and logits are LOCAL: no rank reads a peer's feature rows.

    Memory, as arithmetic (resident): ``cur`` is dropped once ``h`` is complete and ``h`` once ``nxt`` is, so two
    [N, hidden] matrices of ``act_dtype`` are live at a time, as for SAGE (57 GB each in bf16 at N = 111 M, hidden 256;
    layer 1's ``cur`` is the resident table and stays), plus the logits, 2 * N * H * 4 bytes (3.6 GB at H = 4).  The one
    case worse than SAGE: the last layer's h is [N, H * classes], so H > 1 heads multiply it -- 111 M * 4 * 172 * 2 bytes
    = 153 GB in bf16 for H = 4 and 172 classes, which does not fit next to a 57 GB ``cur``, 26 GB of graph and 28 GB of
    features on one 288 GB MI355X.  The reference's model has H = 1 (38 GB).  Partitioned: ``partitioned_inference``."""
    place.open_gat(max(c.heads * c.out_channels for c in model.convs), max(c.heads for c in model.convs), act_dtype)

    def layer(i):
        conv = model.convs[i]
        H, Cc, W = conv.heads, conv.out_channels, conv.lin_src.weight             # W: [H*C, K]
        att = torch.stack([conv.att_src.view(H, Cc), conv.att_dst.view(H, Cc)]).to(torch.float32)
        V = torch.einsum("shc,hck->shk", att, W.to(torch.float32).view(H, Cc, -1)).reshape(2 * H, -1)   # [V_src; V_dst]
        Wt, Vt = W.to(act_dtype).t(), V.t().contiguous()

        def project(cur):
            h, logits = place.gat_rows(cur.size(0), H, Cc, act_dtype)
            for r, n, tile in _row_tiles(cur):
                h[r:r + n] = (tile.to(act_dtype) @ Wt)[:n]
                place.put_logits(logits, r, n, tile.to(torch.float32) @ Vt)
            return h, logits
        return H, Cc, Cc, project, lambda operands, *slab: place.attend(*operands, conv, *slab)
    return graph_gat_workspace_bytes, layer


def _gatv2_layer(model, place, act_dtype):
    """GATv2 over one resident matrix (f3w), project-first as ``GATv2Conv.forward``:

      project    x_l = cur @ W_l^T and x_r = cur @ W_r^T for all rows, [n, H*Cp] each in ``act_dtype``; with
                 ``share_weights`` x_r IS x_l and no second GEMM runs
      attend     ``spp_graph_gatv2_forward`` (``_gatv2_launch``) over the step's graph or the placement's

    Channel padding: the kernels take C % 4 == 0 with C / 4 a power of two, and a last layer has C = classes (47, 172).
    Cp is the next such width (48 -> 64, 172 -> 256): W_l / W_r get Cp - C zero rows per head and att Cp - C zero
    columns, and the driver slices the padded output columns away.  The padding is exact: a padded channel has
    x_l = x_r = 0, so its term of every logit is att * lrelu(0 + 0) = 0 * 0 = +0, added to a dot product -- and its
    position in the butterfly is fixed by (H, Cp), the same for every entry.

    Memory, as arithmetic: ``cur`` is dropped once x_l and x_r are complete (``_attn_layers``), so at the worst moment
    THREE [N, hidden] matrices of ``act_dtype`` are live (cur, x_l, x_r while projecting, with two GEMM tiles of 65 536
    rows on top; then x_l, x_r and nxt): at N = 111 M and hidden 256, 57 GB each in bf16, next to 26 GB of graph and
    28 GB of features: 3 * 57 + 26 + 28 = 225 GB of one 288 GB MI355X.  With ``share_weights`` two are live
    (2 * 57 + 26 + 28 = 168 GB, as SAGE).  The one case worse: the last layer's x_l and x_r are [N, H * Cp] -- for H = 4
    and 172 classes (Cp = 256) 111 M * 4 * 256 * 2 bytes = 227 GB EACH in bf16, which does not fit next to anything;
    H = 1 is 57 GB each (2 * 57 + 57 of ``cur`` + 26 + 28 = 225 GB; 168 GB shared).  A multi-head model of many classes
    at that scale needs ``share_weights`` and fewer heads, or several devices (not built for GATv2)."""
    def layer(i):
        conv = model.convs[i]
        H, Cc, Cp = conv.heads, conv.out_channels, _gatv2_pad(conv.out_channels)

        def padded_t(W):                                 # [H*C, K] -> [K, H*Cp] in act_dtype, zero rows behind each head's C
            if Cp != Cc:
                Wp = W.new_zeros((H, Cp, W.size(1)))
                Wp[:, :Cc] = W.view(H, Cc, -1)
                W = Wp.view(H * Cp, -1)
            return W.to(act_dtype).t()
        shared = conv.lin_r is conv.lin_l
        Wl, Wr = padded_t(conv.lin_l.weight), None if shared else padded_t(conv.lin_r.weight)
        att = torch.zeros((H, Cp), dtype=torch.float32, device=place.dev)
        att[:, :Cc] = conv.att.view(H, Cc)

        def project(cur):
            x_l = torch.empty((cur.size(0), H * Cp), dtype=act_dtype, device=place.dev)
            x_r = x_l if shared else torch.empty_like(x_l)
            for r, n, tile in _row_tiles(cur):
                tile = tile.to(act_dtype)
                x_l[r:r + n] = (tile @ Wl)[:n]
                if not shared:
                    x_r[r:r + n] = (tile @ Wr)[:n]
            return x_l, x_r

        def attend(operands, relu, s, ids, T, out, ws, graph):
            return _gatv2_launch(*operands, att, *(graph or (place.rowptr, place.col)), conv.negative_slope, relu,
                                 -1 if ids is not None else s, ids, T, out, ws)
        return H, Cc, Cp, project, attend
    return graph_gatv2_workspace_bytes, layer


class _Tail:
    """What a layer of ``_attn_layers`` does behind its kernel when that is more than the fused ReLU or the mean of the
    heads (``_transformer_layer``; GAT and GATv2 have none).  ``slab_dtype``: the dtype of a hidden layer's slab.
    ``nxt(operands, rows, ids)``: the matrix the hidden layer's rows go into when the recipe already holds it (the
    projected skip, which the kernel reads and overwrites row by row), or None.  ``hidden(h, operands, s, T, ids)``:
    None when the kernel's rows are the layer's output, else [T, H * Cc] of the slab's dtype -> the layer's output rows.
    ``last(z, operands, s, T, ids)``: the mean of the heads [T, Cc] fp32 -> the logits."""

    def __init__(self, slab_dtype, nxt, hidden, last):
        self.slab_dtype, self.nxt, self.hidden, self.last = slab_dtype, nxt, hidden, last


def _transformer_layer(model, place, act_dtype):
    """GraphTransformer over one resident matrix (f3z), project-first as ``TransformerConv.forward``:

      project    over ``_row_tiles(cur)``, biases included, all in ``act_dtype``: q = lin_query(cur) [n, H*Cp],
                 [k | v] = ONE [n, 2*H*Cp] matrix from one GEMM (lin_key's and lin_value's weights stacked), and with
                 ``root_weight`` skip = lin_skip(cur)
      attend     ``spp_graph_transformer_forward`` (``_transformer_launch``) over the step's graph or the placement's,
                 scale = 1 / sqrt(Cc) from the UNPADDED width

    Channel padding is ``_gatv2_pad``'s: Cp - Cc zero weight rows and zero bias entries per head, so a padded channel
    has q = k = v = 0, adds a product 0 * 0 = +0 to every logit at a position fixed by (H, Cp), and is a zero column of
    the output that the driver slices away.

    Hidden layers, ``beta=False``: the kernel adds the skip row and applies the ReLU, and writes the next activation
    matrix.  With Cp == Cc and ``root_weight`` the skip is projected INTO that matrix and the kernel reads and overwrites
    it in place (spp.h f3z, aliasing); with Cp != Cc the skip is padded like q and the leading columns of a slab are
    copied; without ``root_weight`` there is no skip anywhere.  ``beta=True``: the kernel writes the bare attention as an
    fp32 slab, and b = sigmoid(lin_beta([out, x_r, out - x_r])), b x_r + (1 - b) out and the ReLU are plain torch per
    slab, in fp32 (lin_beta's GEMM over ``_row_tiles``, so that a row's bits do not depend on the slab).  Last layer
    (concat=False): an fp32 slab, the leading Cc columns, the mean of the heads, then the [rows, Cc] skip (gathered by
    ``nodes`` when they are given) added or gated in torch.

    Memory, as arithmetic: ``cur``, q, [k | v] (two matrices' worth) and skip (which becomes ``nxt``) are FIVE
    [N, hidden] matrices of ``act_dtype`` at the end of the projection, with the GEMM tiles of 65 536 rows on top, and
    four while attending (``cur`` is dropped).  At N = 111 M and hidden 256 a matrix is 57 GB in bf16, next to 26 GB of
    graph and 28 GB of features: 5 * 57 + 26 + 28 = 339 GB.  That does NOT fit one 288 GB MI355X; a GraphTransformer of
    hidden 256 cannot be scored at papers scale on one device by this driver (hidden 128: 5 * 28 + 54 = 196 GB does).
    The follow-up that would bring it to four matrices (4 * 57 + 54 = 282 GB) is projecting q and skip per slab, next
    to the kernel's launch, instead of for all rows up front; it is not built.  With ``beta`` the skip is a matrix of
    its own next to ``nxt`` while attending (five there too)."""
    def layer(i):
        conv = model.convs[i]
        H, Cc, Cp = conv.heads, conv.out_channels, _gatv2_pad(conv.out_channels)
        last = i == len(model.convs) - 1
        fused = not last and conv.lin_skip is not None and conv.lin_beta is None    # the skip rides in the kernel
        scale = 1.0 / float(Cc) ** 0.5

        def padded(lin):                                 # [H*C, K], [H*C] -> ([K, H*Cp], [H*Cp]) in act_dtype
            W = lin.weight
            b = lin.bias if lin.bias is not None else W.new_zeros(W.size(0))
            if Cp != Cc:
                Wp, bp = W.new_zeros((H, Cp, W.size(1))), b.new_zeros((H, Cp))
                Wp[:, :Cc], bp[:, :Cc] = W.view(H, Cc, -1), b.view(H, Cc)
                W, b = Wp.view(H * Cp, -1), bp.view(H * Cp)
            return W.to(act_dtype).t(), b.to(act_dtype)
        Wq, bq = padded(conv.lin_query)
        (Wk, bk), (Wv, bv) = padded(conv.lin_key), padded(conv.lin_value)
        Wkv, bkv = torch.cat([Wk, Wv], 1).contiguous(), torch.cat([bk, bv])
        Ws = bs = None
        if conv.lin_skip is not None:
            if fused:
                Ws, bs = padded(conv.lin_skip)
            else:                                        # added in torch: the layer's own width, unpadded
                Ws = conv.lin_skip.weight.to(act_dtype).t()
                bs = conv.lin_skip.bias.to(act_dtype) if conv.lin_skip.bias is not None else None
        Wb = conv.lin_beta.weight.to(torch.float32).t().contiguous() if conv.lin_beta is not None else None

        def project(cur):
            n_rows = cur.size(0)
            q = torch.empty((n_rows, H * Cp), dtype=act_dtype, device=place.dev)
            kv = torch.empty((n_rows, 2 * H * Cp), dtype=act_dtype, device=place.dev)
            skip = torch.empty((n_rows, Ws.size(1)), dtype=act_dtype, device=place.dev) if Ws is not None else None
            for r, n, tile in _row_tiles(cur):
                tile = tile.to(act_dtype)
                q[r:r + n] = torch.addmm(bq, tile, Wq)[:n]          # (one product live at a time)
                kv[r:r + n] = torch.addmm(bkv, tile, Wkv)[:n]
                if skip is not None:
                    skip[r:r + n] = (torch.addmm(bs, tile, Ws) if bs is not None else tile @ Ws)[:n]
            return q, kv, skip

        def attend(operands, relu, s, ids, T, out, ws, graph):
            q, kv, skip = operands
            return _transformer_launch(q, kv[:, :H * Cp], kv[:, H * Cp:], skip if fused else None, H, scale,
                                       *(graph or (place.rowptr, place.col)), relu and conv.lin_beta is None,
                                       -1 if ids is not None else s, ids, T, out, ws)

        def root(out, operands, s, T, ids):              # out [T, width] fp32 -> with the root term, as the layer's forward
            skip = operands[2]
            if skip is None:
                return out
            x_r = (skip[ids] if ids is not None else skip[s:s + T]).to(torch.float32)
            if Wb is None:
                return out + x_r
            g = torch.cat([out, x_r, out - x_r], -1)
            b = torch.empty((T, 1), dtype=torch.float32, device=place.dev)
            for r, n, tile in _row_tiles(g):
                b[r:r + n] = (tile @ Wb)[:n]
            b = torch.sigmoid(b)
            return b * x_r + (1 - b) * out

        def nxt(operands, rows, ids):
            skip = operands[2]
            return skip if fused and Cp == Cc and ids is None and rows == skip.size(0) else None
        gated = conv.lin_beta is not None and not last
        tail = _Tail(torch.float32 if gated else act_dtype, nxt,
                     (lambda h, *slab: torch.relu(root(h, *slab))) if gated else None, root)
        return H, Cc, Cp, project, attend, tail
    return graph_transformer_workspace_bytes, layer


def _attn_layers(model, place, nodes, rows_per_slab, act_dtype, sink, plan=None):
    """GAT, GATv2 and GraphTransformer.  A recipe (``_gat_layer``, ``_gatv2_layer``, ``_transformer_layer``) opens the
    placement and returns (workspace_bytes, layer); ``layer(i)`` -> (H, Cc, Cp, project, attend) and, for
    GraphTransformer alone, a ``_Tail`` behind them (GAT and GATv2 run exactly the ops they ran without it): heads, channels a head, channels a head as the kernel writes
    them, ``project(cur)`` -> the projected operands of all the rank's rows, over ``_row_tiles(cur)``, and
    ``attend(operands, relu, s, ids, T, out, ws, graph)``, a slab's launch over each node's whole row.  Hidden layers go
    through the fused ReLU straight into the next [n, hidden] matrix (Cp != Cc: into a [T, H*Cp] slab whose leading
    columns are copied), the last layer ([T, H*Cp] fp32 per slab) through the mean over its heads into ``sink``.  Two
    boundaries a layer: the projected rows are complete before anyone attends, and read by everyone before the next
    layer overwrites them.  The recipes' memory arithmetic rests on ONE name each for ``cur``, the operands and ``nxt``
    and no view left behind (a tile dies with ``project``'s frame).  ``plan``: as in ``_conv_layers``."""
    recipe = _gatv2_layer if isinstance(model, GATv2) else _transformer_layer if isinstance(model, GraphTransformer) \
        else _gat_layer
    workspace_bytes, layer = recipe(model, place, act_dtype)
    n_layers, dev = len(model.convs), place.dev
    plan = plan or _whole_graph_plan(place, nodes, n_layers)
    ws = torch.empty(workspace_bytes(min(rows_per_slab, max([place.n_local] + [st.rows for st in plan]))),
                     dtype=torch.uint8, device=dev)
    cur = place.x
    for i, step in enumerate(plan):
        last = i == n_layers - 1
        H, Cc, Cp, project, attend, *tail = layer(i)
        tail = tail[0] if tail else None                 # (GraphTransformer's; None: the fused ReLU / the mean is all)
        operands = project(cur)
        del cur                                          # (layer i-1's matrix; layer 1's is the caller's table)
        place.boundary()                                 # every rank's projected rows of this layer are complete
        rows, names = step.rows, step.names
        nxt = None if last or tail is None else tail.nxt(operands, rows, step.ids)
        if nxt is None and not last:
            nxt = torch.empty((rows, H * Cc), dtype=act_dtype, device=dev)
        if last:
            sink.open(place, rows, Cc)
        # the rows go straight into the next activation matrix
        direct = not last and Cp == Cc and (tail is None or tail.hidden is None)
        slab_dtype = torch.float32 if last else act_dtype if tail is None else tail.slab_dtype
        for s, T, tids in _slabs(rows, step.ids, rows_per_slab):
            out = nxt[s:s + T] if direct else torch.empty((T, H * Cp), dtype=slab_dtype, device=dev)
            attend(operands, not last, s, tids, T, out, ws, step.graph)
            if last:                                     # concat=False: the mean of the heads (H = 1: the head itself)
                z = out.view(T, H, Cp)[:, :, :Cc]
                z = z.mean(1) if H > 1 else z.reshape(T, Cc)
                if tail is not None:
                    z = tail.last(z, operands, s, T, tids)
                sink.put(s, T, z, names[s:s + T] if names is not None else None)
            elif not direct:
                h = out.view(T, H, Cp)[:, :, :Cc].reshape(T, H * Cc)
                nxt[s:s + T] = h if tail is None or tail.hidden is None else tail.hidden(h, operands, s, T, tids)
            out = None                                   # (a hidden layer's slab is a VIEW of nxt)
        cur, nxt = nxt, None                             # ONE name holds the matrix: ``del cur`` above must free it
        del operands                                     # (resident: drops them)
        place.boundary()                                 # every rank has finished reading this layer's projected rows
    return sink.result()


def _resinc_head(model):
    """the two bare Linears of SAGEResInception's MLP head (``end_up_with_fc=True``: no BatchNorm, no activation)"""
    mods = list(model.mlp.module_list)
    if len(mods) != 2 or not all(isinstance(m, torch.nn.Linear) for m in mods):
        raise NotImplementedError("layerwise_inference: SAGEResInception's head must be exactly two Linears (its first "
                                  "one is applied block by block, which needs it to be linear in the concatenation)")
    return mods


def _resinc_layers(model, place, nodes, rows_per_slab, act_dtype, sink):
    """SAGEResInception.  In eval mode dropout is the identity and the model is

      layer i    h_i = leaky_relu(BatchNorm_i([mean | h_{i-1}] @ [W_l | W_r]^T)) + res_i,   h_0 = x,
                 res_1 = res_linears[0](x), res_i = h_{i-1} after; per slab one aggregation ("operand"), per fixed GEMM
                 tile one product and one ``resinc_epilogue`` that writes the tile's rows of the next [n, hidden] matrix.
                 Layer 1's residual Linear is stacked into the same product ([0 | W_res] below [W_l | W_r], so the tile
                 is [z | res]); later residuals are the rows of ``cur`` itself -- the rank's OWN previous matrix -- read
                 in place by local slab or, on the last layer with ``nodes``, by the local id list.
      head       lin2(lin1(cat(x, h_1, .., h_L))), handed to ``sink`` tile by tile (log_softmax, or ``classify_rows``).
                 lin1 is a bare Linear, so lin1(cat(..)) is bias + sum_k block_k @ W1[:, block k]^T: an fp32 accumulator ``acc`` [rows, 2 * classes] takes every
                 block's product when the block is complete, and no layer's matrix outlives the next layer.

    Everything behind the aggregation is local to a rank; partitioned, the table and the ping-pong [n_local, hidden]
    buffers are published, one boundary a layer.

    Memory, as arithmetic (resident): two [N, hidden] matrices of ``act_dtype`` at a layer boundary, as for SAGE, plus
    ``acc``: 4 * rows * 2 * classes bytes.  For all N = 111 M nodes and 172 classes that is 153 GB, which does not fit
    beside 2 * 57 + 26 + 28 = 168 GB on one 288 GB MI355X: ``nodes=`` is the papers-scale form."""
    lin1, lin2 = _resinc_head(model)
    x, dev = place.x, place.dev
    n_layers, hidden = len(model.convs), model.hidden_channels
    place.open(min(2, n_layers - 1), hidden, act_dtype)
    rows_out = nodes.numel() if nodes is not None else place.n_local
    local = place.local(nodes) if nodes is not None else None         # the rank's own rows of ``nodes``
    ws = torch.empty(graph_agg_workspace_bytes(min(rows_per_slab, max(place.n_local, rows_out))), dtype=torch.uint8,
                     device=dev)
    acc = torch.zeros((rows_out, lin1.out_features), dtype=torch.float32, device=dev)
    if lin1.bias is not None:
        acc += lin1.bias.to(torch.float32)

    def add_block(block, first_col):                     # acc += block @ W1[:, its columns]^T, over the fixed tiles
        Wb = lin1.weight[:, first_col:first_col + block.size(1)].to(act_dtype).t()
        for r, n, tile in place.head_tiles(block):
            acc[r:r + n] += (tile.to(act_dtype) @ Wb)[:n]

    add_block(x if local is None else x[local], 0)
    cur = x
    for i, (conv, bn) in enumerate(zip(model.convs, model.bns)):
        last = i == n_layers - 1
        # BatchNorm on its running statistics, folded in fp32: a = gamma / sqrt(var + eps), b = beta - mean * a
        a = bn.weight.to(torch.float32) / torch.sqrt(bn.running_var.to(torch.float32) + bn.eps)
        b = bn.bias.to(torch.float32) - bn.running_mean.to(torch.float32) * a
        W = torch.cat([conv.lin_l.weight, conv.lin_r.weight], dim=1)               # [hidden, 2K] = [W_l | W_r]
        bias = conv.lin_l.bias
        res = model.res_linears[i]
        if isinstance(res, torch.nn.Linear):             # (layer 1) stacked: the tile comes out as [z | res(x_t)]
            W = torch.cat([W, torch.cat([torch.zeros_like(res.weight), res.weight], dim=1)], dim=0)
            if bias is not None or res.bias is not None:
                zero = W.new_zeros(hidden)
                bias = torch.cat([bias if bias is not None else zero, res.bias if res.bias is not None else zero])
        Wt = W.to(act_dtype).t()
        bias = bias.to(act_dtype) if bias is not None else None
        ids = nodes if last else None
        rows = ids.numel() if ids is not None else place.n_local
        nxt = place.layer_rows(i, last, rows, hidden, act_dtype)
        for s, T, tids in _slabs(rows, ids, rows_per_slab):
            A = torch.empty((T, 2 * cur.size(1)), dtype=act_dtype, device=dev)
            place.aggregate(i, cur, "operand", 0.0, s, tids, T, A, ws)
            for r, n, tile in _row_tiles(A):
                Z = torch.addmm(bias, tile, Wt) if bias is not None else tile @ Wt
                if Z.size(1) > hidden:
                    residual = dict(residual=Z[:, hidden:], row0=0)
                elif ids is not None:
                    residual = dict(residual=cur, row_ids=local[s + r:s + r + n])
                else:
                    residual = dict(residual=cur, row0=s + r)
                resinc_epilogue(Z[:n, :hidden], a, b, negative_slope=0.01, out=nxt[s + r:s + r + n], **residual)
        add_block(nxt if last or local is None else nxt[local], x.size(1) + i * hidden)
        cur = nxt                                        # (resident: drops layer i-1's matrix)
        place.boundary()
    W2t = lin2.weight.to(act_dtype).t()
    b2 = lin2.bias.to(act_dtype) if lin2.bias is not None else None
    sink.open(place, rows_out, lin2.out_features)
    for r, n, tile in _row_tiles(acc):
        h = tile.to(act_dtype)
        h = torch.addmm(b2, h, W2t) if b2 is not None else h @ W2t
        sink.put(r, n, h[:n], nodes[r:r + n] if nodes is not None else None)
    return sink.result()


_PARTITIONED_MODELS = (SAGE, GIN, GAT, SAGEResInception)    # what an entry admits, in the order its refusal names them
_RESIDENT_MODELS = _PARTITIONED_MODELS + (GCN, GATv2)
_FIELD_MODELS = (SAGE, GIN, GAT)
_GATV2_RESIDENT = ("a GATv2 model is scored over one resident fp16 / fp32 / bf16 matrix by inference.layerwise_inference "
                   "(gatv2_inference is the same call) and inference.evaluate; an Fp8Table input, the field entries and "
                   "the partitioned entries are not built for GATv2")


_TRANSFORMER_RESIDENT = ("a GraphTransformer model is scored over one resident fp16 / fp32 / bf16 matrix by "
                         "inference.layerwise_inference (transformer_inference is the same call) and inference.evaluate; an "
                         "Fp8Table input, the field entries and the partitioned entries are not built for GraphTransformer")


def _check_gat(model, what):
    """the layers as ``models.GAT`` builds them"""
    for i, c in enumerate(model.convs):
        if c.bias is not None or c.concat == (i == len(model.convs) - 1 and c.heads > 1):
            raise NotImplementedError(f"{what}: GAT layers need bias=False, and concat=False on the last layer of a "
                                      "multi-head model only")


def _check_gatv2(model, what):
    """the layers as ``models.GATv2`` builds them, in shapes ``_gatv2_layer`` can put on the kernels"""
    for i, c in enumerate(model.convs):
        last = i == len(model.convs) - 1
        if c.bias is not None or c.lin_l.bias is not None or c.lin_r.bias is not None or c.concat == last:
            raise NotImplementedError(f"{what}: GATv2 layers need bias=False, and concat=False on the last layer only "
                                      "(as models.GATv2 builds them)")
        H, Cc, Cp = c.heads, c.out_channels, _gatv2_pad(c.out_channels)
        if H not in _GATV2_HEADS:
            raise NotImplementedError(f"{what}: layer {i} has heads = {H}; the GATv2 kernels are built for heads in "
                                      f"{{1, 2, 4, 8}} (heads * C = {H} * {Cc} is not the limit that was hit)")
        if H * Cp > _GATV2_MAX_D:
            raise NotImplementedError(f"{what}: layer {i} needs rows of heads * Cp = {H} * {Cp} = {H * Cp} columns "
                                      f"(C = {Cc} padded to Cp = {Cp}, the next multiple of 4 with Cp / 4 a power of "
                                      f"two), above the kernels' {_GATV2_MAX_D} (heads = {H} is not the limit that was hit)")


def _check_transformer(model, what):
    """the layers as ``models.GraphTransformer`` builds them, in shapes ``_transformer_layer`` can put on the kernels"""
    for i, c in enumerate(model.convs):
        last = i == len(model.convs) - 1
        if c.concat == last or c.lin_key.bias is None or c.lin_query.bias is None or c.lin_value.bias is None:
            raise NotImplementedError(f"{what}: GraphTransformer layers need concat=False on the last layer only and "
                                      "biased key / query / value projections (as models.GraphTransformer builds them)")
        H, Cc, Cp = c.heads, c.out_channels, _gatv2_pad(c.out_channels)
        if H not in _GATV2_HEADS:
            raise NotImplementedError(f"{what}: layer {i} has heads = {H}; the TransformerConv kernels are built for "
                                      f"heads in {{1, 2, 4, 8}} (heads * C = {H} * {Cc} is not the limit that was hit)")
        if H * Cp > _GATV2_MAX_D:
            raise NotImplementedError(f"{what}: layer {i} needs rows of heads * Cp = {H} * {Cp} = {H * Cp} columns "
                                      f"(C = {Cc} padded to Cp = {Cp}, the next multiple of 4 with Cp / 4 a power of "
                                      f"two), above the kernels' {_GATV2_MAX_D} (heads = {H} is not the limit that was hit)")


def _check_model(model, what, admits):
    """one of the model classes the entry admits, with what the GAT, GATv2 and SAGEResInception drivers need of its
    layers (SAGE, GIN and GCN: nothing)"""
    if isinstance(model, GraphTransformer):              # admitted next to _RESIDENT_MODELS, whose refusal keeps its wording
        if admits is not _RESIDENT_MODELS:
            raise NotImplementedError(f"{what}: not built for GraphTransformer: {_TRANSFORMER_RESIDENT}")
        return _check_transformer(model, what)
    if not isinstance(model, admits):
        if isinstance(model, GATv2):
            raise NotImplementedError(f"{what}: not built for GATv2: {_GATV2_RESIDENT}")
        names = [c.__name__ for c in admits]
        raise NotImplementedError(f"{what}: implemented for {', '.join(names[:-1])} and {names[-1]}, not "
                                  f"{type(model).__name__}")
    if isinstance(model, GATv2):
        _check_gatv2(model, what)
    if isinstance(model, SAGEResInception):
        _resinc_head(model)
    if isinstance(model, GAT):
        _check_gat(model, what)


def _check_run(what, act_dtype, rows_per_slab, nodes):
    """the drivers' own arguments; returns rows_per_slab as an int"""
    if act_dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: act_dtype must be torch.float32 or torch.bfloat16, got {act_dtype}")
    rows_per_slab = int(rows_per_slab)
    if rows_per_slab < 1:
        raise ValueError(f"{what}: rows_per_slab must be positive, got {rows_per_slab}")
    if nodes is not None and (not isinstance(nodes, torch.Tensor) or nodes.dtype != torch.int64 or nodes.dim() != 1):
        raise ValueError(f"{what}: nodes must be a 1-D int64 tensor")
    return rows_per_slab


def _score(model, place, nodes, rows_per_slab, act_dtype, sink, plan=None):
    """the frame of every driver: eval mode (restored), no gradient, autocast off, the table's device current; a rank
    that fails aborts the placement, so that its peers raise instead of waiting, and every mapping is closed"""
    layers = _attn_layers if isinstance(model, (GAT, GATv2, GraphTransformer)) else \
        _resinc_layers if isinstance(model, SAGEResInception) else _conv_layers
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), torch.autocast("cuda", enabled=False), torch.cuda.device(place.dev):
            place.bind()
            if plan is not None:                         # (a receptive field's: SAGE, GIN and GAT)
                return layers(model, place, nodes, rows_per_slab, act_dtype, sink, plan)
            return layers(model, place, nodes, rows_per_slab, act_dtype, sink)
    except BaseException:
        place.abort()
        raise
    finally:
        place.close()
        model.train(was_training)


def layerwise_inference(model, x, rowptr, col, *, nodes=None, rows_per_slab=1 << 20, act_dtype=torch.float32,
                        edge_weight=None):
    """Exact log-probabilities of every node, [N, classes] fp32 -- or of ``nodes`` (int64, any order, duplicates
    allowed), [len(nodes), classes] -- for a ``SAGE``, ``GIN``, ``GAT``, ``SAGEResInception``, ``GCN`` or ``GATv2`` model
    over the whole graph; every model's ``.inference`` is this call.  The seventh model, ``GraphTransformer``, has no
    ``.inference`` method and is scored by this call directly (``_attn_layers`` with ``_transformer_layer``: heads in
    {1, 2, 4, 8}, heads * padded channels <= 1024, one resident matrix, no ``Fp8Table``, no ``edge_weight``; its five
    live matrices are that recipe's arithmetic).  Each driver's docstring has its order of operations
    and its memory: ``_conv_layers`` (SAGE, GIN and, through ``_gcn_layer``, GCN), ``_attn_layers`` with ``_gat_layer``
    (GAT at any ``heads``) and ``_gatv2_layer`` (GATv2: heads in {1, 2, 4, 8}, heads * padded channels <= 1024, one
    resident matrix and no ``Fp8Table``) and ``_resinc_layers`` (SAGEResInception).  What follows describes SAGE and
    GIN; the arguments, the fixed GEMM tiles, eval mode and ``nodes`` mean the same for all six.

    ``edge_weight`` (GCN only; a ``ValueError`` with any other model): contiguous fp32 [E], one value per entry of
    ``col`` -- what ``adj_t`` carries in training; None: every entry weighs 1.  GCN reads one resident fp16 / fp32 / bf16
    matrix through ``spp_graph_agg_weighted_forward``: with ``normalize=True`` the kernel forms PyG's coefficients from
    ``gcn_dinv``'s fp32 [N] (4 * N bytes, 0.44 GB at N = 111 M), so neither path allocates an [E] array (12.8 GB of
    fp32 at E = 3.2 G); an ``Fp8Table`` and the partitioned and field entries take no weights and refuse the model.

    Layer by layer, slab by slab of ``rows_per_slab`` nodes: ``spp_graph_agg_forward`` over each node's whole neighbour
    row, then the layer's own parameters as torch GEMMs (SAGE: [mean | x] @ [W_l | W_r]^T; GIN: ``conv.nn`` with
    BatchNorm's running statistics), written -- SAGE: through the ReLU -- into the next [N, hidden] activation matrix of
    dtype ``act_dtype``.  The GEMMs run over row tiles of one fixed height, so a node's result is the same bits whatever
    the slab size and whether ``nodes`` selected it.  With ``act_dtype=torch.bfloat16`` operands, weights and activations
    are bf16 as under ``torch.autocast`` in training (fp32 sums, fp32 log_softmax).  With ``nodes`` the last conv layer,
    GIN's head and the log_softmax are computed for those nodes only.  The model is put in eval mode and its mode
    restored; nothing records a gradient.  ``x``: a CUDA fp16 / fp32 / bf16 matrix, one row per node, possibly a strided
    view of the resident table (``FastSampler.resident_graph()``) -- or an ``Fp8Table``, read in place with the bits of
    the same call on its fp32 dequantisation (SAGE, GIN, GAT and SAGEResInception; ``evaluate`` and the field entries
    too).  Nothing waits for the device but the range check of ``nodes``, up front.

    Memory, as arithmetic: an activation matrix is N * hidden * sizeof(act_dtype) bytes and two are live at a layer
    boundary (layer i-1's is freed as soon as layer i is complete).  At N = 111 M and hidden 256 that is 113 GB each in
    fp32 and 57 GB in bf16, next to 26 GB of graph and 28 GB of features: fp32 activations do not fit one 288 GB MI355X
    at papers scale, ``act_dtype=torch.bfloat16`` does (26 + 28 + 2 * 57 = 168 GB)."""
    return _resident("layerwise_inference", model, x, rowptr, col, nodes, rows_per_slab, act_dtype, None, _LogProbs(),
                     edge_weight)


def _check_labels(what, name, y, rows):
    if not isinstance(y, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(y).__name__}")
    if y.dtype != torch.int64 or tuple(y.shape) != (rows,) or not y.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous int64 tensor of shape [{rows}] (one label per node, -1: none), got "
                         f"{tuple(y.shape)} {y.dtype}")


def _resident(what, model, x, rowptr, col, nodes, rows_per_slab, act_dtype, y, sink, edge_weight=None):
    """the resident entries: every argument check, then the device, then the pass into ``sink``"""
    _check_model(model, what, _RESIDENT_MODELS)
    gcn = isinstance(model, GCN)
    if edge_weight is not None and not gcn:
        raise ValueError(f"{what}: edge_weight is GCN's (the values its adj_t carries in training); "
                         f"{type(model).__name__} has no weighted aggregation")
    if gcn:
        if isinstance(x, (list, tuple, P2PPeers)):
            raise NotImplementedError(f"{what}: GCN over a row-partitioned x ({type(x).__name__}); {_WEIGHTS_NOT_BUILT}")
        _check_matrix(x, what, fp8_reason=f"GCN: {_WEIGHTS_NOT_BUILT}")
    elif isinstance(model, GATv2):
        _check_matrix(x, what, fp8_reason=f"GATv2: {_GATV2_RESIDENT}")
    elif isinstance(model, GraphTransformer):
        if isinstance(x, (list, tuple, P2PPeers)):
            raise NotImplementedError(f"{what}: GraphTransformer over a row-partitioned x ({type(x).__name__}); "
                                      f"{_TRANSFORMER_RESIDENT}")
        _check_matrix(x, what, fp8_reason=f"GraphTransformer: {_TRANSFORMER_RESIDENT}")
    else:
        _check_table(x, what)
    N = x.size(0)
    _check_graph(what, N, rowptr, col)
    if edge_weight is not None:
        _check_fp32(what, "edge_weight", edge_weight, (col.numel(),), "one value per entry of col, as adj_t carries them")
        if edge_weight.device != col.device:
            raise ValueError(f"{what}: edge_weight must live on col's device")
    rows_per_slab = _check_run(what, act_dtype, rows_per_slab, nodes)
    if y is not None:
        _check_labels(what, "y", y, N)
    nat.require_device()
    if not (x.is_cuda and rowptr.device == x.device and col.device == x.device):
        raise ValueError(f"{what}: x, rowptr and col must live on one CUDA device")
    if y is not None and y.device != x.device:
        raise ValueError(f"{what}: y must live on x's device")
    if nodes is not None:
        nodes = nodes.to(x.device).contiguous()
        if nodes.numel() and not (0 <= int(nodes.min()) and int(nodes.max()) < N):      # (one read-back, up front)
            raise ValueError(f"{what}: nodes outside the graph's {N} nodes")
    return _score(model, _Resident(x, rowptr, col, edge_weight), nodes, rows_per_slab, act_dtype, sink)


def _check_splits(what, splits, nodes):
    """(nodes, segments) of ``splits``: the concatenation of its id lists and {name: (first, end)} within it"""
    if splits is None:
        return nodes, {}
    if nodes is not None:
        raise ValueError(f"{what}: give either nodes or splits, not both (splits scores the concatenation of its lists)")
    if not isinstance(splits, dict) or not splits:
        raise TypeError(f"{what}: splits must be a non-empty dict of name -> 1-D int64 tensor of node ids")
    segments, first = {}, 0
    for name, ids in splits.items():
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() != 1:
            raise ValueError(f"{what}: splits[{name!r}] must be a 1-D int64 tensor of node ids")
        segments[name] = (first, first + ids.numel())
        first += ids.numel()
    devs = {ids.device for ids in splits.values()}
    if len(devs) > 1:
        raise ValueError(f"{what}: the lists of splits live on different devices ({sorted(map(str, devs))})")
    return torch.cat(list(splits.values())), segments


def evaluate(model, x, rowptr, col, y=None, *, nodes=None, splits=None, rows_per_slab=1 << 20, act_dtype=torch.float32,
             edge_weight=None):
    """Exact whole-graph evaluation: ``layerwise_inference``'s pass -- the same checks, layer loops, fixed GEMM tiles and
    eval-mode frame -- with the other tail: each tile of the last layer's logits goes through ``classify_rows``
    (``spp_classify_rows``) into its rows of ``pred`` and ``nll``, and no [rows, classes] matrix is ever allocated
    (at N = 111 M and 172 classes that matrix is 76 GB of fp32).  Returns an ``Evaluation``.

    ``y``: int64 [N] on x's device, indexed by global node id; a label outside [0, classes) (-1) marks an unlabelled
    node, which counts nowhere and has nll 0.  Without ``y`` only ``pred`` is computed.  ``nodes`` (int64, any order,
    duplicates allowed) scores those nodes only; ``splits`` = {"valid": ids, "test": ids, ...} scores the concatenation
    of the lists once (``pred`` and ``nll`` follow it) and also returns labelled / correct / loss per name.  A node's
    ``pred`` and ``nll`` are the same bits whatever ``rows_per_slab`` is and whether ``nodes`` selected it; ``pred[i]`` is
    the argmax of the logits, so ``layerwise_inference``'s row attains its maximum there.  The counts are reduced on the
    device and read back once, at the end.  ``edge_weight``: GCN's entry weights, as ``layerwise_inference`` takes them.
    The seven models of ``layerwise_inference`` (``GraphTransformer`` included), each through the driver named there."""
    what = "evaluate"
    nodes, segments = _check_splits(what, splits, nodes)
    sink = _resident(what, model, x, rowptr, col, nodes, rows_per_slab, act_dtype, y, _Classify(y), edge_weight)
    return _evaluation(sink, y, None if nodes is None else nodes.to(x.device), segments)


def gatv2_inference(model, x, rowptr, col, *, nodes=None, rows_per_slab=1 << 20, act_dtype=torch.float32):
    """``layerwise_inference`` under the name GATv2's entry had first: the same call, for a ``models.GATv2`` model only"""
    what = "gatv2_inference"
    if not isinstance(model, GATv2):
        raise NotImplementedError(f"{what}: implemented for GATv2, not {type(model).__name__} (the other models: "
                                  "layerwise_inference)")
    return _resident(what, model, x, rowptr, col, nodes, rows_per_slab, act_dtype, None, _LogProbs())


def transformer_inference(model, x, rowptr, col, *, nodes=None, rows_per_slab=1 << 20, act_dtype=torch.float32):
    """``layerwise_inference`` under GraphTransformer's own name: the same call, for a ``models.GraphTransformer`` model
    only (``_transformer_layer`` has the order of operations and the memory)"""
    what = "transformer_inference"
    if not isinstance(model, GraphTransformer):
        raise NotImplementedError(f"{what}: implemented for GraphTransformer, not {type(model).__name__} (the other "
                                  "models: layerwise_inference)")
    return _resident(what, model, x, rowptr, col, nodes, rows_per_slab, act_dtype, None, _LogProbs())


# ---- f3n: a few nodes scored exactly over their receptive field only -------------------------------------------------
def field_chunk():
    """C_f (include/spp.h, f3n): the field kernels finish a row of at most C_f entries with a lane group and give a
    longer one a workgroup"""
    return int(nat.load().spp_field_chunk())


def field_workspace_bytes(num_ids):
    return int(nat.load().spp_field_workspace_bytes(int(num_ids)))


def _field_call(entry, rowptr, col, N, ids, slot, flag=None, frowptr=None, fcol=None):
    """one of the two entries of csrc/field.hip over ``ids``, with a workspace of its own"""
    ws = torch.empty(field_workspace_bytes(ids.numel()), dtype=torch.uint8, device=slot.device)
    d = nat.FieldDesc(rowptr_dev=_p(rowptr), col_dev=_p(col), num_nodes=N, ids_dev=_p(ids), num_ids=ids.numel(),
                      slot_dev=_p(slot), flag_dev=_p(flag), frowptr_dev=_p(frowptr), fcol_dev=_p(fcol),
                      fcol_len=fcol.numel() if fcol is not None else 0)
    with torch.cuda.device(slot.device):
        nat.check(entry(C.byref(d), C.c_void_p(ws.data_ptr()), ws.numel(), _stream()))


def _field_mark(rowptr, col, N, frontier, slot, flag):
    """``spp_field_mark``: flag[j] = 1 for every neighbour j of a frontier node that has no slot"""
    if frontier.numel() and col.numel():
        _field_call(nat.load().spp_field_mark, rowptr, col, N, frontier, slot, flag=flag)


def _field_rows(rowptr, col, N, ids, slot, frowptr, fcol):
    """``spp_field_rows``: the rows of ``ids`` in CSR order, every entry replaced by its slot"""
    if ids.numel() and fcol.numel():
        _field_call(nat.load().spp_field_rows, rowptr, col, N, ids, slot, frowptr=frowptr, fcol=fcol)


def _check_nodes(what, nodes, N):
    """``nodes`` of the field entries: a 1-D int64 tensor inside [0, N) (one read-back when it lives on a device)"""
    if not isinstance(nodes, torch.Tensor):
        raise TypeError(f"{what}: nodes must be a torch.Tensor, got {type(nodes).__name__}")
    if nodes.dtype != torch.int64 or nodes.dim() != 1:
        raise ValueError(f"{what}: nodes must be a 1-D int64 tensor, got {tuple(nodes.shape)} {nodes.dtype}")
    if nodes.numel():
        lo, hi = torch.stack([nodes.min(), nodes.max()]).tolist()
        if lo < 0 or hi >= N:
            raise ValueError(f"{what}: nodes outside the graph's {N} nodes (from {lo} to {hi})")


def _check_hops(what, hops):
    if not isinstance(hops, int) or isinstance(hops, bool):
        raise TypeError(f"{what}: hops must be an int, got {type(hops).__name__}")
    if hops < 0:
        raise ValueError(f"{what}: hops must not be negative, got {hops}")


def _check_csr(what, rowptr, col):
    """a graph's CSR on its own (no matrix gives N): contiguous 1-D int64 tensors, N + 1 >= 1 entries of rowptr"""
    for name, t in (("rowptr", rowptr), ("col", col)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous 1-D int64 tensor")
    if rowptr.numel() < 1:
        raise ValueError(f"{what}: rowptr must hold N + 1 entries, got none")


class Field:
    """The receptive field of ``nodes`` over ``hops`` = h hops, as ``ReceptiveFields.field`` builds it.  Depth 0 is the
    distinct ids of ``nodes``, depth d every neighbour of a node of depth d - 1 that has no smaller depth; SLOTS count
    the field's nodes depth by depth, in ascending id order within a depth.

    ``ids`` int64 [n_h]: the global id of every slot.  ``sizes``: a list, sizes[d] = the nodes of depth <= d, d = 0..h.
    ``pos`` int64 [len(nodes)]: the slot of each given node (< sizes[0]).  ``rowptr`` int64 [sizes[h-1] + 1] and ``col``
    int64: the rows of every node of depth <= h - 1 in slot order, each the node's WHOLE row of the graph in CSR order
    with every entry replaced by its slot (with h = 0: no rows, rowptr == [0]).  The rows [0, sizes[d]) refer only to
    slots below sizes[d + 1]: a nest of prefixes, as a sampled MFG is."""

    def __init__(self, ids, sizes, pos, rowptr, col):
        self.ids, self.sizes, self.pos, self.rowptr, self.col = ids, sizes, pos, rowptr, col

    @property
    def hops(self):
        return len(self.sizes) - 1

    def __repr__(self):
        return f"Field(hops={self.hops}, sizes={self.sizes}, edges={self.col.numel()})"


class ReceptiveFields:
    """What building fields over one resident graph needs, allocated once: the slot map (int32 [N], -1 = not in the
    field) and the flags (one byte per node), 5 bytes a node (555 MB at N = 111 M).  ``field(nodes, hops)`` leaves both as
    it found them -- also when it raises -- by resetting the entries it touched, so a call costs what its own field costs
    plus, per hop, one pass over the flags (``nonzero``: N bytes read, and the hop's count read back)."""

    def __init__(self, rowptr, col):
        what = "ReceptiveFields"
        _check_csr(what, rowptr, col)
        nat.require_device()
        if not (rowptr.is_cuda and col.device == rowptr.device):
            raise ValueError(f"{what}: rowptr and col must live on one CUDA device")
        self.rowptr, self.col, self.N, self.dev = rowptr, col, rowptr.numel() - 1, rowptr.device
        self.slot = torch.full((self.N,), -1, dtype=torch.int32, device=self.dev)
        self.flag = torch.zeros(self.N, dtype=torch.uint8, device=self.dev)

    def field(self, nodes, hops):
        """The ``Field`` of ``nodes`` (int64, any order, duplicates allowed, all inside the graph) over ``hops`` >= 0
        hops.  Deterministic: ``spp_field_mark`` flags the next depth with plain stores of one value, the flags are
        compacted in ascending id order, and ``spp_field_rows`` copies the rows.  Waits for the device once for the
        range check, once per hop (the depth's count), once for the field's edge count and once for the check that
        every entry of ``col`` found its slot."""
        what = "ReceptiveFields.field"
        _check_hops(what, hops)
        _check_nodes(what, nodes, self.N)
        return self._build(nodes.to(self.dev).contiguous(), hops)

    def _build(self, nodes, hops):
        """``field`` behind its checks"""
        rowptr, col, N, slot, flag, dev = self.rowptr, self.col, self.N, self.slot, self.flag, self.dev
        depths, marked = [], False
        try:
            with torch.no_grad(), torch.cuda.device(dev):
                first, pos = torch.unique(nodes, return_inverse=True)          # ascending; pos: each node's slot
                depths.append(first)
                sizes = [first.numel()]
                slot[first] = torch.arange(sizes[0], dtype=torch.int32, device=dev)
                for _ in range(hops):
                    frontier = depths[-1]
                    if frontier.numel():                 # (an empty depth ends the field: the later ones are empty too)
                        marked = True
                        _field_mark(rowptr, col, N, frontier, slot, flag)
                        new = flag.nonzero().view(-1)    # ascending ids; N bytes read, the count read back
                        flag[new] = 0
                        marked = False
                        slot[new] = torch.arange(sizes[-1], sizes[-1] + new.numel(), dtype=torch.int32, device=dev)
                    else:
                        new = frontier
                    depths.append(new)
                    sizes.append(sizes[-1] + new.numel())
                ids = torch.cat(depths)
                rows = ids[:sizes[hops - 1]] if hops else ids[:0]
                frowptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=dev)
                torch.cumsum(rowptr[rows + 1] - rowptr[rows], 0, out=frowptr[1:])
                fcol = torch.empty(int(frowptr[-1]) if rows.numel() else 0, dtype=torch.int64, device=dev)
                _field_rows(rowptr, col, N, rows, slot, frowptr, fcol)
                if fcol.numel() and int(fcol.min()) < 0:
                    raise RuntimeError("ReceptiveFields.field: an entry of the field's rows has no slot (the graph's col "
                                       "leaves [0, N), or rowptr / col changed during the call)")
                return Field(ids, sizes, pos, frowptr, fcol)
        finally:
            for d in depths:
                slot[d] = -1
            if marked:                                   # raised between a mark and its clear: which flags is unknown
                flag.zero_()


def receptive_field(rowptr, col, nodes, hops):
    """``ReceptiveFields(rowptr, col).field(nodes, hops)``: the one-shot form (it allocates and fills the 5 bytes a node)"""
    what = "receptive_field"
    _check_hops(what, hops)
    _check_csr(what, rowptr, col)
    _check_nodes(what, nodes, rowptr.numel() - 1)
    return ReceptiveFields(rowptr, col)._build(nodes.to(rowptr.device).contiguous(), hops)


def _classes(model):
    """the width of the model's logits"""
    return model.lin2.out_features if isinstance(model, GIN) else model.convs[-1].out_channels if isinstance(model, GAT) \
        else model.convs[-1].lin_l.out_features


def _field_score(what, model, x, rowptr, col, nodes, rows_per_slab, act_dtype, fields, y, sink):
    """the field entries: every argument check, then the device, then the field of ``nodes`` and the pass over it into
    ``sink``.  Returns (nodes on x's device, each node's row of the sink or None without nodes)."""
    if isinstance(model, SAGEResInception):
        raise NotImplementedError(f"{what}: SAGEResInception is not scored over a receptive field: its head accumulates a "
                                  "block of every layer for the scored nodes, and the field's layers have different row "
                                  "counts in slot order; layerwise_inference(nodes=...) scores it")
    _check_model(model, what, _FIELD_MODELS)
    if isinstance(x, (list, tuple, P2PPeers)):
        raise NotImplementedError(f"{what}: a row-partitioned table is not scored over a receptive field (layer 0 reads "
                                  "one resident matrix in place and the field's layers live on one device); "
                                  "partitioned_inference(nodes=...) scores it")
    _check_table(x, what)
    N = x.size(0)
    _check_graph(what, N, rowptr, col)
    rows_per_slab = _check_run(what, act_dtype, rows_per_slab, None)
    if y is not None:
        _check_labels(what, "y", y, N)
    if fields is not None:
        if not isinstance(fields, ReceptiveFields):
            raise TypeError(f"{what}: fields must be a ReceptiveFields, got {type(fields).__name__}")
        if fields.rowptr.data_ptr() != rowptr.data_ptr() or fields.col.data_ptr() != col.data_ptr() or fields.N != N:
            raise ValueError(f"{what}: fields was made for another graph than rowptr / col")
    _check_nodes(what, nodes, N)                          # (one read-back, up front)
    nat.require_device()
    if not (x.is_cuda and rowptr.device == x.device and col.device == x.device):
        raise ValueError(f"{what}: x, rowptr and col must live on one CUDA device")
    if y is not None and y.device != x.device:
        raise ValueError(f"{what}: y must live on x's device")
    nodes = nodes.to(x.device).contiguous()
    if not nodes.numel():
        return nodes, None
    n_layers = len(model.convs)
    field = (fields or ReceptiveFields(rowptr, col))._build(nodes, n_layers - 1)
    _score(model, _Resident(x, rowptr, col), None, rows_per_slab, act_dtype, sink, _field_plan(field, n_layers))
    return nodes, field.pos


def field_inference(model, x, rowptr, col, nodes, *, rows_per_slab=1 << 20, act_dtype=torch.float32, fields=None):
    """``layerwise_inference(model, x, rowptr, col, nodes=nodes, ...)`` -- the same bits, [len(nodes), classes] fp32
    log-probabilities -- computed over the receptive field of ``nodes`` only: for a model of L conv layers the nodes
    within L - 1 hops (``ReceptiveFields``, ``Field``), not all N.  ``SAGE``, ``GIN`` and ``GAT`` (any ``heads``) over a
    resident table; SAGEResInception and a partitioned table are refused with the reason.

    The plan (``_field_plan``): layer 0 runs on the ORIGINAL graph and table with ``target_ids=field.ids`` -- the table
    is read in place, nothing of it is gathered, and the widest hop never exists as a matrix (GAT: the first projection
    stays whole-table, the attention takes the list); layer i >= 1 runs on the field's CSR as a slab, for the slots
    below sizes[L-1-i], reading layer i-1's rows; the last layer leaves the DISTINCT nodes' logits, which go through the
    sink and are expanded by ``field.pos``.  Kernels and the fixed GEMM tiles are ``layerwise_inference``'s, and a row's
    bits depend on its own row alone, so the two entries agree bit for bit.

    ``fields``: a ``ReceptiveFields`` of this graph to reuse (5 bytes a node, allocated once); without one a temporary is
    made.  When NOT to use this entry: the field of a few thousand nodes of a small-world graph can approach the whole
    graph after two hops, and then the field (its build, its CSR copy, layer 0 by list) costs more than the plain pass;
    ``ReceptiveFields.field(nodes, L - 1).sizes`` tells before the model runs."""
    what = "field_inference"
    sink = _LogProbs()
    _nodes, pos = _field_score(what, model, x, rowptr, col, nodes, rows_per_slab, act_dtype, fields, None, sink)
    if pos is None:                                      # no nodes: nothing was launched
        return torch.empty((0, _classes(model)), dtype=torch.float32, device=x.device)
    return sink.out[pos]


def field_evaluate(model, x, rowptr, col, y=None, *, nodes=None, splits=None, rows_per_slab=1 << 20,
                   act_dtype=torch.float32, fields=None):
    """``evaluate(model, x, rowptr, col, y, nodes= / splits=, ...)`` over the receptive field of the scored nodes only:
    ``field_inference``'s pass ended in ``classify_rows``.  Distinct nodes are scored once (their labels read as
    ``y[ids]``) and ``pos`` expands ``pred`` and ``nll`` to the order given; ``pred``, ``nll``, the counts, the loss and
    ``splits`` equal ``evaluate``'s exactly.  One of ``nodes`` and ``splits`` is required: ``evaluate`` scores every node."""
    what = "field_evaluate"
    nodes, segments = _check_splits(what, splits, nodes)
    if nodes is None:
        raise ValueError(f"{what}: give nodes or splits (the nodes whose field is scored); evaluate scores every node")
    sink = _Classify(y)
    nodes, pos = _field_score(what, model, x, rowptr, col, nodes, rows_per_slab, act_dtype, fields, y, sink)
    if pos is None:
        sink.classes = _classes(model)
        sink.pred = torch.empty(0, dtype=torch.int64, device=x.device)
        sink.nll = torch.empty(0, dtype=torch.float32, device=x.device) if y is not None else None
    else:
        sink.pred, sink.nll = sink.pred[pos], sink.nll[pos] if sink.nll is not None else None
    return _evaluation(sink, y, nodes, segments)


class LocalPeers:
    """``peers`` of ``partitioned_layerwise_inference`` for ranks that are THREADS of one process on one device: one
    object shared by the threads.  ``share`` hands every rank the others' tensors as plain device addresses; ``barrier``
    is a ``threading.Barrier`` with a timeout.  A rank that fails calls ``abort`` (the driver does), which breaks the
    barrier: the other ranks raise instead of waiting.  ``bind(rank)`` tells the object which rank the calling thread is."""

    def __init__(self, world, timeout=120.0):
        self.world = int(world)
        if self.world < 1:
            raise ValueError(f"LocalPeers: world must be positive, got {world}")
        self._barrier = threading.Barrier(self.world, timeout=float(timeout))
        self._slots = [None] * self.world
        self._tls = threading.local()

    def bind(self, rank):
        if not 0 <= int(rank) < self.world:
            raise ValueError(f"LocalPeers: rank {rank} outside the world of {self.world}")
        self._tls.rank = int(rank)

    def barrier(self):
        try:
            self._barrier.wait()
        except threading.BrokenBarrierError:
            raise RuntimeError("LocalPeers: another rank failed or did not arrive within the timeout") from None

    def abort(self):
        self._barrier.abort()

    def share(self, tensor):
        rank = getattr(self._tls, "rank", None)
        if rank is None:
            raise RuntimeError("LocalPeers: bind(rank) first (which rank is this thread?)")
        self._slots[rank] = tensor
        self.barrier()                                   # every rank has posted
        tabs = list(self._slots)
        self.barrier()                                   # every rank has read: the slots may be posted again
        live = [t for t in tabs if t is not None and t.numel()]
        if len({t.device for t in live}) > 1:
            raise ValueError("LocalPeers: the ranks' tensors live on different devices; in-process ranks share one")
        return P2PPeers([t.data_ptr() if t is not None and t.numel() else 0 for t in tabs],
                        _common_stride([_table_stride_bytes(t) for t in live]) if live else 0, keep=tabs)

    def close(self):
        pass


class IpcPeers:
    """``peers`` of ``partitioned_layerwise_inference`` for one PROCESS per rank on one node, over a torch.distributed
    group of any backend: ``share`` is ``p2p_open_peers`` (HIP IPC handles by all_gather_object; peer access is enabled by
    the mapping call, nowhere else), a fresh set of mappings per call that its ``P2PPeers.close()`` unmaps -- nothing is
    cached between calls, so no address outlives the allocation it was opened for.  ``barrier`` is
    ``dist.monitored_barrier`` with a timeout where the backend has it (gloo), a plain barrier otherwise."""

    def __init__(self, group=None, timeout=300.0):
        self.group, self.timeout = group, float(timeout)

    def share(self, tensor):
        return p2p_open_peers(tensor, self.group)

    def barrier(self):
        import datetime
        import torch.distributed as dist
        if dist.get_backend(self.group) == "gloo":
            dist.monitored_barrier(self.group, timeout=datetime.timedelta(seconds=self.timeout))
        else:
            dist.barrier(self.group)

    def close(self):
        pass


def _partitioned(what, model, x_local, rowptr, col, part_offsets, rank, peers, nodes, rows_per_slab, act_dtype,
                 y_local=None, sink=None):
    """the partitioned entries.  Every argument and model-shape check comes before ``peers``
    is touched, and the device is required last: a refused call publishes nothing and waits for nobody."""
    _check_model(model, what, _PARTITIONED_MODELS)
    _refuse_max_over_parts(what, model)
    _check_matrix(x_local, what, "x_local", "the partitioned drivers do not carry fp8 partitions through peers.share yet "
                  "(graph_aggregate_parts reads them); dequantise the partition, or score the table on one device")
    off = _check_offsets(part_offsets, what)
    P = len(off) - 1
    rank = int(rank)
    if not 0 <= rank < P:
        raise ValueError(f"{what}: rank {rank} outside the {P} parts")
    lo, hi = off[rank], off[rank + 1]
    if x_local.size(0) != hi - lo:
        raise ValueError(f"{what}: x_local has {x_local.size(0)} rows, part_offsets gives rank {rank} {hi - lo}")
    _check_graph(what, off[-1], rowptr, col, parts=True)
    rows_per_slab = _check_run(what, act_dtype, rows_per_slab, nodes)
    if nodes is not None and nodes.numel() and not (lo <= int(nodes.min()) and int(nodes.max()) < hi):
        raise ValueError(f"{what}: nodes outside rank {rank}'s range [{lo}, {hi}) (global ids; every rank scores its own)")
    if y_local is not None:
        _check_labels(what, "y_local", y_local, hi - lo)
    for name in ("share", "barrier", "close"):
        if not callable(getattr(peers, name, None)):
            raise TypeError(f"{what}: peers must provide share(tensor), barrier() and close()")
    nat.require_device()
    dev = x_local.device
    if not (x_local.is_cuda and rowptr.device == dev and col.device == dev):
        raise ValueError(f"{what}: x_local, rowptr and col must live on one CUDA device")
    if y_local is not None and y_local.device != dev:
        raise ValueError(f"{what}: y_local must live on x_local's device")
    if nodes is not None:
        nodes = nodes.to(dev).contiguous()
    return _score(model, _Partitioned(what, x_local, rowptr, col, off, rank, peers), nodes, rows_per_slab, act_dtype,
                  _LogProbs() if sink is None else sink)


def partitioned_inference(model, x_local, rowptr, col, *, part_offsets, rank, peers, nodes=None, rows_per_slab=1 << 20,
                          act_dtype=torch.float32):
    """``layerwise_inference`` for ``SAGE``, ``GIN``, ``GAT`` and ``SAGEResInception`` when the feature table is
    row-partitioned over the ranks.  Every rank calls this with its own partition ``x_local`` (the global rows
    [part_offsets[rank], part_offsets[rank + 1])), the WHOLE graph's CSR (global ids) and the same ``model``, and gets the
    fp32 log-probabilities of ITS node range, [n_local, classes] -- or of ``nodes`` (global ids, all inside the rank's
    range).  The bits are those of ``layerwise_inference`` over the concatenated table, those rows: the layer loops are
    the same code (``_conv_layers``, ``_attn_layers``, ``_resinc_layers``) over the same fixed GEMM tiles.

    Per rank (``_Partitioned``): the buffers the other ranks read are allocated up front and published once through
    ``peers`` -- SAGE, GIN and SAGEResInception: ``x_local`` and the ping-pong activation buffers [n_local, hidden] of
    ``act_dtype`` (one for a two-layer model); GAT: h and the logits, the projection being local.  Each layer aggregates
    the rank's own slabs with the parts kernels over ALL ranks' parts and writes its rows of the next layer into its own
    buffer; then the rank synchronises its stream and waits in ``peers.barrier()`` before anyone reads the layer or
    reuses a buffer (GAT: twice a layer, after h and the logits are written and after the layer is attended).  After the
    last barrier the mappings are closed.

    ``peers``: ``share(tensor) -> P2PPeers`` (collective, same order on every rank), ``barrier()``, ``close()``; optional
    ``bind(rank)`` and ``abort()`` (called when a rank fails, so that the others raise instead of waiting).
    ``LocalPeers`` and ``IpcPeers`` are the two implementations.  The model-shape refusals are
    ``layerwise_inference``'s, and like every argument check they come before ``peers`` is touched.

    Memory, as arithmetic (SAGE on S-mag, N = 121.8 M, F = 768 fp16, hidden 256, bf16): per rank of P, 187 / P GB of
    table and 2 * 62 / P GB of activations next to its copy of the 22 GB graph.  GAT at papers scale (N = 111 M, hidden
    256, 172 classes, H = 1, bf16, P = 8, so 13.9 M rows a rank): the h buffer 13.9 M * 256 * 2 B = 7.1 GB and the logits
    13.9 M * 8 B = 0.11 GB, both live for the whole call; one [n_local, 256] bf16 activation matrix at a time beside them
    (``cur`` while a layer projects, ``nxt`` while it attends), 7.1 GB; the last layer's [n_local, 172] fp32 result,
    9.5 GB; 3.6 GB of table and the rank's copy of the 26 GB graph: about 47 GB at the peak, against 168 GB on one
    device."""
    return _partitioned("partitioned_inference", model, x_local, rowptr, col, part_offsets, rank, peers, nodes,
                        rows_per_slab, act_dtype)


def partitioned_evaluate(model, x_local, rowptr, col, y_local=None, *, part_offsets, rank, peers, nodes=None,
                         rows_per_slab=1 << 20, act_dtype=torch.float32):
    """``evaluate`` when the feature table is row-partitioned over the ranks: ``partitioned_inference``'s pass (same
    arguments, same collective behaviour through ``peers``) ending in ``classify_rows`` instead of the [n_local, classes]
    matrix.  Every rank scores its own rows -- or ``nodes``, global ids inside its range -- and gets an ``Evaluation`` of
    them; the ranks' ``pred`` and ``nll`` concatenated are the bits of ``evaluate`` over the concatenated table.
    ``y_local``: int64 [n_local] on x_local's device, the rank's labels by LOCAL id (-1: unlabelled).  ``labelled``,
    ``correct`` and ``loss`` cover the rank's rows: the caller adds the counts (and ``loss * labelled``) across ranks."""
    what = "partitioned_evaluate"
    sink = _partitioned(what, model, x_local, rowptr, col, part_offsets, rank, peers, nodes, rows_per_slab, act_dtype,
                        y_local, _Classify(y_local))
    lo = sink.place.lo
    return _evaluation(sink, y_local, None if nodes is None else nodes.to(x_local.device) - lo, {})


def partitioned_layerwise_inference(model, x_local, rowptr, col, *, part_offsets, rank, peers, nodes=None,
                                    rows_per_slab=1 << 20, act_dtype=torch.float32):
    """``partitioned_inference`` under the name the entry had first: the same call, its own name in the errors"""
    return _partitioned("partitioned_layerwise_inference", model, x_local, rowptr, col, part_offsets, rank, peers, nodes,
                        rows_per_slab, act_dtype)
