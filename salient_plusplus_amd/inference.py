"""Exact, layer-wise inference over the whole resident graph (reference: driver/models.py:441 ``layerwise_inference``
with ``SAGE.inference``): every node is scored from ALL its neighbours, one pass per layer over the graph's CSR, with
no sampling, no dedup and no exchange.  The message passing is the HIP kernel pair of csrc/graph_aggregate.hip
(``spp_graph_agg_forward``) for SAGE, GIN and SAGEResInception and of csrc/graph_gat.hip (``spp_graph_gat_forward``) for
GAT; SAGEResInception's layer tail is csrc/resinc_epilogue.hip (``spp_resinc_epilogue``); the layers' own parameters run
through the library GEMMs torch dispatches to.

``graph_aggregate``, ``graph_gat_aggregate`` and ``resinc_epilogue`` are the kernels' thin wrappers,
``layerwise_inference`` the driver behind ``SAGE.inference`` and ``GIN.inference`` and the entry point for ``GAT`` and
``SAGEResInception``.  Forward only, one GPU, fp16 / fp32 / bf16 inputs.

Over a row-PARTITIONED feature table (one range of nodes per rank, the peers' partitions mapped into the process):
``graph_aggregate_parts`` (``spp_graph_agg_parts_forward``), ``graph_gat_aggregate_parts``
(``spp_graph_gat_parts_forward``) and ``partitioned_inference`` for all four models (``partitioned_layerwise_inference``
is its SAGE / GIN half), with ``LocalPeers`` (ranks as threads of one process) or ``IpcPeers`` (one process per rank on
one node) between the ranks."""
import ctypes as C
import threading

import torch

from . import _native as nat
from .fast_sampler import P2PPeers, RowRefs, TableRows, _common_stride, _row_stride_elems, _table_stride_bytes, \
    p2p_open_peers
from .fp8 import Fp8Features
from .models import _ELEM, _p, _stream

_EPILOGUES = {"mean": nat.SPP_AGG_MEAN, "operand": nat.SPP_AGG_OPERAND, "sum": nat.SPP_AGG_SUM}
_OUT_DTYPES = (torch.float32, torch.bfloat16)


def graph_agg_chunk():
    """C of the summation contract (include/spp.h): rows of at most C entries are summed serially in CSR order, longer
    rows as chunks of C whose sums are added in chunk order"""
    return int(nat.load().spp_graph_agg_chunk())


def graph_agg_workspace_bytes(num_targets):
    return int(nat.load().spp_graph_agg_workspace_bytes(int(num_targets)))


def _check_matrix(x, what, name="x"):
    """x as the kernels read it: a 2-D fp16 / fp32 / bf16 matrix with unit column stride that carries no gradient"""
    if isinstance(x, Fp8Features):
        raise TypeError(f"{what}: an fp8 feature table (Fp8Features) is not supported as inference input; pass "
                        "x.dequantize(torch.float16)")
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


def _check_graph(x, rowptr, col, what):
    for name, t in (("rowptr", rowptr), ("col", col)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous 1-D int64 tensor")
    if rowptr.numel() != x.size(0) + 1:
        raise ValueError(f"{what}: x has {x.size(0)} rows, the graph {rowptr.numel() - 1} nodes (one row per node)")


def graph_aggregate(x, rowptr, col, *, row0=None, num_targets=None, target_ids=None, epilogue="mean", self_scale=0.0,
                    out_dtype=torch.float32, workspace=None):
    """Aggregation over whole rows of the resident graph (``spp_graph_agg_forward``, include/spp.h).

    ``x`` [N, F]: one row per graph node (fp16 / fp32 / bf16, possibly a strided view); ``rowptr`` / ``col``: the
    graph's CSR (int64, global ids).  The targets are a slab, ``row0`` and ``num_targets`` (output row i is node
    row0 + i), or a list, ``target_ids`` (int64, any order, duplicates allowed).  ``epilogue``: "mean" [T, F],
    "operand" [T, 2F] = [mean | x[target]] or "sum" [T, F] = self_scale * x[target] + sum.  fp32 sums; a bf16 output
    is rounded once.  A ``col`` entry outside the graph reads row 0, a target id outside it gives a row of zeros.

    Forward only: no autograd node is registered and an input that requires grad is refused.  ``workspace``: a uint8
    CUDA tensor of at least ``graph_agg_workspace_bytes(T)`` bytes, reusable between calls on one stream; allocated
    when None.  Nothing here waits for the device."""
    what = "graph_aggregate"
    _check_matrix(x, what)
    _check_graph(x, rowptr, col, what)
    if epilogue not in _EPILOGUES:
        raise ValueError(f"{what}: epilogue must be 'mean', 'operand' or 'sum', got {epilogue!r}")
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
    slab = row0 is not None or num_targets is not None
    if slab == (target_ids is not None):
        raise ValueError(f"{what}: give the targets either as a slab (row0 and num_targets) or as target_ids"
                         + (", not both" if slab else ""))
    N, Fdim = x.shape
    if slab:
        if row0 is None or num_targets is None:
            raise ValueError(f"{what}: a slab needs both row0 and num_targets")
        row0, T = int(row0), int(num_targets)
        if row0 < 0 or T < 0 or row0 + T > N:
            raise ValueError(f"{what}: the slab [{row0}, {row0 + T}) leaves the graph's {N} nodes")
    else:
        if not isinstance(target_ids, torch.Tensor) or target_ids.dtype != torch.int64 or target_ids.dim() != 1 \
                or not target_ids.is_contiguous():
            raise ValueError(f"{what}: target_ids must be a contiguous 1-D int64 tensor")
        row0, T = -1, target_ids.numel()
    nat.require_device()
    tensors = [x, rowptr, col] + ([target_ids] if not slab else []) + ([workspace] if workspace is not None else [])
    if not all(t.is_cuda and t.device == x.device for t in tensors):
        raise ValueError(f"{what}: x, rowptr, col, target_ids and workspace must live on one CUDA device")
    L = nat.load()
    nbytes = int(L.spp_graph_agg_workspace_bytes(T))
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < nbytes:
        raise ValueError(f"{what}: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes")
    width = 2 * Fdim if epilogue == "operand" else Fdim
    out = torch.empty((T, width), dtype=out_dtype, device=x.device)
    d = nat.GraphAggDesc(epilogue=_EPILOGUES[epilogue], x_elem=_ELEM[x.dtype], out_elem=_ELEM[out_dtype],
                         rowptr_dev=_p(rowptr), col_dev=_p(col), x_dev=_p(x),
                         x_stride_elems=x.stride(0) if N > 1 else Fdim, x_rows=N, F=Fdim, target_row0=row0,
                         target_ids_dev=_p(target_ids) if not slab else None, num_targets=T, out_dev=_p(out),
                         out_stride_elems=0, self_scale=float(self_scale))
    with torch.cuda.device(x.device):
        nat.check(L.spp_graph_agg_forward(C.byref(d), C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream()))
    return out


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


def _parts_source(parts, off, dtype, F, what, name="part"):
    """(base addresses [P], row stride in elements, dtype, F, device or None) of the two forms of ``parts``"""
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


def graph_aggregate_parts(parts, part_offsets, rowptr, col, *, row0=None, num_targets=None, target_ids=None,
                          epilogue="mean", self_scale=0.0, out_dtype=torch.float32, workspace=None, out=None,
                          dtype=None, F=None):
    """``graph_aggregate`` over a row-partitioned source (``spp_graph_agg_parts_forward``, include/spp.h): part p holds
    the global rows [part_offsets[p], part_offsets[p + 1]) of x, in an allocation of its own.  The result is the bits of
    ``graph_aggregate(torch.cat(parts), ...)``.

    ``parts``: a list of P CUDA tensors on one device (an empty part may be None or have 0 rows) that share dtype, width
    and row stride -- or a ``P2PPeers`` (the ranks' partitions as addresses in this process, ``p2p_open_peers``) with
    ``dtype=`` and ``F=``.  ``rowptr`` / ``col``: the WHOLE graph's CSR with global ids; the targets, ``epilogue``,
    ``self_scale``, ``out_dtype`` and ``workspace`` as ``graph_aggregate``, the ids global.  ``out``: an fp32 / bf16
    [T, F or 2F] matrix to write into (rows of a larger one allowed).  Nothing here maps memory or enables peer access,
    and nothing waits for the device."""
    what = "graph_aggregate_parts"
    off = _check_offsets(part_offsets, what)
    ptrs, stride, x_dtype, Fdim, dev = _parts_source(parts, off, dtype, F, what)
    N = off[-1]
    for name, t in (("rowptr", rowptr), ("col", col)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous 1-D int64 tensor")
    if rowptr.numel() != N + 1:
        raise ValueError(f"{what}: the parts hold {N} rows, the graph {rowptr.numel() - 1} nodes (one row per node)")
    if epilogue not in _EPILOGUES:
        raise ValueError(f"{what}: epilogue must be 'mean', 'operand' or 'sum', got {epilogue!r}")
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
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
    else:
        if not isinstance(target_ids, torch.Tensor) or target_ids.dtype != torch.int64 or target_ids.dim() != 1 \
                or not target_ids.is_contiguous():
            raise ValueError(f"{what}: target_ids must be a contiguous 1-D int64 tensor")
        row0, T = -1, target_ids.numel()
    width = 2 * Fdim if epilogue == "operand" else Fdim
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != out_dtype or tuple(out.shape) != (T, width) \
                or (width > 1 and out.stride(1) != 1) or out.requires_grad:
            raise ValueError(f"{what}: out must be a {out_dtype} matrix of shape [{T}, {width}] with unit column stride "
                             "that does not require grad")
    nat.require_device()
    dev = rowptr.device if dev is None else dev
    tensors = [rowptr, col] + [t for t in (None if slab else target_ids, workspace, out) if t is not None]
    if dev.type != "cuda" or not all(t.is_cuda and t.device == dev for t in tensors):
        raise ValueError(f"{what}: the parts, rowptr, col, target_ids, workspace and out must live on one CUDA device")
    L = nat.load()
    nbytes = int(L.spp_graph_agg_workspace_bytes(T))
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < nbytes:
        raise ValueError(f"{what}: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes")
    if out is None:
        out = torch.empty((T, width), dtype=out_dtype, device=dev)
    d = nat.GraphAggPartsDesc(epilogue=_EPILOGUES[epilogue], x_elem=_ELEM[x_dtype], out_elem=_ELEM[out_dtype],
                              num_parts=len(off) - 1, rowptr_dev=_p(rowptr), col_dev=_p(col), x_stride_elems=stride,
                              F=Fdim, target_row0=row0, target_ids_dev=_p(target_ids) if not slab else None,
                              num_targets=T, out_dev=_p(out), out_stride_elems=out.stride(0) if T > 1 else 0,
                              self_scale=float(self_scale))
    for p, v in enumerate(off):
        d.part_offsets[p] = v
    for p, v in enumerate(ptrs):
        d.x_parts_dev[p] = v or None
    with torch.cuda.device(dev):
        nat.check(L.spp_graph_agg_parts_forward(C.byref(d), C.c_void_p(workspace.data_ptr()), workspace.numel(),
                                                _stream()))
    return out


def graph_gat_chunk():
    """C_g of the softmax contract (include/spp.h): a row of at most C_g raw entries is one online softmax in CSR order,
    a longer row is chunks of C_g whose softmax states are merged in chunk order"""
    return int(nat.load().spp_graph_gat_chunk())


def graph_gat_workspace_bytes(num_targets):
    return int(nat.load().spp_graph_gat_workspace_bytes(int(num_targets)))


def _gat_forward(h, a_src, a_dst, rowptr, col, heads, negative_slope, relu, row0, target_ids, T, out, workspace):
    """spp_graph_gat_forward on checked arguments, into ``out`` [T, F] (rows of another matrix allowed)"""
    N, Fdim = h.shape
    d = nat.GraphGatDesc(x_elem=_ELEM[h.dtype], out_elem=_ELEM[out.dtype], heads=heads, relu=int(bool(relu)),
                         rowptr_dev=_p(rowptr), col_dev=_p(col), x_dev=_p(h),
                         x_stride_elems=h.stride(0) if N > 1 else Fdim, x_rows=N, F=Fdim, a_src_dev=_p(a_src),
                         a_dst_dev=_p(a_dst), target_row0=row0, target_ids_dev=_p(target_ids) if target_ids is not None else None,
                         num_targets=T, out_dev=_p(out), out_stride_elems=out.stride(0) if T > 1 else 0,
                         negative_slope=float(negative_slope))
    with torch.cuda.device(h.device):
        nat.check(nat.load().spp_graph_gat_forward(C.byref(d), C.c_void_p(workspace.data_ptr()), workspace.numel(),
                                                   _stream()))
    return out


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
    _check_graph(h, rowptr, col, what)
    N, Fdim = h.shape
    if not isinstance(heads, int) or heads < 1 or Fdim % heads != 0:
        raise ValueError(f"{what}: heads must be a positive int that divides F = {Fdim}, got {heads!r}")
    for name, t in (("a_src", a_src), ("a_dst", a_dst)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (N, heads) \
                or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor of shape [{N}, {heads}] (nodes, heads)")
        if t.requires_grad:
            raise RuntimeError(f"{what}: {name} requires grad, and inference is forward only (detach it)")
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
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
    else:
        if not isinstance(target_ids, torch.Tensor) or target_ids.dtype != torch.int64 or target_ids.dim() != 1 \
                or not target_ids.is_contiguous():
            raise ValueError(f"{what}: target_ids must be a contiguous 1-D int64 tensor")
        row0, T = -1, target_ids.numel()
    nat.require_device()
    tensors = [h, a_src, a_dst, rowptr, col] + ([target_ids] if not slab else []) \
        + ([workspace] if workspace is not None else [])
    if not all(t.is_cuda and t.device == h.device for t in tensors):
        raise ValueError(f"{what}: h, a_src, a_dst, rowptr, col, target_ids and workspace must live on one CUDA device")
    nbytes = graph_gat_workspace_bytes(T)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=h.device)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < nbytes:
        raise ValueError(f"{what}: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes")
    out = torch.empty((T, Fdim), dtype=out_dtype, device=h.device)
    return _gat_forward(h, a_src, a_dst, rowptr, col, heads, negative_slope, relu, row0, None if slab else target_ids,
                        T, out, workspace)


def _check_targets(what, N, row0, num_targets, target_ids):
    """(slab?, row0 or -1, T) of the two target forms: a slab inside the graph's N nodes, or a contiguous int64 list"""
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
        return True, row0, T
    if not isinstance(target_ids, torch.Tensor) or target_ids.dtype != torch.int64 or target_ids.dim() != 1 \
            or not target_ids.is_contiguous():
        raise ValueError(f"{what}: target_ids must be a contiguous 1-D int64 tensor")
    return False, -1, target_ids.numel()


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
    ptrs, stride, x_dtype, Fdim, dev = _parts_source(h_parts, off, dtype, F, what)
    if not isinstance(heads, int) or heads < 1 or Fdim % heads != 0:
        raise ValueError(f"{what}: heads must be a positive int that divides F = {Fdim}, got {heads!r}")
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
    N = off[-1]
    for name, t in (("rowptr", rowptr), ("col", col)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous 1-D int64 tensor")
    if rowptr.numel() != N + 1:
        raise ValueError(f"{what}: the parts hold {N} rows, the graph {rowptr.numel() - 1} nodes (one row per node)")
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
    slab, row0, T = _check_targets(what, N, row0, num_targets, target_ids)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != out_dtype or tuple(out.shape) != (T, Fdim) \
                or (Fdim > 1 and out.stride(1) != 1) or out.requires_grad:
            raise ValueError(f"{what}: out must be a {out_dtype} matrix of shape [{T}, {Fdim}] with unit column stride "
                             "that does not require grad")
    nat.require_device()
    dev = rowptr.device if dev is None else dev
    tensors = [rowptr, col] + [t for t in (None if slab else target_ids, workspace, out) if t is not None]
    if dev.type != "cuda" or not all(t.is_cuda and t.device == dev for t in tensors):
        raise ValueError(f"{what}: the parts, rowptr, col, target_ids, workspace and out must live on one CUDA device")
    L = nat.load()
    nbytes = int(L.spp_graph_gat_workspace_bytes(T))
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < nbytes:
        raise ValueError(f"{what}: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes")
    if out is None:
        out = torch.empty((T, Fdim), dtype=out_dtype, device=dev)
    d = nat.GraphGatPartsDesc(x_elem=_ELEM[x_dtype], out_elem=_ELEM[out_dtype], heads=heads, relu=int(bool(relu)),
                              num_parts=len(off) - 1, rowptr_dev=_p(rowptr), col_dev=_p(col), x_stride_elems=stride,
                              a_stride_elems=a_stride, F=Fdim, target_row0=row0,
                              target_ids_dev=_p(target_ids) if not slab else None, num_targets=T, out_dev=_p(out),
                              out_stride_elems=out.stride(0) if T > 1 else 0, negative_slope=float(negative_slope))
    for p, v in enumerate(off):
        d.part_offsets[p] = v
    for p, (hv, av) in enumerate(zip(ptrs, a_ptrs)):
        d.h_parts_dev[p], d.a_parts_dev[p] = hv or None, av or None
    with torch.cuda.device(dev):
        nat.check(L.spp_graph_gat_parts_forward(C.byref(d), C.c_void_p(workspace.data_ptr()), workspace.numel(),
                                                _stream()))
    return out


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
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (Cdim,) or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor of shape [{Cdim}] (one entry per column)")
        if t.requires_grad:
            raise RuntimeError(f"{what}: {name} requires grad, and inference is forward only (detach it)")
    if residual is None:
        if row0 is not None or row_ids is not None:
            raise ValueError(f"{what}: row0 / row_ids address the residual's rows, and there is no residual")
    else:
        _check_matrix(residual, what, "residual")
        if residual.size(1) != Cdim or residual.size(0) < 1:
            raise ValueError(f"{what}: residual must have z's {Cdim} columns and at least one row, got "
                             f"{tuple(residual.shape)}")
        if (row0 is None) == (row_ids is None):
            raise ValueError(f"{what}: address the residual's rows either as a slab (row0) or as row_ids"
                             + (", not both" if row0 is not None else ""))
        if row_ids is None:
            row0 = int(row0)
            if row0 < 0:
                raise ValueError(f"{what}: row0 must not be negative, got {row0}")
        elif not isinstance(row_ids, torch.Tensor) or row_ids.dtype != torch.int64 or tuple(row_ids.shape) != (n,) \
                or not row_ids.is_contiguous():
            raise ValueError(f"{what}: row_ids must be a contiguous int64 tensor of shape [{n}] (one entry per row of z)")
    if out is None:
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        if out_dtype not in _OUT_DTYPES:
            raise ValueError(f"{what}: out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
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


_GEMM_ROWS = 1 << 16


def _row_tiles(A):
    """(first row, rows, tile) over A in tiles of exactly _GEMM_ROWS rows, the last one zero-padded.  The library picks
    a GEMM kernel -- and with it the order of the sum over K -- by the problem's shape, so the same operand row can
    come out with different last bits from a [600, K] and a [75, K] product.  With one shape for every call a node's
    result depends on its own row alone: not on the slab size, and not on whether ``nodes`` selected it."""
    T = A.size(0)
    for r in range(0, T, _GEMM_ROWS):
        n = min(_GEMM_ROWS, T - r)
        tile = A[r:r + n]
        if n < _GEMM_ROWS:
            tile = A.new_zeros((_GEMM_ROWS, A.size(1)))
            tile[:n] = A[r:r + n]
        yield r, n, tile


def _sage_layer(conv, last, act_dtype):
    """(epilogue, self_scale, fn): fn maps a slab's fp32 / bf16 operand [T, 2K] to the layer's output rows"""
    W = torch.cat([conv.lin_l.weight, conv.lin_r.weight], dim=1).to(act_dtype)      # [N, 2K] = [W_l | W_r]
    bias = conv.lin_l.bias

    def fn(A):
        Z = A @ W.t()
        if bias is not None:
            Z = Z + bias.to(Z.dtype)
        return Z if last else torch.relu_(Z)             # the inter-layer ReLU; dropout is the identity in eval mode
    return "operand", 0.0, fn


def _gin_layer(conv, amp):
    def fn(h):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            return conv.nn(h)                            # Linear, BatchNorm1d (running statistics), ReLU, Linear, ReLU
    return "sum", conv._scale(), fn


def _gat_inference(model, x, rowptr, col, nodes, rows_per_slab, act_dtype):
    """layerwise_inference for GAT, in PyG's project-first order (training aggregates first, _GatLayer / _GatLayerMH,
    because an MFG hop has many sources per target; over the whole graph T = S = N, that saving is gone, and the
    aggregate-first intermediate would be [T, H, K] fp32 per slab).  Per layer:

      project    h = cur @ W^T for all N rows, [N, H*C] in ``act_dtype``, over ``_row_tiles``
      logits     [a_src | a_dst] = tile.float() @ V^T with V = W_h^T att (as _GatLayerMH builds it), fp32 [N, H] each:
                 taken from the layer's input rows, never from the rounded h
      aggregate  ``spp_graph_gat_forward`` slab by slab over each node's whole row; hidden layers through the fused ReLU
                 straight into the next [N, hidden] matrix, the last layer ([T, H*classes] fp32 per slab) through the
                 mean over its heads and log_softmax(dtype=float32)

    Memory, as arithmetic: ``cur`` is dropped once ``h`` is complete and ``h`` once ``nxt`` is, so two [N, hidden]
    matrices of ``act_dtype`` are live at a time, as for SAGE (57 GB each in bf16 at N = 111 M, hidden 256; layer 1's
    ``cur`` is the resident table and stays), plus the logits, 2 * N * H * 4 bytes (3.6 GB at H = 4).  The one case
    worse than SAGE: the last layer's h is [N, H * classes], so H > 1 heads multiply it -- 111 M * 4 * 172 * 2 bytes =
    153 GB in bf16 for H = 4 and 172 classes, which does not fit next to a 57 GB ``cur``, 26 GB of graph and 28 GB of
    features on one 288 GB MI355X.  The reference's model has H = 1 (38 GB)."""
    N, dev = x.size(0), x.device
    n_layers = len(model.convs)
    ws = torch.empty(graph_gat_workspace_bytes(min(rows_per_slab, max(N, nodes.numel() if nodes is not None else 0))),
                     dtype=torch.uint8, device=dev)
    cur = x
    for i, conv in enumerate(model.convs):
        last = i == n_layers - 1
        H, Cc = conv.heads, conv.out_channels
        W = conv.lin_src.weight                                                   # [H*C, K]
        att = torch.stack([conv.att_src.view(H, Cc), conv.att_dst.view(H, Cc)]).to(torch.float32)
        V = torch.einsum("shc,hck->shk", att, W.to(torch.float32).view(H, Cc, -1)).reshape(2 * H, -1)   # [V_src; V_dst]
        Wt, Vt = W.to(act_dtype).t(), V.t().contiguous()
        h = torch.empty((N, H * Cc), dtype=act_dtype, device=dev)
        a_src, a_dst = (torch.empty((N, H), dtype=torch.float32, device=dev) for _ in range(2))
        for r, n, tile in _row_tiles(cur):
            h[r:r + n] = (tile.to(act_dtype) @ Wt)[:n]
            a = tile.to(torch.float32) @ Vt
            a_src[r:r + n], a_dst[r:r + n] = a[:n, :H], a[:n, H:]
        del cur                                          # (layer i-1's matrix; layer 1's is the caller's table)
        ids = nodes if last else None
        rows = ids.numel() if ids is not None else N
        width = Cc if last else H * Cc
        nxt = torch.empty((rows, width), dtype=torch.float32 if last else act_dtype, device=dev)
        for s in range(0, rows, rows_per_slab):
            e = min(rows, s + rows_per_slab)
            row0, tids = (-1, ids[s:e]) if ids is not None else (s, None)
            out = nxt[s:e] if not last else torch.empty((e - s, H * Cc), dtype=torch.float32, device=dev)
            _gat_forward(h, a_src, a_dst, rowptr, col, H, conv.negative_slope, not last, row0, tids, e - s, out, ws)
            if last:                                     # concat=False: the mean of the heads (H = 1: the head itself)
                nxt[s:e] = torch.log_softmax(out.view(e - s, H, Cc).mean(1) if H > 1 else out, dim=-1,
                                             dtype=torch.float32)
        cur = nxt                                        # (drops h)
        del h, a_src, a_dst
    return cur


def _resinc_head(model):
    """the two bare Linears of SAGEResInception's MLP head (``end_up_with_fc=True``: no BatchNorm, no activation)"""
    mods = list(model.mlp.module_list)
    if len(mods) != 2 or not all(isinstance(m, torch.nn.Linear) for m in mods):
        raise NotImplementedError("layerwise_inference: SAGEResInception's head must be exactly two Linears (its first "
                                  "one is applied block by block, which needs it to be linear in the concatenation)")
    return mods


def _resinc_inference(model, x, rowptr, col, nodes, rows_per_slab, act_dtype):
    """layerwise_inference for SAGEResInception.  In eval mode dropout is the identity and the model is

      layer i    h_i = leaky_relu(BatchNorm_i([mean | h_{i-1}] @ [W_l | W_r]^T)) + res_i,   h_0 = x,
                 res_1 = res_linears[0](x), res_i = h_{i-1} after; per slab ``graph_aggregate`` ("operand"), per fixed
                 GEMM tile one product and one ``resinc_epilogue`` that writes the tile's rows of the next [N, hidden]
                 matrix.  Layer 1's residual Linear is stacked into the same product ([0 | W_res] below [W_l | W_r], so
                 the tile is [z | res]); later residuals are the rows of ``cur`` itself, read in place by slab or, on the
                 last layer with ``nodes``, by the id list.
      head       log_softmax(lin2(lin1(cat(x, h_1, .., h_L)))).  lin1 is a bare Linear, so lin1(cat(..)) is
                 bias + sum_k block_k @ W1[:, block k]^T: an fp32 accumulator ``acc`` [rows, 2 * classes] takes every
                 block's product when the block is complete, and no layer's matrix outlives the next layer.

    Memory, as arithmetic: two [N, hidden] matrices of ``act_dtype`` at a layer boundary, as for SAGE, plus ``acc``:
    4 * rows * 2 * classes bytes.  For all N = 111 M nodes and 172 classes that is 153 GB, which does not fit beside
    2 * 57 + 26 + 28 = 168 GB on one 288 GB MI355X: ``nodes=`` is the papers-scale form."""
    lin1, lin2 = _resinc_head(model)
    N, dev = x.size(0), x.device
    n_layers, hidden = len(model.convs), model.hidden_channels
    rows_out = nodes.numel() if nodes is not None else N
    ws = torch.empty(graph_agg_workspace_bytes(min(rows_per_slab, max(N, rows_out))), dtype=torch.uint8, device=dev)
    acc = torch.zeros((rows_out, lin1.out_features), dtype=torch.float32, device=dev)
    if lin1.bias is not None:
        acc += lin1.bias.to(torch.float32)

    def add_block(block, first_col):                     # acc += block @ W1[:, its columns]^T, over the fixed tiles
        Wb = lin1.weight[:, first_col:first_col + block.size(1)].to(act_dtype).t()
        for r, n, tile in _row_tiles(block):
            acc[r:r + n] += (tile.to(act_dtype) @ Wb)[:n]

    add_block(x if nodes is None else x[nodes], 0)
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
        rows = ids.numel() if ids is not None else N
        nxt = torch.empty((rows, hidden), dtype=act_dtype, device=dev)
        for s in range(0, rows, rows_per_slab):
            e = min(rows, s + rows_per_slab)
            tgt = dict(target_ids=ids[s:e]) if ids is not None else dict(row0=s, num_targets=e - s)
            A = graph_aggregate(cur, rowptr, col, epilogue="operand", out_dtype=act_dtype, workspace=ws, **tgt)
            for r, n, tile in _row_tiles(A):
                Z = torch.addmm(bias, tile, Wt) if bias is not None else tile @ Wt
                if Z.size(1) > hidden:
                    residual = dict(residual=Z[:, hidden:], row0=0)
                elif ids is not None:
                    residual = dict(residual=cur, row_ids=ids[s + r:s + r + n])
                else:
                    residual = dict(residual=cur, row0=s + r)
                resinc_epilogue(Z[:n, :hidden], a, b, negative_slope=0.01, out=nxt[s + r:s + r + n], **residual)
        add_block(nxt if last or nodes is None else nxt[nodes], x.size(1) + i * hidden)
        cur = nxt                                        # (drops layer i-1's matrix)
    W2t = lin2.weight.to(act_dtype).t()
    b2 = lin2.bias.to(act_dtype) if lin2.bias is not None else None
    out = torch.empty((rows_out, lin2.out_features), dtype=torch.float32, device=dev)
    for r, n, tile in _row_tiles(acc):
        h = tile.to(act_dtype)
        h = torch.addmm(b2, h, W2t) if b2 is not None else h @ W2t
        out[r:r + n] = torch.log_softmax(h[:n], dim=-1, dtype=torch.float32)
    return out


def _check_model_shape(model, what):
    """what the GAT and SAGEResInception drivers need of the model's layers (SAGE and GIN: nothing)"""
    from .models import GAT, SAGEResInception
    if isinstance(model, SAGEResInception):
        _resinc_head(model)
    if isinstance(model, GAT):                                # the layers as models.GAT builds them
        for i, c in enumerate(model.convs):
            mean_heads = i == len(model.convs) - 1 and c.heads > 1
            if c.bias is not None or c.concat == mean_heads:
                raise NotImplementedError(f"{what}: GAT layers need bias=False, and concat=False on the last layer of a "
                                          "multi-head model only")


def layerwise_inference(model, x, rowptr, col, *, nodes=None, rows_per_slab=1 << 20, act_dtype=torch.float32):
    """Exact log-probabilities of every node, [N, classes] fp32 -- or of ``nodes`` (int64, any order, duplicates
    allowed), [len(nodes), classes] -- for a ``SAGE``, ``GIN``, ``GAT`` or ``SAGEResInception`` model over the whole
    graph.  (GAT, at any ``heads``: see ``_gat_inference`` for its order of operations and memory; SAGEResInception:
    ``_resinc_inference``; what follows describes SAGE and GIN, and the arguments, the fixed GEMM tiles, eval mode and
    ``nodes`` mean the same for all four.)

    Layer by layer, slab by slab of ``rows_per_slab`` nodes: ``graph_aggregate`` over each node's whole neighbour row,
    then the layer's own parameters as torch GEMMs (SAGE: [mean | x] @ [W_l | W_r]^T; GIN: ``conv.nn`` with BatchNorm's
    running statistics), written -- SAGE: through the ReLU -- into the next [N, hidden] activation matrix of dtype
    ``act_dtype``.  The GEMMs run over row tiles of one fixed height, so a node's result is the same bits whatever the
    slab size and whether ``nodes`` selected it.  With ``act_dtype=torch.bfloat16`` operands, weights and activations are bf16 as under
    ``torch.autocast`` in training (fp32 sums, fp32 log_softmax).  With ``nodes`` the last conv layer, GIN's head and
    the log_softmax are computed for those nodes only.  The model is put in eval mode and its mode restored; nothing
    records a gradient.  ``x``: a CUDA fp16 / fp32 / bf16 matrix, one row per node, possibly a strided view of the
    resident table (``FastSampler.resident_graph()``).

    Memory, as arithmetic: an activation matrix is N * hidden * sizeof(act_dtype) bytes and two are live at a layer
    boundary (layer i-1's is freed as soon as layer i is complete).  At N = 111 M and hidden 256 that is 113 GB each in
    fp32 and 57 GB in bf16, next to 26 GB of graph and 28 GB of features: fp32 activations do not fit one 288 GB MI355X
    at papers scale, ``act_dtype=torch.bfloat16`` does (26 + 28 + 2 * 57 = 168 GB)."""
    from .models import GAT, GIN, SAGE, SAGEResInception
    what = "layerwise_inference"
    if not isinstance(model, (SAGE, GIN, GAT, SAGEResInception)):
        raise NotImplementedError(f"{what}: implemented for SAGE and GIN (and GAT, SAGEResInception), not "
                                  f"{type(model).__name__}")
    _check_model_shape(model, what)
    _check_matrix(x, what)
    _check_graph(x, rowptr, col, what)
    if act_dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: act_dtype must be torch.float32 or torch.bfloat16, got {act_dtype}")
    rows_per_slab = int(rows_per_slab)
    if rows_per_slab < 1:
        raise ValueError(f"{what}: rows_per_slab must be positive, got {rows_per_slab}")
    if nodes is not None and (not isinstance(nodes, torch.Tensor) or nodes.dtype != torch.int64 or nodes.dim() != 1):
        raise ValueError(f"{what}: nodes must be a 1-D int64 tensor")
    nat.require_device()
    if not (x.is_cuda and rowptr.device == x.device and col.device == x.device):
        raise ValueError(f"{what}: x, rowptr and col must live on one CUDA device")
    N = x.size(0)
    if nodes is not None:
        nodes = nodes.to(x.device).contiguous()
        if nodes.numel() and not (0 <= int(nodes.min()) and int(nodes.max()) < N):      # (one read-back, up front)
            raise ValueError(f"{what}: nodes outside the graph's {N} nodes")
    amp = act_dtype == torch.bfloat16
    gin = isinstance(model, GIN)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            if isinstance(model, GAT):
                return _gat_inference(model, x, rowptr, col, nodes, rows_per_slab, act_dtype)
            if isinstance(model, SAGEResInception):
                return _resinc_inference(model, x, rowptr, col, nodes, rows_per_slab, act_dtype)
            n_layers = len(model.convs)
            ws = torch.empty(graph_agg_workspace_bytes(min(rows_per_slab, max(N, nodes.numel() if nodes is not None else 0))),
                             dtype=torch.uint8, device=x.device)

            def head(h):                                 # what follows the last conv layer, fp32 log-probabilities
                if gin:
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                        h = model.lin2(torch.relu(model.lin1(h)))
                return torch.log_softmax(h, dim=-1, dtype=torch.float32)

            cur = x
            for i, conv in enumerate(model.convs):
                last = i == n_layers - 1
                epilogue, scale, fn = _gin_layer(conv, amp) if gin else _sage_layer(conv, last, act_dtype)
                ids = nodes if last else None
                rows = ids.numel() if ids is not None else N
                nxt = None
                for s in range(0, rows, rows_per_slab):
                    e = min(rows, s + rows_per_slab)
                    tgt = dict(target_ids=ids[s:e]) if ids is not None else dict(row0=s, num_targets=e - s)
                    A = graph_aggregate(cur, rowptr, col, epilogue=epilogue, self_scale=scale, out_dtype=act_dtype,
                                        workspace=ws, **tgt)
                    for r, n, tile in _row_tiles(A):
                        h = head(fn(tile)) if last else fn(tile)
                        if nxt is None:
                            nxt = torch.empty((rows, h.size(1)), dtype=torch.float32 if last else act_dtype,
                                              device=x.device)
                        nxt[s + r:s + r + n] = h[:n]
                if nxt is None:                          # no rows at all
                    width = (model.lin2 if gin else conv.lin_l).out_features if last else model.hidden_channels
                    nxt = torch.empty((0, width), dtype=torch.float32 if last else act_dtype, device=x.device)
                cur = nxt                                # (drops layer i-1's matrix)
            return cur
    finally:
        model.train(was_training)


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


def _check_partitioned(what, x_local, rowptr, col, part_offsets, rank, peers, nodes, rows_per_slab, act_dtype):
    """the arguments every partitioned driver shares, checked before ``peers`` is touched; the device is required last.
    Returns (offsets as a list, rank, nodes on the device or None, rows_per_slab)"""
    _check_matrix(x_local, what, "x_local")
    off = _check_offsets(part_offsets, what)
    P = len(off) - 1
    rank = int(rank)
    if not 0 <= rank < P:
        raise ValueError(f"{what}: rank {rank} outside the {P} parts")
    lo, hi = off[rank], off[rank + 1]
    n_local, N = hi - lo, off[-1]
    if x_local.size(0) != n_local:
        raise ValueError(f"{what}: x_local has {x_local.size(0)} rows, part_offsets gives rank {rank} {n_local}")
    for name, t in (("rowptr", rowptr), ("col", col)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous 1-D int64 tensor")
    if rowptr.numel() != N + 1:
        raise ValueError(f"{what}: the parts hold {N} rows, the graph {rowptr.numel() - 1} nodes (one row per node)")
    if act_dtype not in _OUT_DTYPES:
        raise ValueError(f"{what}: act_dtype must be torch.float32 or torch.bfloat16, got {act_dtype}")
    rows_per_slab = int(rows_per_slab)
    if rows_per_slab < 1:
        raise ValueError(f"{what}: rows_per_slab must be positive, got {rows_per_slab}")
    if nodes is not None:
        if not isinstance(nodes, torch.Tensor) or nodes.dtype != torch.int64 or nodes.dim() != 1:
            raise ValueError(f"{what}: nodes must be a 1-D int64 tensor")
        if nodes.numel() and not (lo <= int(nodes.min()) and int(nodes.max()) < hi):     # (one read-back, up front)
            raise ValueError(f"{what}: nodes outside rank {rank}'s range [{lo}, {hi}) (global ids; every rank scores its own)")
    for name in ("share", "barrier", "close"):
        if not callable(getattr(peers, name, None)):
            raise TypeError(f"{what}: peers must provide share(tensor), barrier() and close()")
    nat.require_device()
    dev = x_local.device
    if not (x_local.is_cuda and rowptr.device == dev and col.device == dev):
        raise ValueError(f"{what}: x_local, rowptr and col must live on one CUDA device")
    if nodes is not None:
        nodes = nodes.to(dev).contiguous()
    return off, rank, nodes, rows_per_slab


def partitioned_layerwise_inference(model, x_local, rowptr, col, *, part_offsets, rank, peers, nodes=None,
                                    rows_per_slab=1 << 20, act_dtype=torch.float32):
    """``layerwise_inference`` for SAGE and GIN when the feature table is row-partitioned over the ranks: every rank calls
    this with its own partition ``x_local`` (the global rows [part_offsets[rank], part_offsets[rank + 1])), the WHOLE
    graph's CSR (global ids) and the same ``model``, and gets the fp32 log-probabilities of ITS node range,
    [n_local, classes] -- or of ``nodes`` (global ids, all inside the rank's range).  The bits are those of
    ``layerwise_inference`` over the concatenated table, rows [part_offsets[rank], part_offsets[rank + 1]).

    Per rank: the ping-pong activation buffers [n_local, hidden] of ``act_dtype`` are allocated up front (one for a
    two-layer model) and published with ``x_local`` once through ``peers``; each layer aggregates the rank's own slabs with
    ``graph_aggregate_parts`` over ALL ranks' previous-layer parts, runs the layer's parameters over the same fixed GEMM
    tiles as ``layerwise_inference`` and writes its rows of the next layer into its own buffer; then the rank synchronises
    its stream and waits in ``peers.barrier()`` before anyone reads the layer or reuses a buffer.  After the last barrier
    the mappings are closed.

    ``peers``: ``share(tensor) -> P2PPeers`` (collective, same order on every rank), ``barrier()``, ``close()``; optional
    ``bind(rank)`` and ``abort()``.  ``LocalPeers`` and ``IpcPeers`` are the two implementations.  GAT and
    SAGEResInception are refused here and scored by ``partitioned_inference``, the entry for all four models.

    Memory, as arithmetic (S-mag, N = 121.8 M, F = 768 fp16, hidden 256, bf16): per rank of P, 187 / P GB of table and
    2 * 62 / P GB of activations next to its copy of the 22 GB graph."""
    from .models import GAT, GIN, SAGE, SAGEResInception
    what = "partitioned_layerwise_inference"
    if isinstance(model, (GAT, SAGEResInception)):
        raise NotImplementedError(f"{what}: {type(model).__name__} over a partitioned table is not scored by this entry "
                                  "(its layers need the long-row softmax / the fused layer tail over parts); SAGE and GIN "
                                  "are.  partitioned_inference scores all four models")
    if not isinstance(model, (SAGE, GIN)):
        raise NotImplementedError(f"{what}: implemented for SAGE and GIN, not {type(model).__name__}")
    off, rank, nodes, rows_per_slab = _check_partitioned(what, x_local, rowptr, col, part_offsets, rank, peers, nodes,
                                                         rows_per_slab, act_dtype)
    lo, n_local, dev = off[rank], off[rank + 1] - off[rank], x_local.device
    amp = act_dtype == torch.bfloat16
    gin = isinstance(model, GIN)
    n_layers, hidden = len(model.convs), model.hidden_channels
    was_training = model.training
    model.eval()
    shared = []
    try:
        with torch.no_grad(), torch.autocast("cuda", enabled=False), torch.cuda.device(dev):
            if hasattr(peers, "bind"):
                peers.bind(rank)
            # the buffers follow the resident tables' row-stride rule, so that every rank's have one stride whatever its
            # row count (a one-row part has no stride of its own)
            esize = torch.empty(0, dtype=act_dtype).element_size()
            se = _row_stride_elems(hidden, esize)
            bufs = [torch.empty((n_local, se), dtype=act_dtype, device=dev)[:, :hidden] for _ in range(min(2, n_layers - 1))]
            shared = [(peers.share(x_local), x_local.dtype, x_local.size(1))]
            shared += [(peers.share(b), act_dtype, hidden) for b in bufs]
            rows_out = nodes.numel() if nodes is not None else n_local
            ws = torch.empty(graph_agg_workspace_bytes(min(rows_per_slab, max(n_local, rows_out))), dtype=torch.uint8,
                             device=dev)

            def head(h):                                 # what follows the last conv layer, fp32 log-probabilities
                if gin:
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                        h = model.lin2(torch.relu(model.lin1(h)))
                return torch.log_softmax(h, dim=-1, dtype=torch.float32)

            result = None
            for i, conv in enumerate(model.convs):
                last = i == n_layers - 1
                epilogue, scale, fn = _gin_layer(conv, amp) if gin else _sage_layer(conv, last, act_dtype)
                src, src_dtype, src_F = shared[0] if i == 0 else shared[1 + (i - 1) % len(bufs)]
                ids = nodes if last else None
                rows = ids.numel() if ids is not None else n_local
                nxt = None if last else bufs[i % len(bufs)]
                for s in range(0, rows, rows_per_slab):
                    e = min(rows, s + rows_per_slab)
                    tgt = dict(target_ids=ids[s:e]) if ids is not None else dict(row0=lo + s, num_targets=e - s)
                    A = graph_aggregate_parts(src, off, rowptr, col, dtype=src_dtype, F=src_F, epilogue=epilogue,
                                              self_scale=scale, out_dtype=act_dtype, workspace=ws, **tgt)
                    for r, n, tile in _row_tiles(A):
                        h = head(fn(tile)) if last else fn(tile)
                        if nxt is None:
                            nxt = torch.empty((rows, h.size(1)), dtype=torch.float32, device=dev)
                        nxt[s + r:s + r + n] = h[:n]
                if last:
                    if nxt is None:                      # no rows at all
                        width = (model.lin2 if gin else conv.lin_l).out_features
                        nxt = torch.empty((0, width), dtype=torch.float32, device=dev)
                    result = nxt
                # layer i is complete HERE before any rank reads it, and every rank has finished reading layer i-1 before
                # its buffer is written again (after the last layer: before anyone unmaps)
                torch.cuda.current_stream(dev).synchronize()
                peers.barrier()
            return result
    except BaseException:
        if hasattr(peers, "abort"):
            peers.abort()
        raise
    finally:
        for sh, _dt, _f in shared:
            sh.close()
        model.train(was_training)


def _tiles_contiguous(A):
    """``_row_tiles`` with every tile contiguous: a full tile of a padded buffer is a strided view, and the GEMM's
    operand layout is part of its shape (the whole-table drivers multiply contiguous matrices)"""
    for r, n, tile in _row_tiles(A):
        yield r, n, tile.contiguous()


def _gat_partitioned(model, x_local, rowptr, col, off, rank, peers, nodes, rows_per_slab, act_dtype, shared):
    """``_gat_inference`` for one rank of a row-partitioned table: the same operations on the same fixed tiles, so the
    same bits.  Projection and logits are LOCAL (a rank's own rows of the layer's input), so no rank reads a peer's
    feature rows and ``x_local`` is not published.  Two buffers are, once: h [n_local, max H*C] of ``act_dtype`` and the
    logits [n_local, 2 * max H] fp32 = [a_src | a_dst], both laid out by the resident tables' row-stride rule (one stride
    on every rank); a layer narrower than the buffer reads its leading columns at the buffer's stride.  Per layer: write
    the rank's h and logits; synchronise and barrier (every rank's h is complete); attend the rank's slabs with
    ``graph_gat_aggregate_parts`` over all ranks' parts into a local matrix; synchronise and barrier (everyone has
    finished reading h before the next layer overwrites it, or, after the last layer, before anyone unmaps)."""
    lo, dev = off[rank], x_local.device
    n_local = off[rank + 1] - lo
    n_layers = len(model.convs)
    Fmax = max(c.heads * c.out_channels for c in model.convs)
    Hmax = max(c.heads for c in model.convs)
    esize = torch.empty(0, dtype=act_dtype).element_size()
    hbuf = torch.empty((n_local, _row_stride_elems(Fmax, esize)), dtype=act_dtype, device=dev)[:, :Fmax]
    abuf = torch.empty((n_local, _row_stride_elems(2 * Hmax, 4)), dtype=torch.float32, device=dev)[:, :2 * Hmax]
    shared.append(peers.share(hbuf))
    shared.append(peers.share(abuf))
    h_peers, a_peers = shared
    rows_out = nodes.numel() if nodes is not None else n_local
    ws = torch.empty(graph_gat_workspace_bytes(min(rows_per_slab, max(n_local, rows_out))), dtype=torch.uint8, device=dev)
    cur = x_local
    for i, conv in enumerate(model.convs):
        last = i == n_layers - 1
        H, Cc = conv.heads, conv.out_channels
        W = conv.lin_src.weight                                                   # [H*C, K]
        att = torch.stack([conv.att_src.view(H, Cc), conv.att_dst.view(H, Cc)]).to(torch.float32)
        V = torch.einsum("shc,hck->shk", att, W.to(torch.float32).view(H, Cc, -1)).reshape(2 * H, -1)   # [V_src; V_dst]
        Wt, Vt = W.to(act_dtype).t(), V.t().contiguous()
        for r, n, tile in _row_tiles(cur):
            hbuf[r:r + n, :H * Cc] = (tile.to(act_dtype) @ Wt)[:n]
            abuf[r:r + n, :2 * H] = (tile.to(torch.float32) @ Vt)[:n]
        del cur
        torch.cuda.current_stream(dev).synchronize()
        peers.barrier()                                  # every rank's h and logits of this layer are complete
        ids = nodes if last else None
        rows = ids.numel() if ids is not None else n_local
        width = Cc if last else H * Cc
        nxt = torch.empty((rows, width), dtype=torch.float32 if last else act_dtype, device=dev)
        for s in range(0, rows, rows_per_slab):
            e = min(rows, s + rows_per_slab)
            tgt = dict(target_ids=ids[s:e]) if ids is not None else dict(row0=lo + s, num_targets=e - s)
            out = nxt[s:e] if not last else torch.empty((e - s, H * Cc), dtype=torch.float32, device=dev)
            graph_gat_aggregate_parts(h_peers, a_peers, off, rowptr, col, heads=H, negative_slope=conv.negative_slope,
                                      relu=not last, out_dtype=out.dtype, out=out, workspace=ws, dtype=act_dtype,
                                      F=H * Cc, **tgt)
            if last:                                     # concat=False: the mean of the heads (H = 1: the head itself)
                nxt[s:e] = torch.log_softmax(out.view(e - s, H, Cc).mean(1) if H > 1 else out, dim=-1,
                                             dtype=torch.float32)
        cur = nxt
        torch.cuda.current_stream(dev).synchronize()
        peers.barrier()                                  # every rank has finished reading this layer's h
    return cur


def _resinc_partitioned(model, x_local, rowptr, col, off, rank, peers, nodes, rows_per_slab, act_dtype, shared):
    """``_resinc_inference`` for one rank of a row-partitioned table.  ``x_local`` and the ping-pong [n_local, hidden]
    buffers are published once; each layer aggregates with ``graph_aggregate_parts`` ("operand") over all ranks' parts,
    and everything behind the aggregation is local: the GEMM tiles, ``resinc_epilogue`` (the residual of layers >= 2 is
    the rank's OWN previous buffer, by local slab or by ``ids - lo``), the head accumulator.  One synchronise and barrier
    per layer."""
    lin1, lin2 = _resinc_head(model)
    lo, dev = off[rank], x_local.device
    n_local = off[rank + 1] - lo
    n_layers, hidden = len(model.convs), model.hidden_channels
    esize = torch.empty(0, dtype=act_dtype).element_size()
    se = _row_stride_elems(hidden, esize)
    bufs = [torch.empty((n_local, se), dtype=act_dtype, device=dev)[:, :hidden] for _ in range(min(2, n_layers - 1))]
    shared.append(peers.share(x_local))
    for b in bufs:
        shared.append(peers.share(b))
    rows_out = nodes.numel() if nodes is not None else n_local
    local = nodes - lo if nodes is not None else None    # the rank's own rows of ``nodes``
    ws = torch.empty(graph_agg_workspace_bytes(min(rows_per_slab, max(n_local, rows_out))), dtype=torch.uint8, device=dev)
    acc = torch.zeros((rows_out, lin1.out_features), dtype=torch.float32, device=dev)
    if lin1.bias is not None:
        acc += lin1.bias.to(torch.float32)

    def add_block(block, first_col):                     # acc += block @ W1[:, its columns]^T, over the fixed tiles
        Wb = lin1.weight[:, first_col:first_col + block.size(1)].to(act_dtype).t()
        for r, n, tile in _tiles_contiguous(block):
            acc[r:r + n] += (tile.to(act_dtype) @ Wb)[:n]

    add_block(x_local if local is None else x_local[local], 0)
    cur = x_local
    for i, (conv, bn) in enumerate(zip(model.convs, model.bns)):
        last = i == n_layers - 1
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
        src = shared[0] if i == 0 else shared[1 + (i - 1) % len(bufs)]
        ids = nodes if last else None
        rows = ids.numel() if ids is not None else n_local
        nxt = torch.empty((rows, hidden), dtype=act_dtype, device=dev) if last else bufs[i % len(bufs)]
        for s in range(0, rows, rows_per_slab):
            e = min(rows, s + rows_per_slab)
            tgt = dict(target_ids=ids[s:e]) if ids is not None else dict(row0=lo + s, num_targets=e - s)
            A = graph_aggregate_parts(src, off, rowptr, col, dtype=cur.dtype, F=cur.size(1), epilogue="operand",
                                      out_dtype=act_dtype, workspace=ws, **tgt)
            for r, n, tile in _row_tiles(A):
                Z = torch.addmm(bias, tile, Wt) if bias is not None else tile @ Wt
                if Z.size(1) > hidden:
                    residual = dict(residual=Z[:, hidden:], row0=0)
                elif ids is not None:
                    residual = dict(residual=cur, row_ids=local[s + r:s + r + n])
                else:
                    residual = dict(residual=cur, row0=s + r)
                resinc_epilogue(Z[:n, :hidden], a, b, negative_slope=0.01, out=nxt[s + r:s + r + n], **residual)
        add_block(nxt if last or local is None else nxt[local], x_local.size(1) + i * hidden)
        cur = nxt
        # layer i is complete HERE before any rank reads it, and every rank has finished reading layer i-1 before its
        # buffer is written again (after the last layer: before anyone unmaps)
        torch.cuda.current_stream(dev).synchronize()
        peers.barrier()
    W2t = lin2.weight.to(act_dtype).t()
    b2 = lin2.bias.to(act_dtype) if lin2.bias is not None else None
    out = torch.empty((rows_out, lin2.out_features), dtype=torch.float32, device=dev)
    for r, n, tile in _row_tiles(acc):
        h = tile.to(act_dtype)
        h = torch.addmm(b2, h, W2t) if b2 is not None else h @ W2t
        out[r:r + n] = torch.log_softmax(h[:n], dim=-1, dtype=torch.float32)
    return out


def partitioned_inference(model, x_local, rowptr, col, *, part_offsets, rank, peers, nodes=None, rows_per_slab=1 << 20,
                          act_dtype=torch.float32):
    """``layerwise_inference`` for ``SAGE``, ``GIN``, ``GAT`` and ``SAGEResInception`` when the feature table is
    row-partitioned over the ranks.  Every rank calls this with its own partition ``x_local`` (the global rows
    [part_offsets[rank], part_offsets[rank + 1])), the WHOLE graph's CSR (global ids) and the same ``model``, and gets the
    fp32 log-probabilities of ITS node range, [n_local, classes] -- or of ``nodes`` (global ids, all inside the rank's
    range).  The bits are those of ``layerwise_inference`` over the concatenated table, those rows.

    SAGE and GIN: ``partitioned_layerwise_inference``, whose arguments, ``peers`` protocol and failure rule (``abort()``
    when a rank fails, ``close()`` of every mapping at the end) hold here.  GAT: ``_gat_partitioned`` (local projection,
    h and logits published once, two barriers a layer); SAGEResInception: ``_resinc_partitioned`` (one barrier a layer).
    The model-shape refusals are ``layerwise_inference``'s, and like every argument check they come before ``peers`` is
    touched.

    Memory per rank of P, as arithmetic (GAT at papers scale: N = 111 M, hidden 256, 172 classes, H = 1, bf16, P = 8, so
    13.9 M rows a rank): the h buffer 13.9 M * 256 * 2 B = 7.1 GB and the logits 13.9 M * 8 B = 0.11 GB, both live for the
    whole call; one [n_local, 256] bf16 activation matrix at a time beside them (``cur`` while a layer projects, ``nxt``
    while it attends), 7.1 GB; the last layer's [n_local, 172] fp32 result, 9.5 GB; 3.6 GB of table and the rank's copy
    of the 26 GB graph: about 47 GB at the peak, against 168 GB on one device."""
    from .models import GAT, GIN, SAGE, SAGEResInception
    what = "partitioned_inference"
    if not isinstance(model, (SAGE, GIN, GAT, SAGEResInception)):
        raise NotImplementedError(f"{what}: implemented for SAGE, GIN, GAT and SAGEResInception, not "
                                  f"{type(model).__name__}")
    if isinstance(model, (SAGE, GIN)):
        return partitioned_layerwise_inference(model, x_local, rowptr, col, part_offsets=part_offsets, rank=rank,
                                               peers=peers, nodes=nodes, rows_per_slab=rows_per_slab, act_dtype=act_dtype)
    _check_model_shape(model, what)
    off, rank, nodes, rows_per_slab = _check_partitioned(what, x_local, rowptr, col, part_offsets, rank, peers, nodes,
                                                         rows_per_slab, act_dtype)
    dev = x_local.device
    run = _gat_partitioned if isinstance(model, GAT) else _resinc_partitioned
    was_training = model.training
    model.eval()
    shared = []
    try:
        with torch.no_grad(), torch.autocast("cuda", enabled=False), torch.cuda.device(dev):
            if hasattr(peers, "bind"):
                peers.bind(rank)
            return run(model, x_local, rowptr, col, off, rank, peers, nodes, rows_per_slab, act_dtype, shared)
    except BaseException:
        if hasattr(peers, "abort"):
            peers.abort()
        raise
    finally:
        for sh in shared:
            sh.close()
        model.train(was_training)
