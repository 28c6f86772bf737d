"""Model-step fallback for boxes without PyG / torch_sparse: the reference's flagship
``SAGE`` (driver/models.py:19-56: ``num_layers`` x SAGEConv(bias=False, mean aggregation), ReLU +
dropout 0.5 between layers, log_softmax) on the MFG's CSR, with the message passing on HIP kernels
(csrc/aggregate.hip) and the linear layers on the library GEMMs torch dispatches to.  The reference's other working
models follow: GAT (csrc/gat.hip), GIN (sum aggregation) and SAGEResInception; ``get_model_type`` maps their names (driver/main.py:74-95).

The constructor, ``reset_parameters`` and ``forward(x, adjs)`` follow the reference; ``adjs`` is
what the data path delivers: ``[(adj_t, e_id, (S, T)), ...]``, outermost hop first."""
import contextlib
import ctypes as C

import torch
import torch.nn.functional as F

from . import _native as nat
from .fast_sampler import RowRefs, TableRows
from .fp8 import Fp8Features


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None


def _stream():
    # the raw handle of the current stream of the current device (torch.cuda.current_stream() builds a Stream object: 5 us)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


# ---- bf16 mixed precision (torch.autocast("cuda", dtype=torch.bfloat16)) ----
# Under bf16 autocast the HIP nodes store activations, operands and activation gradients in bf16, run their GEMMs in
# bf16 (fp32 accumulation) and keep parameters and parameter gradients fp32.  The aggregation kernels accumulate in fp32
# and round every stored element once (include/spp.h, spp_agg_forward).  Under any other autocast dtype the nodes run
# their fp32 path with autocast disabled inside them.  Each node decides in its forward and records the decision on
# ctx; its backward uses explicit dtypes only.  The mean / operand / sum aggregations take one call path for every
# element type and row source: the descriptor entries spp_agg_forward, spp_agg_forward_fp8 and spp_agg_backward
# (_agg_forward, _agg_backward below), with the compute dtype as a value.
_ELEM = {torch.float32: nat.SPP_ELEM_F32, torch.float16: nat.SPP_ELEM_F16, torch.bfloat16: nat.SPP_ELEM_BF16}


def amp_bf16():
    """True when the HIP nodes take their bf16 path: CUDA autocast is on with dtype bfloat16"""
    return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16


def _no_autocast():
    return torch.autocast("cuda", enabled=False) if torch.is_autocast_enabled("cuda") else contextlib.nullcontext()


def _draw_seed():
    """a 64-bit seed for the kernels' counter-based dropout from torch's CPU generator (one draw): torch.manual_seed
    makes a run repeatable.  Called only where a mask is needed (training, p > 0)."""
    return int(torch.empty((), dtype=torch.int64).random_().item()) & 0xFFFFFFFFFFFFFFFF


_attn_seed = _draw_seed            # the name the attention layers draw through: their tests replace it to plant a seed


def _call_drop(L, name, args, drop):
    """the entry `name`, or with attention dropout (drop = (p, seed)) its _drop spelling, which takes (p, training = 1,
    seed) after the same arguments: the one place that picks between the two"""
    if drop:
        nat.check(getattr(L, name + "_drop")(*args, drop[0], 1, drop[1]))
    else:
        nat.check(getattr(L, name)(*args))


def _is_prefix(x, x_target):
    """x_target starts where x starts with x's strides (x[:T], the MFG contract); a call site that needs the widths
    to agree or T <= S says so itself"""
    return x_target.data_ptr() == x.data_ptr() and x_target.stride() == x.stride()


_GATHER_MIN_WORK = 1 << 22         # E x F from which an aggregation's input gradient is gathered over the transposed hop
_ATTN_HEADS = (1, 2, 4, 8)         # the head counts the GAT, GATv2 and Transformer kernels are built for


class _Refs:
    """RowRefs on their way through _SageStack.apply (a non-tensor argument)"""
    __slots__ = ("r",)

    def __init__(self, r):
        self.r = r


def _rows(x):
    """The row-source fields of spp_agg_fwd_desc (include/spp.h) for x, and the fp8 column exponents (None for fp32 /
    fp16 / bf16 rows).  x: a dense matrix or Fp8Features, a TableRows over either, a RowRefs, or what _SageStack.apply
    receives in their place (the tuple (table, n_id), a _Refs)."""
    if isinstance(x, _Refs):
        x = x.r
    if isinstance(x, RowRefs):                           # batch row j = the row at address addr[j]
        return dict(source=nat.SPP_AGG_ROWS, x_elem=_ELEM[x.dtype], n_id_dev=_p(x.addr), F=x.width), None
    n_id = exps = None
    if isinstance(x, TableRows):                         # batch row j = table[n_id[j]]
        x, n_id = x.table, x.n_id
    elif isinstance(x, tuple):
        x, n_id = x
    if isinstance(x, Fp8Features):                       # one byte per element, the column scales applied on load
        x, exps, elem = x.q, x.scale_log2, nat.SPP_ELEM_FP8_E4M3
    else:
        elem = _ELEM[x.dtype]
    rows, Fdim = x.shape
    return dict(source=nat.SPP_AGG_DENSE if n_id is None else nat.SPP_AGG_TABLE, x_elem=elem, x_dev=_p(x),
                x_stride_elems=x.stride(0) if rows > 1 else Fdim, x_rows=rows if n_id is not None else 0,
                n_id_dev=_p(n_id), F=Fdim), exps


def _is_fp8(x):
    """x is a dense Fp8Features, or a TableRows / (table, n_id) over one"""
    if isinstance(x, TableRows):
        x = x.table
    elif isinstance(x, tuple):
        x = x[0]
    return isinstance(x, Fp8Features)


def _agg_forward(epilogue, rowptr, col, T, x, out_dtype, *, scale=0.0, act=(0.0, 0, 0), st=None):
    """spp_agg_forward (spp_agg_forward_fp8 for fp8 rows) over the row source x (see _rows): the new dense [T, F or 2F]
    fp32 / bf16 result"""
    src, exps = _rows(x)
    width = src["F"] if epilogue in (nat.SPP_AGG_MEAN, nat.SPP_AGG_SUM) else 2 * src["F"]
    out = torch.empty((T, width), dtype=out_dtype, device=rowptr.device)
    d = nat.AggFwdDesc(epilogue=epilogue, out_elem=_ELEM[out_dtype], rowptr_dev=_p(rowptr), col_dev=_p(col),
                       num_targets=T, out_dev=_p(out), out_stride_elems=0, self_scale=float(scale), p=float(act[0]),
                       training=int(act[1]), seed=int(act[2]) & (2 ** 64 - 1), **src)
    L = nat.load()
    st = st if st is not None else _stream()
    nat.check(L.spp_agg_forward(C.byref(d), st) if exps is None else L.spp_agg_forward_fp8(C.byref(d), _p(exps), st))
    return out


def _agg_backward(epilogue, rowptr, col, T, S, g, Fdim, out_dtype, *, gather, z=None, scale=0.0, act=(0.0, 0, 0),
                  st=None):
    """spp_agg_backward: g [T, F or 2F] (unit column stride) -> the new dense grad_x [S, F]; the workspace is allocated
    here.  gather: over the transposed hop (built by the entry: count, scan, fill) instead of E x F fp32 atomics."""
    L = nat.load()
    E = col.numel()
    grad_x = torch.empty((S, Fdim), dtype=out_dtype, device=g.device)
    if gather:
        nbytes = int(L.spp_sage_operand_backward_workspace_bytes(T, S, E))
    else:
        nbytes = 4 * S * Fdim if out_dtype != torch.float32 else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device) if nbytes else None
    d = nat.AggBwdDesc(form=nat.SPP_AGG_GATHER if gather else nat.SPP_AGG_SCATTER, epilogue=epilogue,
                       grad_elem=_ELEM[g.dtype], out_elem=_ELEM[out_dtype],
                       z_elem=_ELEM[z.dtype] if z is not None else nat.SPP_ELEM_F32, rowptr_dev=_p(rowptr),
                       col_dev=_p(col), num_targets=T, num_sources=S, num_edges=E, grad_out_dev=_p(g),
                       grad_out_stride_elems=g.stride(0) if T > 1 else 0, F=Fdim, grad_x_dev=_p(grad_x), z_dev=_p(z),
                       self_scale=float(scale), p=float(act[0]), training=int(act[1]), seed=int(act[2]) & (2 ** 64 - 1))
    nat.check(L.spp_agg_backward(C.byref(d), _p(ws), nbytes, st if st is not None else _stream()))
    return grad_x


def _no_input_grad(ctx, what):
    # an fp8 table is no leaf: nothing flows back into it (the first layer's input gets no gradient)
    if ctx.needs_input_grad[0]:
        raise RuntimeError(f"{what}: an fp8 feature table cannot receive a gradient")


def _grad_in(g):
    """an incoming gradient as the descriptor entries read it: unit column stride, fp32 or bf16"""
    if g.dtype not in (torch.float32, torch.bfloat16):
        g = g.float()
    return g if g.stride(1) == 1 else g.contiguous()


class _MeanAggregate(torch.autograd.Function):
    """out[t] = mean_{e in row t} x[col[e]]  (empty rows give 0, as PyG's mean aggregation).

    With ``concat_target`` the result is the fused operand ``[mean | x_target]`` of shape [T, 2F] (fp32)
    where x_target = x[:T] (the MFG contract, driver/models.py:44-45): both halves are written by the
    one kernel, so lin_l and lin_r become ONE GEMM, and the backward writes grad_x completely (target
    half's gradient, zeros, scattered mean gradient) instead of autograd zero-padding the slice's
    gradient and adding two full-size tensors."""

    @staticmethod
    def forward(ctx, x, rowptr, col, num_targets, concat_target):
        nat.require_device()
        assert x.is_cuda and _readable(x), "fp16 / fp32 / bf16 / fp8 rows on the GPU"
        if _is_fp8(x):
            _no_input_grad(ctx, "mean_aggregate")
        out = _agg_forward(nat.SPP_AGG_OPERAND if concat_target else nat.SPP_AGG_MEAN, rowptr, col, num_targets, x,
                           torch.bfloat16 if amp_bf16() else torch.float32)
        ctx.save_for_backward(rowptr, col)
        ctx.shape = (x.size(0), x.size(1), num_targets)
        ctx.in_dtype = x.dtype
        ctx.concat = bool(concat_target)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        rowptr, col = ctx.saved_tensors
        S, Fdim, T = ctx.shape
        # bf16 / fp32 gradient in, the input's dtype out (fp16 through an fp32 buffer)
        g = _grad_in(grad_out)
        odt = ctx.in_dtype if ctx.in_dtype in (torch.float32, torch.bfloat16) else torch.float32
        vec = Fdim % 4 == 0 and (T <= 1 or g.stride(0) % 4 == 0) and g.data_ptr() % (4 * g.element_size()) == 0
        if ctx.concat and vec:
            grad_x = _agg_backward(nat.SPP_AGG_OPERAND, rowptr, col, T, S, g, Fdim, odt,
                                   gather=col.numel() * Fdim >= _GATHER_MIN_WORK)
        else:
            grad_x = _agg_backward(nat.SPP_AGG_MEAN, rowptr, col, T, S, g if not ctx.concat else g[:, :Fdim], Fdim, odt,
                                   gather=False)
            if ctx.concat:
                grad_x[:T] += g[:, Fdim:].to(odt)
        return grad_x.to(ctx.in_dtype), None, None, None, None


class _ReluDropout(torch.autograd.Function):
    """F.dropout(F.relu(x), p, training) (driver/models.py:47-48) in one pass over x, with a backward
    that needs only the output (csrc/aggregate.hip k_relu_dropout_*)."""

    @staticmethod
    def forward(ctx, x, p, training):
        L = nat.load()
        xc = x.contiguous()
        y = torch.empty_like(xc)
        # the seed comes from torch's CPU generator, so torch.manual_seed makes a run repeatable
        seed = _draw_seed() if training else 0
        nat.check(L.spp_relu_dropout_forward(_p(xc), xc.numel(), float(p), int(bool(training)), seed, _p(y), _stream()))
        ctx.save_for_backward(y)
        ctx.scale = 1.0 / (1.0 - float(p)) if training else 1.0
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        gc = g.contiguous()
        gx = torch.empty_like(gc)
        nat.check(nat.load().spp_relu_dropout_backward(_p(gc), _p(y), gc.numel(), ctx.scale, _p(gx), _stream()))
        return gx, None, None


def relu_dropout(x, p=0.5, training=True):
    """relu followed by dropout; fp32 CUDA tensors take the fused HIP kernel"""
    if x.is_cuda and x.dtype == torch.float32 and x.numel() > 0 and x.data_ptr() % 16 == 0:
        return _ReluDropout.apply(x, p, training)
    return F.dropout(F.relu(x), p=p, training=training)


def mean_aggregate(x, rowptr, col, num_targets):
    return _MeanAggregate.apply(x, rowptr, col, num_targets, False)


# ---- max aggregation (SAGEConv(aggr="max"); csrc/aggregate_max.hip, spp.h f3q) ----
def _max_reference(x, rowptr, col, T):
    """Plain torch restatement of spp_agg_max_forward on a dense x: (out fp32 [T, F], arg int32 [T, F]).  out[t, c] is
    the maximum of column c over the rows x[col[k]] of row t, arg[t, c] the col entry of the FIRST k that attains it: the
    first NaN if the column holds one (it propagates, as torch.amax), else the first of the equal maxima (-0.0 == +0.0:
    the earlier stays).  An empty row gives 0 and -1."""
    x = x.float()
    Fdim = x.size(1)
    out = torch.zeros((T, Fdim), dtype=torch.float32, device=x.device)
    arg = torch.full((T, Fdim), -1, dtype=torch.int32, device=x.device)
    ptr = rowptr.tolist()
    for t in range(T):
        b, e = ptr[t], ptr[t + 1]
        if e <= b:
            continue
        idx = col[b:e]
        rows = x[idx]                                                   # [d, F]
        pos = torch.arange(e - b, device=x.device).unsqueeze(1).expand_as(rows)
        nan = rows.isnan()
        hit = torch.where(nan.any(0, keepdim=True), nan, rows == rows.amax(0, keepdim=True))
        k = torch.where(hit, pos, e - b).amin(0)                        # the first hit of every column
        out[t] = rows.gather(0, k.unsqueeze(0))[0]
        arg[t] = idx[k].to(torch.int32)
    return out, arg


def _agg_max_forward(rowptr, col, T, x, out_dtype, concat, want_arg):
    """spp_agg_max_forward over the row source x (see _rows): the new dense [T, F or 2F] fp32 / bf16 result and the
    int32 [T, F] argmax (None unless want_arg)"""
    src, exps = _rows(x)
    Fdim = src["F"]
    out = torch.empty((T, 2 * Fdim if concat else Fdim), dtype=out_dtype, device=rowptr.device)
    arg = torch.empty((T, Fdim), dtype=torch.int32, device=rowptr.device) if want_arg else None
    d = nat.AggMaxFwdDesc(out_elem=_ELEM[out_dtype], concat_target=int(bool(concat)), rowptr_dev=_p(rowptr),
                          col_dev=_p(col), num_targets=T, scale_log2_dev=_p(exps), out_dev=_p(out), out_stride_elems=0,
                          arg_dev=_p(arg), **src)
    nat.check(nat.load().spp_agg_max_forward(C.byref(d), _stream()))
    return out, arg


class _MaxAggregate(torch.autograd.Function):
    """out[t] = max_{e in row t} x[col[e]], element-wise (empty rows give 0, as PyG's max aggregation); with
    ``concat_target`` the operand [max | x_target] of shape [T, 2F], x_target = x[:T], as _MeanAggregate's.  The
    gradient of out[t, c] goes to the one source row the forward recorded (the first that attains the maximum)."""

    @staticmethod
    def forward(ctx, x, rowptr, col, num_targets, concat_target):
        nat.require_device()
        assert x.is_cuda and _readable(x), "fp16 / fp32 / bf16 / fp8 rows on the GPU"
        if _is_fp8(x):
            _no_input_grad(ctx, "max_aggregate")
        out, arg = _agg_max_forward(rowptr, col, num_targets, x, torch.bfloat16 if amp_bf16() else torch.float32,
                                    concat_target, ctx.needs_input_grad[0])
        if arg is not None:
            ctx.save_for_backward(arg)
        ctx.shape = (x.size(0), x.size(1), num_targets)
        ctx.in_dtype = x.dtype
        ctx.concat = bool(concat_target)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        (arg,) = ctx.saved_tensors
        S, Fdim, T = ctx.shape
        g = _grad_in(grad_out)                           # bf16 / fp32 in, the input's dtype out (fp16 through fp32)
        odt = ctx.in_dtype if ctx.in_dtype in (torch.float32, torch.bfloat16) else torch.float32
        grad_x = torch.empty((S, Fdim), dtype=odt, device=g.device)
        nbytes = 4 * S * Fdim if odt != torch.float32 else 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device) if nbytes else None
        d = nat.AggMaxBwdDesc(grad_elem=_ELEM[g.dtype], out_elem=_ELEM[odt], concat_target=int(ctx.concat), arg_dev=_p(arg),
                              num_targets=T, num_sources=S, grad_out_dev=_p(g),
                              grad_out_stride_elems=g.stride(0) if T > 1 else 0, F=Fdim, grad_x_dev=_p(grad_x),
                              workspace_dev=_p(ws), workspace_bytes=nbytes)
        nat.check(nat.load().spp_agg_max_backward(C.byref(d), _stream()))
        return grad_x.to(ctx.in_dtype), None, None, None, None


def _check_max_source(what, x):
    """what the max kernels read, checked before any device call"""
    m = x.table if isinstance(x, TableRows) else x
    if isinstance(x, RowRefs) or isinstance(m, Fp8Features):
        return
    if not isinstance(m, torch.Tensor):
        raise TypeError(f"{what}: x must be a tensor, a TableRows, a RowRefs or fp8 features, got {type(x).__name__}")
    if m.dim() != 2 or m.dtype not in _ELEM:
        raise ValueError(f"{what}: x must be a 2-D fp32 / fp16 / bf16 matrix, got {tuple(m.shape)} of {m.dtype}")


def max_aggregate(x, rowptr, col, num_targets):
    """The element-wise maximum over every target's neighbour rows, [num_targets, F] (an empty row gives 0); the
    gradient goes to the first row that attains each maximum.  x: as mean_aggregate's."""
    _check_max_source("max_aggregate", x)
    return _MaxAggregate.apply(x, rowptr, col, num_targets, False)


_SAGE_AGGRS = ("mean", "max")


def _check_aggr(what, aggr):
    if aggr not in _SAGE_AGGRS:
        raise ValueError(f"{what}: aggr must be 'mean' or 'max', got {aggr!r}")
    return aggr


# ---- the training tail behind a GEMM: dropout(act(BatchNorm(z))) [+ residual]  (csrc/bn_act.hip, spp.h f3p) ----
_BN_ACTS = {"none": nat.SPP_BN_ACT_NONE, "relu": nat.SPP_BN_ACT_RELU, "leaky_relu": nat.SPP_BN_ACT_LEAKY_RELU}


class _BatchNormAct(torch.autograd.Function):
    """One node for BatchNorm1d (batch statistics in training, running statistics in eval), the activation, dropout and
    the residual add.  Saves z, mean, invstd, gamma and beta and keeps the seed: neither the output nor a mask; the
    backward recomputes the sign of the pre-activation and the keep pattern (spp_bn_act_backward)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, residual, bn, act, slope, p, training):
        L = nat.load()
        n, Cdim = z.shape
        if training:
            if n < 2:       # torch's message, before any buffer is touched
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(z.shape)}")
            # the seed comes from torch's CPU generator, so torch.manual_seed makes a run repeatable
            seed = _draw_seed() if p > 0 else 0
            bn.num_batches_tracked.add_(1)
        else:
            seed = 0
        y_dtype = torch.promote_types(z.dtype, residual.dtype) if residual is not None else z.dtype
        y = torch.empty((n, Cdim), dtype=y_dtype, device=z.device)
        mean = torch.empty(Cdim, dtype=torch.float32, device=z.device)
        invstd = torch.empty_like(mean)
        ws = torch.empty(L.spp_bn_act_workspace_bytes(n, Cdim), dtype=torch.uint8, device=z.device)
        d = nat.BnActDesc(z_elem=_ELEM[z.dtype], r_elem=_ELEM[residual.dtype] if residual is not None else 0,
                          y_elem=_ELEM[y_dtype], act=_BN_ACTS[act], training=int(training), negative_slope=float(slope),
                          p=float(p), eps=float(bn.eps), momentum=-1.0 if bn.momentum is None else float(bn.momentum),
                          seed=seed, n=n, C=Cdim, z_dev=_p(z), gamma_dev=_p(gamma), beta_dev=_p(beta),
                          running_mean_dev=_p(bn.running_mean), running_var_dev=_p(bn.running_var),
                          num_batches_tracked_dev=_p(bn.num_batches_tracked), r_dev=_p(residual), y_dev=_p(y),
                          mean_dev=_p(mean), invstd_dev=_p(invstd), workspace_dev=_p(ws), workspace_bytes=ws.numel())
        nat.check(L.spp_bn_act_forward(C.byref(d), _stream()))
        ctx.save_for_backward(z, gamma, beta, mean, invstd)
        ctx.cfg = (_BN_ACTS[act], float(slope), float(p), int(training), seed, float(bn.eps))
        ctx.res_dtype = residual.dtype if residual is not None else None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        L = nat.load()
        z, gamma, beta, mean, invstd = ctx.saved_tensors
        act, slope, p, training, seed, eps = ctx.cfg
        n, Cdim = z.shape
        gc = g.contiguous()
        if gc.dtype not in (torch.float32, torch.bfloat16):
            gc = gc.to(torch.float32)
        g_res = g.to(ctx.res_dtype) if ctx.needs_input_grad[3] else None
        dz = torch.empty_like(z)
        dgamma = torch.empty(Cdim, dtype=torch.float32, device=z.device)
        dbeta = torch.empty_like(dgamma)
        if n > 0:
            ws = torch.empty(L.spp_bn_act_workspace_bytes(n, Cdim), dtype=torch.uint8, device=z.device)
            d = nat.BnActDesc(z_elem=_ELEM[z.dtype], g_elem=_ELEM[gc.dtype], act=act, training=training,
                              negative_slope=slope, p=p, eps=eps, seed=seed, n=n, C=Cdim, z_dev=_p(z), gamma_dev=_p(gamma),
                              beta_dev=_p(beta), mean_dev=_p(mean), invstd_dev=_p(invstd), g_dev=_p(gc), dz_dev=_p(dz),
                              dgamma_dev=_p(dgamma), dbeta_dev=_p(dbeta), workspace_dev=_p(ws), workspace_bytes=ws.numel())
            nat.check(L.spp_bn_act_backward(C.byref(d), _stream()))
        else:
            dgamma.zero_(), dbeta.zero_()
        return dz, dgamma.to(gamma.dtype), dbeta.to(beta.dtype), g_res, None, None, None, None, None


def _bn_act_torch(z, bn, act, negative_slope, p, training, residual):
    """The plain torch composition: F.dropout(act(bn(z)), p, training) + residual"""
    if training == bn.training:
        h = bn(z)
    else:                                           # BatchNorm1d.forward with the other mode
        was = bn.training
        bn.train(training)
        try:
            h = bn(z)
        finally:
            bn.train(was)
    if act == "relu":
        h = F.relu(h)
    elif act == "leaky_relu":
        h = F.leaky_relu(h, negative_slope)
    h = F.dropout(h, p=p, training=training)
    return h if residual is None else h + residual


def batch_norm_act(z, bn, *, act="none", negative_slope=0.01, p=0.0, training=None, residual=None):
    """``F.dropout(act(bn(z)), p, training) + residual`` as one autograd node on HIP kernels (csrc/bn_act.hip).

    ``bn`` is a ``torch.nn.BatchNorm1d``: its weight, bias, running buffers, ``momentum``, ``eps`` and
    ``num_batches_tracked`` are used and updated as the module's own forward would; ``training`` defaults to
    ``bn.training``.  ``act`` is "none", "relu" or "leaky_relu" (``negative_slope``); ``residual`` has z's shape.
    Dropout draws its seed from torch's CPU generator (``torch.manual_seed`` makes a run repeatable); its keep pattern
    is this library's counter-based generator, not torch's.

    Contiguous fp32 / bf16 CUDA matrices take the kernels.  Everything else -- CPU tensors, other dtypes or shapes,
    ``affine=False`` or ``track_running_stats=False`` modules -- runs the plain torch composition.  Double backward
    through the kernel path is not supported."""
    if act not in _BN_ACTS:
        raise ValueError(f"batch_norm_act: act must be one of {sorted(_BN_ACTS)}, got {act!r}")
    training = bn.training if training is None else bool(training)
    ok = lambda t: (t.is_cuda and t.dim() == 2 and t.is_contiguous() and t.dtype in (torch.float32, torch.bfloat16))
    fused = (isinstance(bn, torch.nn.BatchNorm1d) and bn.affine and bn.track_running_stats and ok(z)
             and z.size(1) == bn.num_features and (training or z.size(0) > 0) and 0.0 <= p < 1.0
             and bn.weight.dtype == torch.float32 and bn.weight.is_cuda and bn.weight.device == z.device
             and (residual is None or (ok(residual) and residual.shape == z.shape and residual.device == z.device)))
    if not fused:
        return _bn_act_torch(z, bn, act, negative_slope, p, training, residual)
    return _BatchNormAct.apply(z, bn.weight, bn.bias, residual, bn, act, negative_slope, p, training)


class _TallLinear(torch.autograd.Function):
    """y = a @ w.T for a very tall ``a`` ([T, K], T ~ 1e5) and a small ``w`` ([N, K]).

    The weight gradient ``g.T @ a`` is a [N, K] output reduced over T: as one GEMM it has a handful
    of output tiles for 256 CUs (measured 505 us at T=165k, K=200, N=256 -- 27 % of the step).  It is
    computed as a batched GEMM over row slabs (split-K) and summed instead.

    Under bf16 autocast a and w are used in bf16 (y bf16); the weight gradient comes back in w's dtype (fp32), the input
    gradient in a's."""

    @staticmethod
    def forward(ctx, a, w):
        ctx.amp = amp_bf16()
        with _no_autocast():
            if ctx.amp:
                ctx.dtypes = (a.dtype, w.dtype)
                a, w = a.to(torch.bfloat16), w.to(torch.bfloat16)
            ctx.save_for_backward(a, w)
            return a @ w.t()

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        if ctx.amp:
            g = g.to(torch.bfloat16).contiguous()
            grad_a = (g @ w).to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None
            grad_w = _wgrad(g, a).to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None
            return grad_a, grad_w
        grad_a = g @ w if ctx.needs_input_grad[0] else None
        grad_w = None
        if ctx.needs_input_grad[1]:
            T = a.size(0)
            slabs = min(64, T // 4096)
            if slabs >= 2 and a.is_contiguous() and g.is_contiguous():
                c = T // slabs
                head = torch.bmm(g[:slabs * c].view(slabs, c, -1).transpose(1, 2), a[:slabs * c].view(slabs, c, -1))
                grad_w = head.sum(0)
                if slabs * c < T:
                    grad_w = grad_w + g[slabs * c:].t() @ a[slabs * c:]
            else:
                grad_w = g.t() @ a
        return grad_a, grad_w


def init_weights(m):                                     # driver/models.py:12-16
    if isinstance(m, torch.nn.Linear):
        torch.nn.init.xavier_uniform_(m.weight, gain=torch.nn.init.calculate_gain("relu"))


class SAGEConv(torch.nn.Module):
    """torch_geometric.nn.SAGEConv(in, out, aggr='mean' | 'max', root_weight=True, bias=...) on a bipartite
    ((x, x_target), adj_t):  lin_l(aggr_j x_j) + lin_r(x_target); only lin_l carries the bias.  ``aggr`` chooses the
    neighbour reduction (the mean, or the element-wise maximum); the parameters are the same for both."""

    def __init__(self, in_channels, out_channels, bias=True, *, aggr="mean"):
        super().__init__()
        self.aggr = _check_aggr("SAGEConv", aggr)
        self.lin_l = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.lin_r = torch.nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()

    def forward(self, x_pair, adj_t):
        x, x_target = x_pair
        rowptr, col, _ = adj_t.csr()
        aggregate = _MaxAggregate if self.aggr == "max" else _MeanAggregate
        if _is_fp8(x) or isinstance(x, (TableRows, RowRefs)):   # rows read in place: the targets are the first rows of x
            if x_target is not None and x_target is not x:
                raise RuntimeError("SAGEConv over fp8 rows: the targets are the first rows of x (pass (x, None))")
            fused = aggregate.apply(x, rowptr, col, int(adj_t.sparse_sizes()[0]), True)
            out = _TallLinear.apply(fused, torch.cat([self.lin_l.weight, self.lin_r.weight], dim=1))
            return out if self.lin_l.bias is None else out + self.lin_l.bias
        # [mean_j x_j | x_target] @ [W_l | W_r]^T: one GEMM instead of two plus an add
        T = x_target.size(0)
        if _is_prefix(x, x_target) and x_target.size(1) == x.size(1):
            fused = aggregate.apply(x, rowptr, col, T, True)                # x_target = x[:T] (the MFG contract)
        else:                                                               # a foreign target matrix
            mean = aggregate.apply(x, rowptr, col, T, False)                # (bf16 under bf16 autocast)
            fused = torch.cat([mean, x_target.to(mean.dtype)], dim=1)
        out = _TallLinear.apply(fused, torch.cat([self.lin_l.weight, self.lin_r.weight], dim=1))
        return out if self.lin_l.bias is None else out + self.lin_l.bias


class _ConvModel(torch.nn.Module):
    """What every model here shares: ``convs``, reset as the reference resets them"""

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
            conv.apply(init_weights)


class _LayerwiseInference:
    """``model.inference`` of the models that have one (GraphTransformer does not: see its docstring)"""

    @torch.no_grad()
    def inference(self, x_all, rowptr, col, **kw):
        """Exact log-probabilities of every node (or of ``nodes=``) from the whole graph, layer by layer: see
        ``inference.layerwise_inference`` (keywords ``nodes``, ``rows_per_slab``, ``act_dtype``).  The reference's
        ``inference(x_all, device, make_subgraph_iter)`` walks sampled full-neighbour subgraphs; here nothing is sampled:
        the graph and x_all are resident, so the arguments are the matrix and the graph's CSR.

        GAT and GATv2: the long-row softmax behind ``_attn_layers`` (``_gat_layer`` / ``_gatv2_layer``).  GIN: BatchNorm
        on its running statistics.  GCN: keyword ``edge_weight``, what ``adj_t`` carries in training.  SAGEResInception:
        the head as a running accumulator (``_resinc_layers``)."""
        from .inference import layerwise_inference
        return layerwise_inference(self, x_all, rowptr, col, **kw)


class SAGE(_LayerwiseInference, _ConvModel):
    """``aggr="max"`` (keyword only) replaces every layer's mean by the element-wise maximum over the neighbours
    (PyG's SAGEConv(aggr="max")); parameters and state-dict keys are those of the default."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, *, aggr="mean"):
        super().__init__()
        self.aggr = _check_aggr("SAGE", aggr)
        self.num_layers = num_layers
        self.hidden_channels = hidden_channels
        self.convs = torch.nn.ModuleList()
        self.convs.append(SAGEConv(in_channels, hidden_channels, bias=False, aggr=aggr))
        for _ in range(num_layers - 2):
            self.convs.append(SAGEConv(hidden_channels, hidden_channels, bias=False, aggr=aggr))
        self.convs.append(SAGEConv(hidden_channels, out_channels, bias=False, aggr=aggr))
        self.reset_parameters()

    def forward(self, x, adjs):
        # the reference converts the whole feature matrix to fp32 first (models.py:43); the first
        # aggregation reads the fp16 rows directly instead (exact) and only the targets are converted
        if self.aggr == "max":
            return self._forward_max(x, adjs)
        if x.is_cuda and _SageStack.usable(self, x, adjs):
            hops = []
            for adj_t, _e_id, size in adjs:
                rowptr, col, _ = adj_t.csr()
                hops.append((rowptr, col, int(size[1])))
            weights = [w for conv in self.convs for w in (conv.lin_l.weight, conv.lin_r.weight)]
            if isinstance(x, TableRows):                 # fused first layer: the batch's rows are read from the table
                x = (x.table, x.n_id)
            elif isinstance(x, RowRefs):                 # ... or wherever the partitioned path found them
                x = _Refs(x)
            return _SageStack.apply(x, hops, self.training, 0.5, *weights)
        if isinstance(x, (TableRows, RowRefs)):
            x = x.materialize()
        elif isinstance(x, Fp8Features):
            x = x.dequantize(torch.float16)
        for i, (adj_t, _e_id, size) in enumerate(adjs):
            x_target = x[:size[1]]
            x = self.convs[i]((x, x_target), adj_t)
            if i != self.num_layers - 1:
                x = relu_dropout(x, 0.5, self.training)       # F.relu + F.dropout(p=0.5) (models.py:47-48)
        return torch.log_softmax(x, dim=-1)

    def _forward_max(self, x, adjs):
        """aggr="max", layer by layer: max_aggregate's operand [max | x_target], one tall GEMM, ReLU + dropout.  The
        first layer reads a TableRows, a RowRefs or fp8 rows in place, as the mean's fused first layer does."""
        for i, (adj_t, _e_id, size) in enumerate(adjs):
            in_place = _is_fp8(x) or isinstance(x, (TableRows, RowRefs))
            x = self.convs[i]((x, None if in_place else x[:size[1]]), adj_t)
            if i != self.num_layers - 1:
                x = relu_dropout(x, 0.5, self.training)
        return torch.log_softmax(x, dim=-1)


def _wgrad(g, a):
    """g.T @ a for very tall g [T, N], a [T, K]: batched over row slabs and summed (see _TallLinear).  64 slabs of
    >= 2048 rows in the a.T @ g order are what the library runs fastest at T = 164 k, N = K = 256 (162 us against 174-181
    for 32 slabs and 483 for the single product; tools/gemm_variants.py).

    bf16 g and a (autocast): every slab's product is accumulated in fp32 by the GEMM and rounded to bf16 once, the
    slabs are summed in fp32, and the result is fp32 (a weight gradient)."""
    T = a.size(0)
    slabs = min(64, T // 2048)
    if slabs < 2:
        return (g.t() @ a).float()
    c = T // slabs
    acc = torch.bmm(a[:slabs * c].view(slabs, c, -1).transpose(1, 2), g[:slabs * c].view(slabs, c, -1)).sum(
        0, dtype=torch.float32)                                                                            # [K, N]
    if slabs * c < T:      # the < `slabs` rows left over
        if g.dtype == torch.float32:
            acc.addmm_(a[slabs * c:].t(), g[slabs * c:])   # accumulated in place (one launch; it was a product + an add)
        else:
            acc.add_(a[slabs * c:].t() @ g[slabs * c:])    # bf16: the product rounded once, like every slab's
    return acc.t()


def _split_wgrad(gW):
    """[N, 2K] weight gradient of the [W_l | W_r] operand -> (grad W_l, grad W_r), each [N, K] contiguous, with ONE copy
    launch for both: gW is the transposed view of a contiguous [2K, N] sum (see _wgrad), so its two halves are the two
    [K, N] blocks of that buffer, transposed together."""
    N, K2 = gW.shape
    base = gW.t()
    if not base.is_contiguous():
        return gW[:, :K2 // 2].contiguous(), gW[:, K2 // 2:].contiguous()
    both = base.view(2, K2 // 2, N).transpose(1, 2).contiguous()      # [2, N, K]
    return both[0], both[1]


def _tall_linear(a, w):
    """a @ w.T for a very tall a [T, K].  Round 3 issued it in four row chunks (206 against 214-236 us for the single
    product at T = 164 k, N = K = 256 then); with this stack's library F.linear(a, w) takes the transposed weight as it is and
    runs as fast (201-204 against 207 us, tools/corun_gemm.py), and one launch instead of an empty + a transposed copy +
    four products is 0.1 ms less host time per step: resident step 1.010-1.015 -> 0.995-0.997 ms, with the data path
    1.140-1.156 -> 1.111-1.121 (tools/overlap_ab.py, SPP_SAGE_ONE_PRODUCT A/B of round 4)."""
    return torch.nn.functional.linear(a, w)


def _readable(x):
    """a feature matrix, TableRows or RowRefs the aggregation kernels read in place (fp16 / fp32 / bf16 rows)"""
    if isinstance(x, RowRefs):
        return x.dtype in _ELEM
    m = x.table if isinstance(x, TableRows) else x
    if isinstance(m, Fp8Features):                        # fp8 rows with column scales: spp_agg_forward_fp8
        return m.is_cuda
    return m.is_cuda and m.dim() == 2 and m.stride(1) == 1 and m.dtype in _ELEM


class _SageStack(torch.autograd.Function):
    """The whole SAGE forward (all layers: fused operand, one GEMM, ReLU + dropout; log_softmax) as ONE
    autograd node with a hand-written backward.  The kernels are the ones the layer-wise path uses; what
    goes away is the host side: ~25 autograd nodes, nine Python-level backward calls and the slice /
    accumulate bookkeeping of x[:T] cost more wall time than the GPU work they enqueue (1.06 ms of
    kernels in a 1.34 ms step at papers scale)."""

    @staticmethod
    def usable(model, x, adjs):
        # a matrix, or the first layer reads the resident table (TableRows) / the rows' addresses (RowRefs) itself
        rows = x.table if isinstance(x, TableRows) else x
        if not _readable(x) or (isinstance(rows, torch.Tensor) and rows.requires_grad):
            return False
        k = x.size(1)
        for conv in model.convs:
            if conv.lin_l.bias is not None or conv.lin_l.weight.dtype != torch.float32 or k % 4:
                return False
            k = conv.lin_l.weight.size(0)
        return len(adjs) == len(model.convs)

    @staticmethod
    def forward(ctx, x, hops, training, p, *weights):
        """x: a feature matrix or Fp8Features, the (table, n_id) of a TableRows, or a _Refs.  Under bf16 autocast the
        operands A [T, 2K], [W_l | W_r] (cast once per layer, in the one copy) and the pre-activations Z are bf16, else
        fp32; log_softmax is fp32 in both."""
        if _is_fp8(x):
            _no_input_grad(ctx, "SAGE")
        nat.require_device()
        ctx.amp = amp_bf16()
        dt = torch.bfloat16 if ctx.amp else torch.float32
        st = _stream()
        n_layers = len(hops)
        operands, acts, wcats, seeds = [], [], [], []
        with _no_autocast():
            for i, (rowptr, col, T) in enumerate(hops):
                if i == 0:
                    A = _agg_forward(nat.SPP_AGG_OPERAND, rowptr, col, T, x, dt, st=st)
                else:
                    # Z is the previous layer's PRE-activation: ReLU + dropout are applied to its rows as they are
                    # loaded (no separate pass over the activation, which is never materialised)
                    A = _agg_forward(nat.SPP_AGG_OPERAND_ACT, rowptr, col, T, Z, dt, act=(p, bool(training), seeds[i - 1]),
                                     st=st)
                wl, wr = weights[2 * i], weights[2 * i + 1]
                W = torch.cat([wl, wr], dim=1, out=torch.empty((wl.size(0), A.size(1)), dtype=dt, device=A.device))
                Z = _tall_linear(A, W)                                          # W: [N, 2K] = [W_l | W_r]
                operands.append(A)
                wcats.append(W)
                if i != n_layers - 1:
                    seeds.append(_draw_seed() if training else 0)
                    acts.append(Z)                                              # the pre-activation
            out = torch.log_softmax(Z, dim=-1, dtype=torch.float32)
        # tensors through save_for_backward (saved-tensor hooks, in-place version checks, a second backward with
        # retain_graph all behave as autograd users expect); only ints and seeds live on ctx
        hop_t = [t for (rowptr, col, _T) in hops for t in (rowptr, col)]
        ctx.save_for_backward(*operands, *acts, *wcats, out, *hop_t)
        ctx.hop_T = [int(T) for (_r, _c, T) in hops]
        ctx.act = (float(p), int(bool(training)), seeds)
        batch_rows = x[1].numel() if isinstance(x, tuple) else x.r.size(0) if isinstance(x, _Refs) else x.size(0)
        ctx.src_rows = [batch_rows] + [a.size(0) for a in acts]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        st = _stream()
        dt = torch.bfloat16 if ctx.amp else torch.float32
        n_layers = len(ctx.hop_T)
        sv = ctx.saved_tensors
        operands, acts = sv[:n_layers], sv[n_layers:2 * n_layers - 1]
        wcats, out = sv[2 * n_layers - 1:3 * n_layers - 1], sv[3 * n_layers - 1]
        hop_t = sv[3 * n_layers:]
        hops = [(hop_t[2 * i], hop_t[2 * i + 1], ctx.hop_T[i]) for i in range(n_layers)]
        p_, training_, seeds = ctx.act
        grads = [None] * (2 * n_layers)
        with _no_autocast():
            gZ = torch._log_softmax_backward_data(g_out.float().contiguous(), out, -1, torch.float32).to(dt)
            for i in range(n_layers - 1, -1, -1):
                A, W = operands[i], wcats[i]
                K = A.size(1) // 2
                gW = _wgrad(gZ, A)                                              # fp32
                grads[2 * i], grads[2 * i + 1] = _split_wgrad(gW)
                if i == 0:
                    break
                rowptr, col, T = hops[i]
                gA = gZ @ W                                                     # [T, 2K]
                # the input gradient with the ReLU + dropout backward applied before the row is stored: by gather over
                # the transposed hop, or (small hops) k_grad_init, the scatter and k_relu_dropout_bwd_pre
                gZ = _agg_backward(nat.SPP_AGG_OPERAND_ACT, rowptr, col, T, ctx.src_rows[i], gA, K, dt,
                                   gather=col.numel() * K >= _GATHER_MIN_WORK, z=acts[i - 1],
                                   act=(p_, training_, seeds[i - 1]), st=st)
        return (None, None, None, None, *grads)


# --------------------------------------------------------------------------------------------
# GAT  (driver/models.py:195-231: GATConv(bias=False, heads=1))
# --------------------------------------------------------------------------------------------
class _GatAggregate(torch.autograd.Function):
    """out[i] = sum_j softmax_j(leaky_relu(a_src[j] + a_dst[i])) h[j] over row i (its diagonal entry
    dropped) plus the self loop GATConv adds."""

    @staticmethod
    def forward(ctx, h, a_src, a_dst, rowptr, col, slope):
        L = nat.load()
        nat.require_device()
        h, a_src, a_dst = h.contiguous().float(), a_src.contiguous().float(), a_dst.contiguous().float()
        T, Fdim = a_dst.numel(), h.size(1)
        out = torch.empty((T, Fdim), dtype=torch.float32, device=h.device)
        rmax = torch.empty(T, dtype=torch.float32, device=h.device)
        rsum = torch.empty(T, dtype=torch.float32, device=h.device)
        nat.check(L.spp_gat_forward(_p(rowptr), _p(col), T, _p(h), Fdim, _p(a_src), _p(a_dst), float(slope), _p(out),
                                    _p(rmax), _p(rsum), _stream()))
        ctx.save_for_backward(h, a_src, a_dst, rowptr, col, out, rmax, rsum)
        ctx.slope = float(slope)
        return out

    @staticmethod
    def backward(ctx, g):
        h, a_src, a_dst, rowptr, col, out, rmax, rsum = ctx.saved_tensors
        T, Fdim = a_dst.numel(), h.size(1)
        g = g.contiguous().float()
        grad_h = torch.zeros_like(h)
        grad_as = torch.zeros_like(a_src)
        grad_ad = torch.zeros_like(a_dst)
        nat.check(nat.load().spp_gat_backward(_p(rowptr), _p(col), T, _p(h), Fdim, _p(a_src), _p(a_dst), ctx.slope,
                                              _p(out), _p(rmax), _p(rsum), _p(g), _p(grad_h), _p(grad_as), _p(grad_ad),
                                              _stream()))
        return grad_h, grad_as, grad_ad, None, None, None


def _check_heads(heads, bool_ok=True):
    """a conv's or a model's ``heads``; only TransformerConv and GraphTransformer refuse a bool"""
    if (isinstance(heads, bool) and not bool_ok) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"heads must be a positive int, got {heads!r}")


def _check_attn_dropout(dropout):
    if isinstance(dropout, bool) or not isinstance(dropout, (int, float)) or not 0.0 <= dropout < 1.0:
        raise ValueError(f"dropout must be a number in [0, 1), got {dropout!r}")


def _gat_kernels_read(x, x_target):
    """the rows _GatLayer / _GatLayerMH read in place, with the targets the prefix of x"""
    K = x.size(1)
    return (x.is_cuda and x.dim() == 2 and x.stride(1) == 1 and x.dtype in _ELEM and K % 4 == 0 and K <= 1024 and
            _is_prefix(x, x_target))


class GATConv(torch.nn.Module):
    """torch_geometric.nn.GATConv(in, out, heads=1, concat=True, negative_slope=0.2, dropout=0, add_self_loops=True,
    bias=...) on a bipartite ((x, x_target), adj_t): one shared linear map for sources and targets
    (an int ``in_channels``), attention vectors att_src / att_dst, softmax over the incoming edges.

    ``heads`` = H: W is [H * out, in], att_src / att_dst are [1, H, out] (PyG's layout), every head has its own
    softmax, and the output is the H heads side by side ([T, H * out], ``concat=True``) or their mean ([T, out]);
    ``bias`` has the output's width.  heads=1 runs the single-head path; H in {1, 2, 4, 8} with the rows the kernels
    read takes _GatLayerMH, anything else a plain-torch restatement of the same function (_gat_mh_reference).

    ``dropout`` = p in [0, 1): F.dropout(alpha, p, training) on the attention coefficients of every (entry, head), the
    self loop included (PyG's self loops are edges like any other); the softmax itself runs over all entries.  p = 0 and
    eval mode run exactly the paths above.  In training with p > 0, the inputs the kernels read (any H in {1, 2, 4, 8},
    heads=1 too) take _GatLayerMH with the mask generated inside its kernels from a seed drawn from torch's CPU generator
    (spp.h f3t; _attn_keep_reference restates it); everything else takes _gat_mh_reference with F.dropout on its alpha:
    torch's own mask there, not the kernels'.  No parameter or buffer: the state dict does not change."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, bias=True):
        super().__init__()
        _check_heads(heads)
        _check_attn_dropout(dropout)
        self.heads, self.out_channels, self.concat = heads, out_channels, bool(concat)
        self.negative_slope = negative_slope
        self.dropout = float(dropout)
        self.lin_src = torch.nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        width = heads * out_channels if concat else out_channels
        self.bias = torch.nn.Parameter(torch.zeros(width)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        self.lin_src.reset_parameters()
        # (xavier_uniform_ on [1, H, C]: bound sqrt(6 / (H*C + C)); PyG's glorot takes sqrt(6 / (H + C)).  Kept as it
        # was for heads=1, whose initial values must not change; the training tests start from this bound at every H.)
        torch.nn.init.xavier_uniform_(self.att_src)
        torch.nn.init.xavier_uniform_(self.att_dst)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x_pair, adj_t):
        if self.heads != 1 or (self.training and self.dropout > 0.0):
            return self._forward_heads(x_pair, adj_t)
        x, x_target = x_pair
        rowptr, col, _ = adj_t.csr()
        T = x_target.size(0)
        if _gat_kernels_read(x, x_target):
            # aggregate the raw rows with the attention weights, project only the T targets (_GatLayer)
            out = _GatLayer.apply(x, self.lin_src.weight, self.att_src.view(-1), self.att_dst.view(-1), rowptr, col, T,
                                  self.negative_slope)
            return out if self.bias is None else out + self.bias
        h = _TallLinear.apply(x.to(torch.float32), self.lin_src.weight)   # targets are the first rows of the sources
        h_t = h[:x_target.size(0)]
        a_src = (h * self.att_src.view(1, -1)).sum(-1)       # (a gemv on this tall shape measured 3x slower)
        a_dst = (h_t * self.att_dst.view(1, -1)).sum(-1)
        out = _GatAggregate.apply(h, a_src, a_dst, rowptr, col, self.negative_slope)
        return out if self.bias is None else out + self.bias

    def _forward_heads(self, x_pair, adj_t):
        x, x_target = x_pair
        rowptr, col, _ = adj_t.csr()
        T, H = x_target.size(0), self.heads
        att_src, att_dst = self.att_src.view(H, -1), self.att_dst.view(H, -1)
        p = self.dropout if self.training else 0.0
        if H in _ATTN_HEADS and _gat_kernels_read(x, x_target):
            out = _GatLayerMH.apply(x, self.lin_src.weight, att_src, att_dst, rowptr, col, T, self.negative_slope,
                                    self.concat, p)
        else:
            out = _gat_mh_reference(x, x_target, self.lin_src.weight, att_src, att_dst, rowptr, col,
                                    self.negative_slope, self.concat, p)
        return out if self.bias is None else out + self.bias


def _attn_keep_reference(E, T, H, p, seed):
    """The keep rule of the attention dropout kernels (spp.h f3t) in numpy uint64: keep [(E + T), H] uint8, entry-major
    (the E CSR entries, then the T self loops); what spp_gat_mh_attn_keep writes.  Draw index i = entry * H + h is the low
    (i even) or high (i odd) half of mix64(seed + (i >> 1) * 0x9E3779B97F4A7C15), kept iff below (1 - p) * 2^32."""
    import numpy as np
    keep = 1.0 - float(np.float32(p))                                       # the entries take p as a C float
    thr = np.uint64(0xFFFFFFFF if keep >= 1.0 else int(keep * 4294967296.0))
    i = np.arange((E + T) * H, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (i >> np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)      # mix64: the splitmix64 finaliser
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    draw = np.where(i & np.uint64(1), z >> np.uint64(32), z & np.uint64(0xFFFFFFFF))
    return (draw < thr).astype(np.uint8).reshape(E + T, H)


def _with_self_loops(rowptr, col, T):
    """GATConv's and GATv2Conv's edge list (src, dst) of a hop: set_diag -- the diagonal entries dropped, then one self
    loop (i, i) per target, after the E' kept entries"""
    dst = torch.repeat_interleave(torch.arange(T, device=col.device), rowptr[1:] - rowptr[:-1])
    keep = col != dst
    loops = torch.arange(T, device=col.device)
    return torch.cat([col[keep], loops]), torch.cat([dst[keep], loops])


def _softmax_aggregate(e, src, dst, rows, T, p):
    """The tail of the three plain-torch references: alpha = the softmax of the logits e [E', H] over every target's
    entries, F.dropout on it when p > 0, out[t] = sum alpha * rows[src] -- [T, H, C], all in e's dtype"""
    dt, H = e.dtype, e.size(1)
    emax = torch.full((T, H), float("-inf"), dtype=dt, device=e.device)
    emax = emax.scatter_reduce(0, dst[:, None].expand(-1, H), e, "amax")
    w = torch.exp(e - emax[dst])
    den = torch.zeros((T, H), dtype=dt, device=e.device).index_add_(0, dst, w)
    alpha = w / den[dst]
    if p > 0.0:
        alpha = F.dropout(alpha, p, training=True)
    out = torch.zeros((T,) + tuple(rows.shape[1:]), dtype=dt, device=e.device)
    return out.index_add_(0, dst, alpha[:, :, None] * rows[src].to(dt))


def _gat_mh_reference(x, x_target, W, att_src, att_dst, rowptr, col, slope, concat, p=0.0):
    """GATConv with H heads in PyG's project-first order, in plain torch ops (the path for inputs the kernels do not
    read: K % 4 != 0, K > 1024, other head counts, a target block that is not the prefix of x, CPU tensors).
    x [S, K], x_target [T, K], W [H*C, K], att_* [H, C]; set_diag: diagonal entries dropped, one self loop (i, i) per
    target, whose message is source row i.  p > 0 (training): F.dropout on alpha -- torch's own mask, from the
    generator of alpha's device, NOT the kernels' counter-based one (_attn_keep_reference)."""
    H, Cc = att_src.shape
    S, T = x.size(0), x_target.size(0)
    h = F.linear(x.to(W.dtype), W).view(S, H, Cc)
    h_t = h[:T] if _is_prefix(x, x_target) else F.linear(x_target.to(W.dtype), W).view(T, H, Cc)
    a_src = (h * att_src).sum(-1)                                           # [S, H]
    a_dst = (h_t * att_dst).sum(-1)                                         # [T, H]
    src, dst = _with_self_loops(rowptr, col, T)
    e = F.leaky_relu(a_src[src].float() + a_dst[dst].float(), slope)        # [E', H], fp32 from here on
    out = _softmax_aggregate(e, src, dst, h, T, p)
    return out.reshape(T, H * Cc) if concat else out.mean(1)


def _gat_kernels_forward(x, V_src, V_dst, rowptr, col, T, H, slope, p=0.0):
    """The kernel calls of a GAT layer's forward, the spp_gat_mh_* entries with heads = H (_GatLayer: H = 1): the
    logits a_src [S, H], a_dst [T, H] of x's rows (fp32, fp16 or bf16) with V_src, V_dst [H, K], then z [T, H, K] with
    the softmax statistics rmax, rsum [T, H]; all fp32.  p > 0: attention dropout inside the kernels (spp.h f3t).
    Returns (a_src, a_dst, z, rmax, rsum, drop), drop = (p, seed) for the backward's identical mask, or None."""
    L = nat.load()
    nat.require_device()
    st = _stream()
    S, K = x.size(0), x.size(1)
    elem = _ELEM[x.dtype]
    xs = x.stride(0) if S > 1 else K
    f32 = dict(dtype=torch.float32, device=x.device)
    a_src, a_dst = torch.empty((S, H), **f32), torch.empty((T, H), **f32)
    nat.check(L.spp_gat_mh_logits(_p(x), elem, xs, S, T, K, H, _p(V_src), _p(V_dst), _p(a_src), _p(a_dst), st))
    z = torch.empty((T, H, K), **f32)
    rmax, rsum = torch.empty((T, H), **f32), torch.empty((T, H), **f32)
    drop = (p, _attn_seed()) if p > 0.0 else None
    _call_drop(L, "spp_gat_mh_aggregate_forward",
                        (_p(rowptr), _p(col), T, _p(x), elem, xs, K, H, _p(a_src), _p(a_dst), float(slope), _p(z),
                         _p(rmax), _p(rsum), st), drop)
    return a_src, a_dst, z, rmax, rsum, drop


def _gat_kernels_backward(x, rowptr, col, a_src, a_dst, z, rmax, rsum, g_z, V, slope, want_gx, drop):
    """The kernel calls of a GAT layer's backward from g_z [T, H, K] fp32 (the forward's buffers and drop as
    _gat_kernels_forward returned them; V = [V_src, V_dst], [2, H, K], read by the gather form only).  Returns (g_x, g_as, g_ad, g_V, gathered): g_as [S, H] and g_ad [T, H], the
    logits' gradients; g_V [2, H, K], those of V_src, V_dst; g_x [S, K] fp32, None unless want_gx.  From E * K = 2^22 on
    g_x comes by gather over the transposed hop and is complete (gathered); below, by atomics, and the caller still adds
    the logits' terms g_as V_src + g_ad V_dst (rows :T)."""
    L = nat.load()
    st = _stream()
    S, K = x.size(0), x.size(1)
    T, H = a_dst.shape
    elem = _ELEM[x.dtype]
    xs = x.stride(0) if S > 1 else K
    E = col.numel()
    gather = want_gx and E * K >= _GATHER_MIN_WORK
    f32 = dict(dtype=torch.float32, device=x.device)
    g_as, g_ad = torch.zeros((S, H), **f32), torch.empty((T, H), **f32)
    if gather:      # no E x K fp32 atomics, no zero fill, and the logits' rank-1 terms are added in the same pass
        g_x = torch.empty((S, K), **f32)
        nbytes = int(L.spp_gat_mh_aggregate_backward_gather_workspace_bytes(T, S, E, H))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _call_drop(L, "spp_gat_mh_aggregate_backward_gather",
                            (_p(rowptr), _p(col), T, S, E, _p(x), elem, xs, K, H, _p(a_src), _p(a_dst), slope, _p(z),
                             _p(rmax), _p(rsum), _p(g_z), _p(V[0]), _p(V[1]), _p(g_x), _p(g_as), _p(g_ad), _p(ws),
                             nbytes, st), drop)
    else:
        g_x = torch.zeros((S, K), **f32) if want_gx else None
        _call_drop(L, "spp_gat_mh_aggregate_backward",
                            (_p(rowptr), _p(col), T, _p(x), elem, xs, K, H, _p(a_src), _p(a_dst), slope, _p(z),
                             _p(rmax), _p(rsum), _p(g_z), _p(g_x), _p(g_as), _p(g_ad), st), drop)
    g_V = torch.empty((2, H, K), **f32)
    nat.check(L.spp_gat_mh_logits_backward(_p(x), elem, xs, S, T, K, H, _p(g_as), _p(g_ad), _p(g_V[0]), _p(g_V[1]),
                                           st))
    return g_x, g_as, g_ad, g_V, gather


class _GatLayerMH(torch.autograd.Function):
    """GATConv with H > 1 heads on ((x, x[:T]), adj_t) as ONE node, _GatLayer's aggregate-then-project form per head:

        V_src[h] = W_h^T att_src[h], V_dst[h] = W_h^T att_dst[h]   (W_h: rows h*C .. (h+1)*C of W; V: [H, K])
        z[i,h,:] = sum_j alpha_ij^h x_j                              (raw rows, each read once per edge for all heads)
        concat:  out[:, h*C:(h+1)*C] = z[:,h,:] @ W_h^T             (one batched GEMM)
        mean:    out = z.view(T, H*K) @ [W_0^T; ...; W_{H-1}^T] / H  (one GEMM)

    x rows fp32, fp16 or bf16; V, the logits, z and the softmax statistics fp32.  Under bf16 autocast the projection and
    the backward's GEMMs run in bf16 (bf16 output); parameters and their gradients stay fp32."""

    @staticmethod
    def forward(ctx, x, W, att_src, att_dst, rowptr, col, T, slope, concat, p=0.0):
        ctx.amp = amp_bf16()
        with _no_autocast():
            return _GatLayerMH._forward(ctx, x, W, att_src, att_dst, rowptr, col, T, slope, concat, float(p))

    @staticmethod
    def _forward(ctx, x, W, att_src, att_dst, rowptr, col, T, slope, concat, p):
        K = x.size(1)
        H, Cc = att_src.shape
        W3 = W.to(torch.float32).view(H, Cc, K)
        att = torch.stack([att_src, att_dst]).to(torch.float32)                  # [2, H, C]
        V = torch.einsum("shc,hck->shk", att, W3).contiguous()                   # [2, H, K]: V_src, V_dst
        a_src, a_dst, z, rmax, rsum, ctx.drop = _gat_kernels_forward(x, V[0], V[1], rowptr, col, T, H, slope, p)
        ctx.save_for_backward(x, W, att_src, att_dst, rowptr, col, a_src, a_dst, z, rmax, rsum, V)
        ctx.dims = (T, K, H, Cc, float(slope), bool(concat))
        dt = torch.bfloat16 if ctx.amp else torch.float32
        zc, Wc = z.to(dt), W.to(dt).view(H, Cc, K)
        if concat:                                                               # [H, T, K] @ [H, K, C] -> [T, H, C]
            return torch.bmm(zc.transpose(0, 1), Wc.transpose(1, 2)).transpose(0, 1).reshape(T, H * Cc)
        return (zc.view(T, H * K) @ Wc.transpose(1, 2).reshape(H * K, Cc)) * (1.0 / H)

    @staticmethod
    def backward(ctx, g_out):
        with _no_autocast():
            return _GatLayerMH._backward(ctx, g_out)

    @staticmethod
    def _backward(ctx, g_out):
        x, W, att_src, att_dst, rowptr, col, a_src, a_dst, z, rmax, rsum, V = ctx.saved_tensors
        T, K, H, Cc, slope, concat = ctx.dims
        dt = torch.bfloat16 if ctx.amp else torch.float32
        g = g_out.to(dt).contiguous()
        zc, Wc = z.to(dt), W.to(dt).view(H, Cc, K)
        if concat:
            g3 = g.view(T, H, Cc).transpose(0, 1)                                # [H, T, C]
            g_z = torch.bmm(g3, Wc).transpose(0, 1).float().contiguous()        # [T, H, K]
            gW = torch.bmm(g3.transpose(1, 2), zc.transpose(0, 1)).float().reshape(H * Cc, K)
        else:
            g = g * (1.0 / H)
            g_z = (g @ Wc.transpose(1, 2).reshape(H * K, Cc).t()).float().view(T, H, K)
            gW = _wgrad(g, zc.view(T, H * K)).view(Cc, H, K).transpose(0, 1).reshape(H * Cc, K)
        want_gx = ctx.needs_input_grad[0]
        g_x, g_as, g_ad, g_V, gathered = _gat_kernels_backward(x, rowptr, col, a_src, a_dst, z, rmax, rsum, g_z, V,
                                                               slope, want_gx, ctx.drop)
        if want_gx:                                                              # a_src = x V_src^T, a_dst = x[:T] V_dst^T
            if not gathered:
                g_x.addmm_(g_as, V[0])
                g_x[:T].addmm_(g_ad, V[1])
            g_x = g_x.to(x.dtype)
        # V[s, h] = att[s, h] @ W_h
        att = torch.stack([att_src, att_dst]).to(torch.float32)                  # [2, H, C]
        gW = gW + torch.einsum("shc,shk->hck", att, g_V).reshape(H * Cc, K)
        g_att = torch.einsum("shk,hck->shc", g_V, W.to(torch.float32).view(H, Cc, K))
        return (g_x, gW.to(W.dtype), g_att[0].to(att_src.dtype), g_att[1].to(att_dst.dtype), None, None, None, None,
                None, None)


class _GatLayer(torch.autograd.Function):
    """GATConv(heads=1) on ((x, x[:T]), adj_t) as ONE node, in aggregate-then-project form:

        att . (W x_j) = x_j . (W^T att)          -> the logits need two K-vectors, not the projected rows
        sum_j alpha_ij (W x_j) = W sum_j alpha_ij x_j   -> aggregate raw rows, project the T targets only

    The same function as projecting all S source rows first (PyG's order), with S/T times less GEMM work
    and -- in the first layer -- 128-wide fp16 rows in the gather instead of 256-wide fp32 ones.

    x rows fp32, fp16 or bf16 (the kernels' element code); v, the logits, z and the softmax statistics are fp32.  Under
    bf16 autocast the projection z @ W^T runs in bf16 (bf16 output), and the backward's GEMMs too."""

    @staticmethod
    def forward(ctx, x, W, att_src, att_dst, rowptr, col, T, slope):
        ctx.amp = amp_bf16()
        with _no_autocast():
            return _GatLayer._forward(ctx, x, W, att_src, att_dst, rowptr, col, T, slope)

    @staticmethod
    def _forward(ctx, x, W, att_src, att_dst, rowptr, col, T, slope):
        v = torch.stack([att_src, att_dst]).to(torch.float32) @ W.to(torch.float32)   # [2, K]: W^T att_src, W^T att_dst
        # the H = 1 buffers ([S, 1], [T, 1], [T, 1, K]) are the [S], [T], [T, K] ones: views where torch wants those
        a_src, a_dst, z, rmax, rsum, _ = _gat_kernels_forward(x, v[0], v[1], rowptr, col, T, 1, slope)
        z = z.view(T, x.size(1))
        ctx.save_for_backward(x, W, att_src, att_dst, rowptr, col, a_src, a_dst, z, rmax, rsum, v)
        ctx.dims = (T, float(slope))
        if ctx.amp:
            return z.to(torch.bfloat16) @ W.to(torch.bfloat16).t()
        return z @ W.t()

    @staticmethod
    def backward(ctx, g_out):
        with _no_autocast():
            return _GatLayer._backward(ctx, g_out)

    @staticmethod
    def _backward(ctx, g_out):
        x, W, att_src, att_dst, rowptr, col, a_src, a_dst, z, rmax, rsum, v = ctx.saved_tensors
        T, slope = ctx.dims
        g_out = g_out.contiguous()
        if ctx.amp:                                                          # bf16 GEMMs, fp32 results
            g16 = g_out.to(torch.bfloat16)
            gW = _wgrad(g16, z.to(torch.bfloat16))                           # [N, K] fp32
            g_z = (g16 @ W.to(torch.bfloat16)).float()                       # [T, K]
        else:
            gW = _wgrad(g_out, z)                                            # [N, K]
            g_z = g_out @ W                                                  # [T, K]
        want_gx = ctx.needs_input_grad[0]
        g_x, g_as, g_ad, g_v, gathered = _gat_kernels_backward(x, rowptr, col, a_src, a_dst, z, rmax, rsum, g_z, v,
                                                               slope, want_gx, None)
        g_v = g_v.view(2, -1)                                                # [2, 1, K] as [2, K]
        if want_gx:                                                          # a_src = x v_src, a_dst = x[:T] v_dst
            if not gathered:
                g_x.addr_(g_as.view(-1), v[0])
                g_x[:T].addr_(g_ad.view(-1), v[1])
            g_x = g_x.to(x.dtype)
        # v = [att_src; att_dst] @ W
        att = torch.stack([att_src, att_dst]).to(torch.float32)
        gW = gW + att.t() @ g_v                                              # [N, 2] @ [2, K]
        g_att = g_v @ W.t()                                                  # [2, N]
        return g_x, gW, g_att[0].to(att_src.dtype), g_att[1].to(att_dst.dtype), None, None, None, None


class _AttentionModel(_ConvModel):
    """The shape GAT, GATv2 and GraphTransformer share: ``num_layers`` convs of the class ``conv`` (keywords ``kw``),
    ReLU + dropout 0.5 between layers, log_softmax.  Every hidden layer is ``heads`` heads of ``hidden_channels // heads``
    channels, concatenated; the last layer is the mean of its heads (``last_concat``: their concatenation)."""

    def __init__(self, conv, in_channels, hidden_channels, out_channels, num_layers, heads, last_concat=False, **kw):
        super().__init__()
        _check_heads(heads)
        if hidden_channels % heads != 0:
            raise ValueError(f"hidden_channels ({hidden_channels}) must be a multiple of heads ({heads})")
        self.num_layers = num_layers
        self.hidden_channels = hidden_channels
        self.heads = heads
        c = hidden_channels // heads
        self.convs = torch.nn.ModuleList()
        self.convs.append(conv(in_channels, c, heads=heads, concat=True, **kw))
        for _ in range(num_layers - 2):
            self.convs.append(conv(hidden_channels, c, heads=heads, concat=True, **kw))
        self.convs.append(conv(hidden_channels, out_channels, heads=heads, concat=last_concat, **kw))
        self.reset_parameters()

    def forward(self, x, adjs):
        if isinstance(x, (TableRows, RowRefs)):          # (the fused first layer exists for SAGE)
            x = x.materialize()
        # the reference converts the features to fp32 first (models.py:221); the convs here read the fp16 rows directly
        # (exact: every fp16 value is an fp32 value)
        for i, (adj_t, _e_id, size) in enumerate(adjs):
            x_target = x[:size[1]]
            x = self.convs[i]((x, x_target), adj_t)
            if i != self.num_layers - 1:
                x = relu_dropout(x, 0.5, self.training)
        return torch.log_softmax(x, dim=-1)


class GAT(_LayerwiseInference, _AttentionModel):
    """The reference's GAT (driver/models.py:195-231): ``num_layers`` GATConv(bias=False), ReLU + dropout 0.5 between
    layers, log_softmax.

    ``heads`` (keyword only, default 1): heads=1 is the reference model.  heads=H > 1 follows PyG's GAT examples, with
    the hidden WIDTH kept: every hidden layer is GATConv(d_in, hidden_channels // H, heads=H, concat=True), so its
    output is still ``hidden_channels`` wide ("3 x 256, heads=4" is four heads of 64), and the last layer is
    GATConv(hidden_channels, out_channels, heads=H, concat=False), the mean of its heads.  ``hidden_channels`` must be
    a multiple of ``heads``.

    ``attn_dropout`` (keyword only, default 0): GATConv's ``dropout`` of every conv, PyG's dropout on the attention
    coefficients (p = 0.6 in the GAT paper).  Training only: eval mode and the inference drivers score the model exactly
    as the same model with 0."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, *, heads=1, attn_dropout=0.0):
        # heads=1, the reference model: the last layer keeps GATConv's default concat=True too (one head: the same
        # function, and with attn_dropout the GEMM spelling _GatLayerMH has always run for it)
        super().__init__(GATConv, in_channels, hidden_channels, out_channels, num_layers, heads, last_concat=heads == 1,
                         bias=False, dropout=attn_dropout)


# --------------------------------------------------------------------------------------------
# GATv2  (PyG's GATv2Conv, "dynamic attention": csrc/gatv2.hip, spp.h f3v)
# --------------------------------------------------------------------------------------------
def _gatv2_reference(x_l, x_r, att, rowptr, col, slope, p=0.0):
    """GATv2Conv's message passing in PyG's order, in plain torch ops, on the projected rows: x_l [S, H, C] = lin_l(x),
    x_r [T, H, C] = lin_r(x_target), att [H, C] -> out [T, H, C] (fp32; float64 for float64 rows).  The path for
    everything the kernels do not read: CPU tensors, head counts outside {1, 2, 4, 8}, C with C / 4 not a power of two,
    H * C > 1024, and share_weights with a target block that is not the prefix of x.
    set_diag: diagonal entries dropped, one self loop (i, i) per target, whose message is source row i.
    p > 0 (training): F.dropout on alpha -- torch's own mask, from the generator of alpha's device, NOT the kernels'
    counter-based one (_attn_keep_reference), which the rows the kernels read get (spp.h f3x)."""
    T = x_r.size(0)
    dt = torch.float64 if x_l.dtype == torch.float64 else torch.float32
    x_l, x_r, att = x_l.to(dt), x_r.to(dt), att.to(dt)
    src, dst = _with_self_loops(rowptr, col, T)
    e = (F.leaky_relu(x_l[src] + x_r[dst], slope) * att).sum(-1)            # [E', H]
    return _softmax_aggregate(e, src, dst, x_l, T, p)


def _gatv2_desc(x_l, x_r, att, rowptr, col, slope, out, rmax, rsum, **grads):
    """spp_gatv2_desc for projected rows x_l [S, D], x_r [T, D] (unit column stride, one dtype) and att [H, C] fp32"""
    H, Cc = att.shape
    S, T, D = x_l.size(0), x_r.size(0), H * Cc
    return nat.Gatv2Desc(heads=H, x_elem=_ELEM[x_l.dtype], negative_slope=float(slope), rowptr_dev=_p(rowptr),
                         col_dev=_p(col), num_targets=T, num_sources=S, C=Cc, x_l_dev=_p(x_l),
                         x_l_stride_elems=x_l.stride(0) if S > 1 else D, x_r_dev=_p(x_r),
                         x_r_stride_elems=x_r.stride(0) if T > 1 else D, att_dev=_p(att), out_dev=_p(out),
                         row_max_dev=_p(rmax), row_sum_dev=_p(rsum), **{k: _p(v) for k, v in grads.items()})


def _attn_kernels_read(H, Cc, *rows):
    """the rows and widths the GATv2 / Transformer kernel pair accepts (spp.h f3v, f3y): CUDA matrices of one fp32 / fp16
    / bf16 dtype with unit column stride and rows aligned to 4 elements, H in {1, 2, 4, 8}, C % 4 == 0 with C / 4 a power
    of two, H * C <= 1024"""
    g = Cc // 4
    x = rows[0]
    return (x.is_cuda and H in _ATTN_HEADS and Cc > 0 and Cc % 4 == 0 and g & (g - 1) == 0 and H * Cc <= 1024 and
            x.dtype in _ELEM and
            all(t.dtype == x.dtype and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and
                t.data_ptr() % (4 * t.element_size()) == 0 for t in rows))


def _gatv2_kernels_read(x_l, x_r, H, Cc):
    return _attn_kernels_read(H, Cc, x_l, x_r)


def _attn_forward(ctx, name, desc, T, H, Cc, p, device):
    """What the forwards of _GATv2Layer and _TransformerLayer share: the new out [T, H, C] and softmax statistics rmax,
    rsum [T, H] (fp32), ctx.drop = (p, seed) with the seed drawn here (_attn_seed), or None for p = 0, and the one call
    of the entry `name` (_call_drop) on desc(out, rmax, rsum)."""
    L = nat.load()
    nat.require_device()
    f32 = dict(dtype=torch.float32, device=device)
    out = torch.empty((T, H, Cc), **f32)
    rmax, rsum = torch.empty((T, H), **f32), torch.empty((T, H), **f32)
    ctx.drop = (float(p), _attn_seed()) if p > 0.0 else None
    _call_drop(L, name, (C.byref(desc(out, rmax, rsum)), _stream()), ctx.drop)
    return out, rmax, rsum


def _grad_back(g, row, wanted=True):
    """a kernel's fp32 gradient in its row matrix's dtype; None if it was not computed or nobody wants it"""
    return g.to(row.dtype) if wanted and g is not None else None


class _GATv2Layer(torch.autograd.Function):
    """GATv2Conv's message passing as ONE node on the projected rows: (x_l [S, D], x_r [T, D], att [H, C]) -> out
    [T, H, C] fp32, spp_gatv2_forward / spp_gatv2_backward.  The rows are fp32, fp16 or bf16 (under bf16 autocast the
    projections outside the node give bf16 rows, which the kernels read as such); x_r may be a view of x_l
    (share_weights).  The node runs with autocast off, returns fp32 and casts grad_xl / grad_xr back to the rows' dtype;
    att and its gradient are fp32.  p > 0: attention dropout inside the kernels (spp.h f3x) -- the forward draws a seed
    from torch's CPU generator (_attn_forward), and both directions call the _drop entries with (p, training = 1, seed),
    so the backward applies the forward's mask; p = 0 calls the entries without dropout."""

    @staticmethod
    def forward(ctx, x_l, x_r, att, rowptr, col, slope, p=0.0):
        with _no_autocast():
            H, Cc = att.shape
            att32 = att.detach().to(torch.float32).contiguous()
            out, rmax, rsum = _attn_forward(
                ctx, "spp_gatv2_forward", lambda *o: _gatv2_desc(x_l, x_r, att32, rowptr, col, slope, *o),
                x_r.size(0), H, Cc, p, x_l.device)
            ctx.save_for_backward(x_l, x_r, att32, rowptr, col, out, rmax, rsum)
            ctx.slope, ctx.att_dtype = float(slope), att.dtype
            return out

    @staticmethod
    def backward(ctx, g):
        with _no_autocast():
            x_l, x_r, att32, rowptr, col, out, rmax, rsum = ctx.saved_tensors
            H, Cc = att32.shape
            S, T, D = x_l.size(0), x_r.size(0), H * Cc
            g = g.to(torch.float32).contiguous()
            f32 = dict(dtype=torch.float32, device=x_l.device)
            g_xl = torch.zeros((S, D), **f32) if ctx.needs_input_grad[0] else None
            g_xr, g_att = torch.empty((T, D), **f32), torch.empty((H, Cc), **f32)
            d = _gatv2_desc(x_l, x_r, att32, rowptr, col, ctx.slope, out, rmax, rsum, grad_out_dev=g, grad_x_l_dev=g_xl,
                            grad_x_r_dev=g_xr, grad_att_dev=g_att)
            _call_drop(nat.load(), "spp_gatv2_backward", (C.byref(d), _stream()), ctx.drop)
            return (_grad_back(g_xl, x_l), _grad_back(g_xr, x_r, ctx.needs_input_grad[1]), g_att.to(ctx.att_dtype),
                    None, None, None, None)


class GATv2Conv(torch.nn.Module):
    """torch_geometric.nn.GATv2Conv(in, out, heads=1, concat=True, negative_slope=0.2, dropout=0, add_self_loops=True,
    bias=True, share_weights=False) on a bipartite ((x, x_target), adj_t), with PyG's parameter names (a PyG state dict
    loads): lin_l (sources) and lin_r (targets; the SAME module as lin_l with share_weights), both [H * out, in] with a
    bias when ``bias``; att [1, H, out]; bias of the output's width (H * out with ``concat``, else out).

        x_l = lin_l(x) [S, H, C],  x_r = lin_r(x_target) [T, H, C]
        e_ij^h = att[h] . leaky_relu(x_l[j,h] + x_r[i,h]),   out[i,h] = sum_j softmax_j(e_ij^h) x_l[j,h]

    over row i without its diagonal entries plus one self loop whose message is source row i (GATConv's convention
    here).  The projections are ordinary F.linear calls; the message passing is _GATv2Layer (csrc/gatv2.hip) for CUDA
    rows with H in {1, 2, 4, 8}, C % 4 == 0 with C / 4 a power of two and H * C <= 1024, and _gatv2_reference, the same
    function in plain torch ops, for everything else.  With share_weights and x_target the prefix of x, x_r is the view
    x_l[:T]: no second GEMM, and autograd sums the two gradients through the view; share_weights with any other
    x_target takes the reference path.

    ``dropout`` = p in [0, 1): F.dropout(alpha, p, training) on the attention coefficients of every (entry, head), the
    self loop included; the softmax itself runs over all entries.  p = 0 and eval mode run exactly the paths above.  In
    training with p > 0 the rows the kernels read take _GATv2Layer with the mask generated inside its kernels from a
    seed drawn from torch's CPU generator (spp.h f3x; GATConv's rule, _attn_keep_reference restates it: torch.manual_seed
    makes a run repeatable); everything else takes _gatv2_reference with F.dropout on its alpha: torch's own mask there,
    not the kernels'.  No parameter or buffer: the state dict does not change."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, bias=True,
                 share_weights=False):
        super().__init__()
        _check_heads(heads)
        _check_attn_dropout(dropout)
        self.heads, self.out_channels, self.concat = heads, out_channels, bool(concat)
        self.negative_slope = negative_slope
        self.dropout = float(dropout)
        self.share_weights = bool(share_weights)
        self.lin_l = torch.nn.Linear(in_channels, heads * out_channels, bias=bool(bias))
        self.lin_r = self.lin_l if share_weights else torch.nn.Linear(in_channels, heads * out_channels, bias=bool(bias))
        self.att = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        width = heads * out_channels if concat else out_channels
        self.bias = torch.nn.Parameter(torch.zeros(width)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_l, self.lin_r):                    # PyG: glorot weights, zero biases
            torch.nn.init.xavier_uniform_(lin.weight)
            if lin.bias is not None:
                torch.nn.init.zeros_(lin.bias)
        torch.nn.init.xavier_uniform_(self.att)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x_pair, adj_t):
        x, x_target = x_pair
        rowptr, col, _ = adj_t.csr()
        S, T, H, Cc = x.size(0), x_target.size(0), self.heads, self.out_channels
        prefix = _is_prefix(x, x_target) and T <= S
        if not torch.is_autocast_enabled(x.device.type):        # (autocast casts the GEMM's operands itself)
            x, x_target = x.to(self.lin_l.weight.dtype), x_target.to(self.lin_r.weight.dtype)
        x_l = self.lin_l(x)
        x_r = x_l[:T] if self.share_weights and prefix else self.lin_r(x_target)
        att = self.att.view(H, Cc)
        p = self.dropout if self.training else 0.0
        if (prefix or not self.share_weights) and _gatv2_kernels_read(x_l, x_r, H, Cc):
            out = _GATv2Layer.apply(x_l, x_r, att, rowptr, col, self.negative_slope, p)
        else:
            out = _gatv2_reference(x_l.view(S, H, Cc), x_r.view(T, H, Cc), att, rowptr, col, self.negative_slope, p)
        out = out.reshape(T, H * Cc) if self.concat else out.mean(1)
        return out if self.bias is None else out + self.bias


class GATv2(_LayerwiseInference, _AttentionModel):
    """GAT's shape with GATv2Conv layers: ``num_layers`` GATv2Conv(bias=False), ReLU + dropout 0.5 between layers,
    log_softmax.  Every hidden layer is ``heads`` heads of ``hidden_channels // heads`` channels, concatenated (the hidden
    width stays ``hidden_channels``, which must be a multiple of ``heads``); the last layer is the mean of its heads.
    ``share_weights`` and ``attn_dropout`` are every conv's ``share_weights`` and ``dropout``."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, *, heads=1, share_weights=False,
                 attn_dropout=0.0):
        super().__init__(GATv2Conv, in_channels, hidden_channels, out_channels, num_layers, heads, bias=False,
                         share_weights=share_weights, dropout=attn_dropout)


# --------------------------------------------------------------------------------------------
# GraphTransformer  (PyG's TransformerConv, scaled dot-product attention: csrc/transformer_conv.hip, spp.h f3y)
# --------------------------------------------------------------------------------------------
def _transformer_reference(q, k, v, rowptr, col, scale, p=0.0):
    """TransformerConv's message passing in plain torch ops, on the projected rows: q [T, H, C] = lin_query(x_target),
    k [S, H, C] = lin_key(x), v [S, H, C] = lin_value(x) -> out [T, H, C] (fp32; float64 for float64 rows):
    e_ij^h = scale * q[i,h] . k[j,h], alpha = softmax_j(e), out[i,h] = sum_j alpha_ij^h v[j,h] over ALL CSR entries of
    row i -- no self loop, diagonal entries kept, a repeated entry counted as often as it appears -- and zeros for a
    row without entries.  The path for everything the kernels do not read: CPU tensors, head counts outside
    {1, 2, 4, 8}, C with C / 4 not a power of two, H * C > 1024.  p > 0 (training): F.dropout on alpha -- torch's own
    mask, from the generator of alpha's device, NOT the kernels' counter-based one (_attn_keep_reference), which the
    rows the kernels read get (spp.h f4a)."""
    T = q.size(0)
    dt = torch.float64 if q.dtype == torch.float64 else torch.float32
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    dst = torch.repeat_interleave(torch.arange(T, device=col.device), rowptr[1:] - rowptr[:-1])
    e = (q[dst] * k[col]).sum(-1) * scale                                   # [E, H]
    return _softmax_aggregate(e, col, dst, v, T, p)


def _transformer_desc(q, k, v, H, rowptr, col, scale, out, rmax, rsum, **grads):
    """spp_transformer_desc for projected rows q [T, D], k and v [S, D] (unit column stride, one dtype)"""
    S, T, D = k.size(0), q.size(0), q.size(1)
    return nat.TransformerDesc(heads=H, x_elem=_ELEM[q.dtype], scale=float(scale), rowptr_dev=_p(rowptr),
                               col_dev=_p(col), num_targets=T, num_sources=S, C=D // H, q_dev=_p(q),
                               q_stride_elems=q.stride(0) if T > 1 else D, k_dev=_p(k),
                               k_stride_elems=k.stride(0) if S > 1 else D, v_dev=_p(v),
                               v_stride_elems=v.stride(0) if S > 1 else D, out_dev=_p(out), row_max_dev=_p(rmax),
                               row_sum_dev=_p(rsum), **{n: _p(t) for n, t in grads.items() if t is not None})


def _transformer_kernels_read(q, k, v, H, Cc):
    return _attn_kernels_read(H, Cc, q, k, v)


class _TransformerLayer(torch.autograd.Function):
    """TransformerConv's message passing as ONE node on the projected rows: (q [T, D], k [S, D], v [S, D]) -> out
    [T, H, C] fp32, spp_transformer_forward / spp_transformer_backward.  The rows are fp32, fp16 or bf16 (under bf16
    autocast the projections outside the node give bf16 rows, which the kernels read as such); k and v may be views
    of one [S, 2 D] matrix.  The node runs with autocast off, returns fp32 and casts grad_q / grad_k / grad_v back to
    the rows' dtype; a gradient nobody needs is not computed (NULL in the descriptor).  p > 0: attention dropout
    inside the kernels (spp.h f4a), as _GATv2Layer's: seed and call in _attn_forward, the same (p, seed) in the
    backward."""

    @staticmethod
    def forward(ctx, q, k, v, rowptr, col, heads, scale, p=0.0):
        with _no_autocast():
            T, D = q.shape
            out, rmax, rsum = _attn_forward(
                ctx, "spp_transformer_forward", lambda *o: _transformer_desc(q, k, v, heads, rowptr, col, scale, *o),
                T, heads, D // heads, p, q.device)
            ctx.save_for_backward(q, k, v, rowptr, col, out, rmax, rsum)
            ctx.heads, ctx.scale = int(heads), float(scale)
            return out

    @staticmethod
    def backward(ctx, g):
        with _no_autocast():
            q, k, v, rowptr, col, out, rmax, rsum = ctx.saved_tensors
            (T, D), S = q.shape, k.size(0)
            g = g.to(torch.float32).contiguous()
            f32 = dict(dtype=torch.float32, device=q.device)
            g_q = torch.empty((T, D), **f32)
            g_k = torch.zeros((S, D), **f32) if ctx.needs_input_grad[1] else None
            g_v = torch.zeros((S, D), **f32) if ctx.needs_input_grad[2] else None
            d = _transformer_desc(q, k, v, ctx.heads, rowptr, col, ctx.scale, out, rmax, rsum, grad_out_dev=g,
                                  grad_q_dev=g_q, grad_k_dev=g_k, grad_v_dev=g_v)
            _call_drop(nat.load(), "spp_transformer_backward", (C.byref(d), _stream()), ctx.drop)
            return (_grad_back(g_q, q, ctx.needs_input_grad[0]), _grad_back(g_k, k), _grad_back(g_v, v), None, None,
                    None, None, None)


class TransformerConv(torch.nn.Module):
    """torch_geometric.nn.TransformerConv(in, out, heads=1, concat=True, beta=False, dropout=0, edge_dim=None,
    bias=True, root_weight=True) (Shi et al., "Masked Label Prediction: Unified Message Passing Model for
    Semi-Supervised Classification") on a bipartite ((x, x_target), adj_t), with PyG's parameter names (a PyG state
    dict loads): lin_key, lin_query, lin_value, each [H * out, in] with a bias; with ``root_weight`` lin_skip of the
    output's width (H * out with ``concat``, else out), whose bias is ``bias``; with ``beta and root_weight`` lin_beta
    [1, 3 * width] without a bias.

        q = lin_query(x_target) [T, H, C],  k = lin_key(x) [S, H, C],  v = lin_value(x) [S, H, C]
        e_ij^h = q[i,h] . k[j,h] / sqrt(C),   out[i,h] = sum_j softmax_j(e_ij^h) v[j,h]

    over ALL entries of row i as adj_t has them: no self loop is added, diagonal entries stay, a repeated entry counts
    as often as it appears, and a target without entries gets zeros.  Then the heads are concatenated or averaged;
    with ``root_weight`` x_r = lin_skip(x_target) is added, or, with ``beta``, out = b x_r + (1 - b) out with
    b = sigmoid(lin_beta([out, x_r, out - x_r])).  The projections, the skip and the gate are plain torch; the message
    passing is _TransformerLayer (csrc/transformer_conv.hip) for CUDA rows with H in {1, 2, 4, 8}, C % 4 == 0 with
    C / 4 a power of two and H * C <= 1024, and _transformer_reference, the same function in plain torch ops, for
    everything else.

    ``dropout`` = p in [0, 1): F.dropout(alpha, p, training) on the attention coefficients of every (entry, head); the
    softmax itself runs over all entries.  p = 0 and eval mode run exactly the paths above.  In training with p > 0 the
    rows the kernels read take _TransformerLayer with the mask generated inside its kernels from a seed drawn from
    torch's CPU generator (spp.h f4a; GATConv's rule without self loops, _attn_keep_reference(E, 0, H, p, seed) restates
    it: torch.manual_seed makes a run repeatable); everything else takes _transformer_reference with F.dropout on its
    alpha: torch's own mask there, not the kernels'.  No parameter or buffer: the state dict does not change.
    ``edge_dim`` other than None (edge features) is not built: NotImplementedError."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None,
                 bias=True, root_weight=True):
        super().__init__()
        if edge_dim is not None:
            raise NotImplementedError("TransformerConv: edge features (edge_dim) are not built; use edge_dim=None")
        _check_heads(heads, bool_ok=False)
        _check_attn_dropout(dropout)
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.root_weight = bool(concat), bool(root_weight)
        self.beta = bool(beta) and self.root_weight
        self.dropout = float(dropout)
        self.lin_key = torch.nn.Linear(in_channels, heads * out_channels)
        self.lin_query = torch.nn.Linear(in_channels, heads * out_channels)
        self.lin_value = torch.nn.Linear(in_channels, heads * out_channels)
        width = heads * out_channels if concat else out_channels
        self.lin_skip = torch.nn.Linear(in_channels, width, bias=bool(bias)) if self.root_weight else None
        self.lin_beta = torch.nn.Linear(3 * width, 1, bias=False) if self.beta else None
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip, self.lin_beta):   # PyG: each Linear's own
            if lin is not None:
                lin.reset_parameters()

    def forward(self, x_pair, adj_t):
        x, x_target = x_pair
        rowptr, col, _ = adj_t.csr()
        S, T, H, Cc = x.size(0), x_target.size(0), self.heads, self.out_channels
        if not torch.is_autocast_enabled(x.device.type):        # (autocast casts the GEMM's operands itself)
            x, x_target = x.to(self.lin_key.weight.dtype), x_target.to(self.lin_query.weight.dtype)
        q, k, v = self.lin_query(x_target), self.lin_key(x), self.lin_value(x)
        scale = 1.0 / float(Cc) ** 0.5
        p = self.dropout if self.training else 0.0
        if _transformer_kernels_read(q, k, v, H, Cc) and (p == 0.0 or q.is_cuda):
            out = _TransformerLayer.apply(q, k, v, rowptr, col, H, scale, *((p,) if p > 0.0 else ()))
        else:
            out = _transformer_reference(q.view(T, H, Cc), k.view(S, H, Cc), v.view(S, H, Cc), rowptr, col, scale, p)
        out = out.reshape(T, H * Cc) if self.concat else out.mean(1)
        if self.root_weight:
            x_r = self.lin_skip(x_target)
            if self.lin_beta is not None:
                b = torch.sigmoid(self.lin_beta(torch.cat([out, x_r, out - x_r], -1)))
                out = b * x_r + (1 - b) * out
            else:
                out = out + x_r
        return out


class GraphTransformer(_AttentionModel):
    """GAT's shape with TransformerConv layers (the UniMP model without label propagation): ``num_layers``
    TransformerConv, ReLU + dropout 0.5 between layers, log_softmax.  Every hidden layer is ``heads`` heads of
    ``hidden_channels // heads`` channels, concatenated (the hidden width stays ``hidden_channels``, which must be a
    multiple of ``heads``); the last layer is the mean of its heads.  ``beta`` and ``attn_dropout`` are every conv's
    ``beta`` and ``dropout``; with ``attn_dropout`` > 0 a training step stays on the HIP kernels (the mask is drawn
    inside them, spp.h f4a), and eval mode and the layer-wise scoring below apply no dropout.

    There is no ``inference`` method.  Exact layer-wise scoring over the resident graph is
    ``inference.layerwise_inference(model, ...)`` (``inference.evaluate`` for predictions and loss;
    csrc/graph_transformer.hip); the partitioned, field and fp8 entries are not built for this model.  It can also be
    evaluated batch-wise, through this forward on sampled batches in eval mode, as the reference evaluates its
    models."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, *, heads=1, beta=False, attn_dropout=0.0):
        _check_heads(heads, bool_ok=False)
        super().__init__(TransformerConv, in_channels, hidden_channels, out_channels, num_layers, heads, beta=beta,
                         dropout=attn_dropout)


# --------------------------------------------------------------------------------------------
# GIN  (driver/models.py:234-283: GINConv(Sequential(Linear, BatchNorm1d, ReLU, Linear, ReLU)), eps = 0)
# --------------------------------------------------------------------------------------------
_SUM_GATHER_MIN_WORK = _GATHER_MIN_WORK     # (the name the sum's tests know it by)


class _SumAggregate(torch.autograd.Function):
    """out[t] = s * x[t] + sum_{e in row t} x[col[e]]  (fp32 [T, F]; targets are the first T rows of x).

    ``x`` is a feature matrix (fp16 / fp32 / bf16, any row stride), a TableRows or a RowRefs: the latter two are read in
    place (spp_agg_forward's SPP_AGG_TABLE / SPP_AGG_ROWS sources) and get no gradient.  With s == 0 the targets' rows are not read.
    Under bf16 autocast the result is bf16 (fp32 sums, rounded once)."""

    @staticmethod
    def forward(ctx, x, rowptr, col, num_targets, scale):
        nat.require_device()
        S, Fdim = x.size(0), x.size(1)
        assert x.is_cuda and rowptr.is_cuda and col.is_cuda and _readable(x), "fp16 / fp32 / bf16 / fp8 rows on the GPU"
        assert num_targets <= S or scale == 0.0, "the targets are the first rows of the sources"
        if _is_fp8(x):
            _no_input_grad(ctx, "sum_aggregate")
        out = _agg_forward(nat.SPP_AGG_SUM, rowptr, col, num_targets, x, torch.bfloat16 if amp_bf16() else torch.float32,
                           scale=scale)
        ctx.save_for_backward(rowptr, col)
        ctx.shape = (S, Fdim, num_targets)
        ctx.scale = float(scale)
        ctx.in_dtype = x.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:            # the first layer: the batch's features are no leaves
            return None, None, None, None, None
        rowptr, col = ctx.saved_tensors
        S, Fdim, T = ctx.shape
        # bf16 / fp32 gradient in, the input's dtype out (fp16 through an fp32 buffer)
        odt = ctx.in_dtype if ctx.in_dtype in (torch.float32, torch.bfloat16) else torch.float32
        grad_x = _agg_backward(nat.SPP_AGG_SUM, rowptr, col, T, S, _grad_in(grad_out), Fdim, odt,
                               gather=col.numel() * Fdim >= _SUM_GATHER_MIN_WORK, scale=ctx.scale)
        return grad_x.to(ctx.in_dtype), None, None, None, None


def sum_aggregate(x, rowptr, col, num_targets, scale=1.0):
    """scale * x[:T] + the sum of each target's neighbour rows (GINConv's aggregation with scale = 1 + eps)"""
    return _SumAggregate.apply(x, rowptr, col, num_targets, scale)


class GINConv(torch.nn.Module):
    """torch_geometric.nn.GINConv(nn, eps=0., train_eps=False) on a bipartite ((x, x_target), adj_t):
    nn((1 + eps) * x_target + sum_j x_j), the sum over every entry of the target's row.  ``eps`` is a buffer.

    ``forward(x, adj_t, size)`` with a single ``x`` (a matrix, TableRows or RowRefs) takes the first size[1] rows
    as the targets (the MFG contract)."""

    def __init__(self, nn, eps=0., train_eps=False, fused_norm=False):
        super().__init__()
        if train_eps:
            raise NotImplementedError("the reference models use GINConv with a fixed eps (train_eps=False)")
        self.nn = nn
        # fused_norm: nn is _gin_mlp's Sequential and its BatchNorm1d + ReLU run as batch_norm_act
        self.fused_norm = fused_norm
        self.initial_eps = eps
        self.register_buffer("eps", torch.empty(1))
        self._scale_key = self._scale_val = None
        self.reset_parameters()

    def reset_parameters(self):
        for m in self.nn.children():                     # PyG's reset(nn)
            if hasattr(m, "reset_parameters"):
                m.reset_parameters()
        with torch.no_grad():
            self.eps.fill_(self.initial_eps)

    def _scale(self):
        # 1 + eps as a host float for the kernel, read back only when the buffer has changed (a device read syncs)
        key = (self.eps.data_ptr(), self.eps._version)
        if key != self._scale_key:
            self._scale_val, self._scale_key = 1.0 + float(self.eps), key
        return self._scale_val

    def forward(self, x, adj_t, size=None):
        rowptr, col, _ = adj_t.csr()
        if isinstance(x, tuple):
            x, x_target = x
            T = x_target.size(0)
        else:
            x_target = None
            T = int(size[1]) if size is not None else x.size(0)
        if not _readable(x):
            x = (x.materialize() if isinstance(x, (TableRows, RowRefs)) else x).to(torch.float32).contiguous()
            if x_target is not None:
                x_target = x[:T]
        prefix = x_target is None or (isinstance(x, torch.Tensor) and _is_prefix(x, x_target) and
                                      x_target.size(1) == x.size(1))
        if prefix:                                                          # x_target = x[:T] (the MFG contract)
            h = _SumAggregate.apply(x, rowptr, col, T, self._scale())
        else:                                                               # a foreign target matrix
            h = _SumAggregate.apply(x, rowptr, col, T, 0.0)
            h = h + (1 + self.eps) * x_target.to(h.dtype)
        if self.fused_norm:
            h = batch_norm_act(self.nn[0](h), self.nn[1], act="relu")
            return F.relu(self.nn[3](h))
        return self.nn(h)


def _gin_mlp(d_in, d_hidden):
    return torch.nn.Sequential(torch.nn.Linear(d_in, d_hidden), torch.nn.BatchNorm1d(d_hidden), torch.nn.ReLU(),
                               torch.nn.Linear(d_hidden, d_hidden), torch.nn.ReLU())


class GIN(_LayerwiseInference, _ConvModel):
    """``num_layers`` GINConv (in -> hidden, then hidden -> hidden, the last one included), then lin1, ReLU, dropout,
    lin2, log_softmax.  The first layer reads a TableRows / RowRefs input in place.  ``fused_norm=True`` runs every
    conv's BatchNorm1d + ReLU as ``batch_norm_act`` (same modules, same state dict)."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, *, dropout=0.5, fused_norm=False):
        super().__init__()
        self.num_layers = num_layers
        self.hidden_channels = hidden_channels
        self.dropout = dropout
        self.fused_norm = fused_norm
        self.convs = torch.nn.ModuleList()
        self.convs.append(GINConv(_gin_mlp(in_channels, hidden_channels), fused_norm=fused_norm))
        for _ in range(num_layers - 1):
            self.convs.append(GINConv(_gin_mlp(hidden_channels, hidden_channels), fused_norm=fused_norm))
        self.lin1 = torch.nn.Linear(hidden_channels, hidden_channels)
        self.lin2 = torch.nn.Linear(hidden_channels, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()

    def forward(self, x, adjs):
        # the reference converts the features to fp32 first (models.py:272); the sum reads fp16 rows directly (exact)
        for i, (adj_t, _e_id, size) in enumerate(adjs):
            if isinstance(x, (TableRows, RowRefs, Fp8Features)):
                x = self.convs[i](x, adj_t, size)
            else:
                x = self.convs[i]((x, x[:size[1]]), adj_t)
        x = F.relu(self.lin1(x))
        x = F.dropout(x, p=self.dropout, training=self.training)
        return torch.log_softmax(self.lin2(x), dim=-1)


# --------------------------------------------------------------------------------------------
# Edge-weighted aggregation, gcn_norm, GCNConv and GCN  (driver/models.py:343-381; csrc/aggregate_weighted.hip, spp.h f3r)
# --------------------------------------------------------------------------------------------
def _entry_rows(rowptr, col, T):
    """(the target row of every entry [E], E) of the hop's first T rows"""
    E = int(rowptr[T])
    deg = rowptr[1:T + 1] - rowptr[:T]
    return torch.repeat_interleave(torch.arange(T, device=col.device), deg, output_size=E), E


def _weighted_reference(x, rowptr, col, weight, T, self_weight=None):
    """Plain torch restatement of spp_agg_weighted_forward on a dense x: out[t] = sum_k w[k] * x[col[k]] over row t
    (+ self_weight[t] * x[t]), [T, F].  Computed in fp32 -- in float64 when x is float64 -- on x's device, and
    differentiable in x, weight and self_weight."""
    dt = torch.float64 if x.dtype == torch.float64 else torch.float32
    x = x.to(dt)
    row, E = _entry_rows(rowptr, col, T)
    out = torch.zeros((T, x.size(1)), dtype=dt, device=x.device)
    out = out.index_add(0, row, x[col[:E]] * weight[:E].to(dt).unsqueeze(1))
    if self_weight is not None:
        out = out + self_weight.to(dt).unsqueeze(1) * x[:T]
    return out


def _gcn_fill(add_self_loops, improved):
    return (2 if improved else 1) if add_self_loops else 0


def _gcn_norm_reference(rowptr, col, T, edge_weight=None, *, add_self_loops=True, improved=False, dtype=None):
    """Plain torch restatement of spp_gcn_norm: PyG's gcn_norm of the hop padded to a square (rows >= T are empty), so a
    source that is no target has degree ``fill``.  (coef [E], self_coef [T]) in ``dtype`` (default: float64 if
    edge_weight is, else fp32)."""
    if dtype is None:
        dtype = torch.float64 if edge_weight is not None and edge_weight.dtype == torch.float64 else torch.float32
    fill = float(_gcn_fill(add_self_loops, improved))
    row, E = _entry_rows(rowptr, col, T)
    w = torch.ones(E, dtype=dtype, device=col.device) if edge_weight is None else edge_weight[:E].to(dtype)
    deg = torch.full((T,), fill, dtype=dtype, device=col.device).index_add(0, row, w)
    dinv = deg.pow(-0.5)
    dinv = dinv.masked_fill(dinv == float("inf"), 0.0)
    c = col[:E]
    foreign = torch.full((), fill ** -0.5 if fill > 0 else 0.0, dtype=dtype, device=col.device)
    dsrc = torch.where(c < T, dinv[c.clamp(max=max(T - 1, 0))], foreign) if T > 0 else foreign.expand(E)
    return dinv[row] * w * dsrc, fill * dinv * dinv


def _check_hop(what, rowptr, col, num_targets):
    for name, t in (("rowptr", rowptr), ("col", col)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError(f"{what}: {name} must be a 1-D int64 tensor")
    if not isinstance(num_targets, int) or num_targets < 0 or rowptr.numel() < num_targets + 1:
        raise ValueError(f"{what}: num_targets must be an int in [0, {rowptr.numel() - 1}] (rowptr has "
                         f"{rowptr.numel()} entries), got {num_targets!r}")


def _check_weights(what, name, w, n):
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 1 or w.numel() != n:
        got = f"{tuple(w.shape)} of {w.dtype}" if isinstance(w, torch.Tensor) else type(w).__name__
        raise ValueError(f"{what}: {name} must be a 1-D fp32 tensor of {n} values, got {got}")


def _check_weighted_source(what, x):
    """what the weighted kernels read, checked before any device call"""
    m = x.table if isinstance(x, TableRows) else x
    if isinstance(m, Fp8Features):
        raise ValueError(f"{what}: fp8 rows are not supported (fp32, fp16 or bf16 rows)")
    if isinstance(x, RowRefs):
        if x.dtype not in _ELEM:
            raise ValueError(f"{what}: row references must name fp32 / fp16 / bf16 rows, got {x.dtype}")
        return
    if not isinstance(m, torch.Tensor):
        raise TypeError(f"{what}: x must be a tensor, a TableRows or a RowRefs, got {type(x).__name__}")
    if m.dim() != 2 or m.dtype not in _ELEM or m.stride(1) != 1:
        raise ValueError(f"{what}: x must be a 2-D fp32 / fp16 / bf16 matrix with unit column stride, got "
                         f"{tuple(m.shape)} of {m.dtype}")


class _WeightedAggregate(torch.autograd.Function):
    """out[t] = sum_{k in row t} weight[k] * x[col[k]]  (+ self_weight[t] * x[t]; targets are the first T rows of x).

    ``x`` is a feature matrix (fp16 / fp32 / bf16, any row stride), a TableRows or a RowRefs: the latter two are read in
    place and get no gradient.  fp32 fmaf chain in CSR order, the self term last; under bf16 autocast the result is bf16
    (rounded once).  ``weight`` and ``self_weight`` get their gradients (one dot product per entry) only if they
    require one."""

    @staticmethod
    def forward(ctx, x, rowptr, col, weight, self_weight, num_targets):
        nat.require_device()
        src, _ = _rows(x)
        T, E = num_targets, col.numel()
        out = torch.empty((T, src["F"]), dtype=torch.bfloat16 if amp_bf16() else torch.float32, device=rowptr.device)
        weight = weight.contiguous()
        self_weight = self_weight.contiguous() if self_weight is not None else None
        d = nat.AggWeightedFwdDesc(out_elem=_ELEM[out.dtype], rowptr_dev=_p(rowptr), col_dev=_p(col), num_targets=T,
                                   num_edges=E, w_dev=_p(weight), self_w_dev=_p(self_weight), out_dev=_p(out),
                                   out_stride_elems=0, **src)
        nat.check(nat.load().spp_agg_weighted_forward(C.byref(d), _stream()))
        wgrad = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        ctx.save_for_backward(rowptr, col, weight, self_weight, x if wgrad and isinstance(x, torch.Tensor) else None)
        ctx.rows = x if wgrad and not isinstance(x, torch.Tensor) else None      # a TableRows / RowRefs, read again
        ctx.shape = (x.size(0), src["F"], T)
        ctx.in_dtype = x.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        rowptr, col, weight, self_weight, x = ctx.saved_tensors
        S, Fdim, T = ctx.shape
        E = col.numel()
        L = nat.load()
        g = _grad_in(grad_out)
        gs = g.stride(0) if T > 1 else 0
        grad_x = grad_w = grad_sw = None
        if ctx.needs_input_grad[0]:
            # bf16 / fp32 gradient in, the input's dtype out (fp16 through an fp32 buffer)
            odt = ctx.in_dtype if ctx.in_dtype in (torch.float32, torch.bfloat16) else torch.float32
            grad_x = torch.empty((S, Fdim), dtype=odt, device=g.device)
            nbytes = int(L.spp_agg_weighted_backward_workspace_bytes(T, S, E))
            ws = torch.empty(max(nbytes, 0), dtype=torch.uint8, device=g.device)
            d = nat.AggWeightedBwdDesc(grad_elem=_ELEM[g.dtype], out_elem=_ELEM[odt], rowptr_dev=_p(rowptr),
                                       col_dev=_p(col), num_targets=T, num_sources=S, num_edges=E, grad_out_dev=_p(g),
                                       grad_out_stride_elems=gs, F=Fdim, w_dev=_p(weight), self_w_dev=_p(self_weight),
                                       grad_x_dev=_p(grad_x))
            nat.check(L.spp_agg_weighted_backward(C.byref(d), _p(ws), nbytes, _stream()))
            grad_x = grad_x.to(ctx.in_dtype)
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            src, _ = _rows(x if x is not None else ctx.rows)
            grad_w = torch.empty(E, dtype=torch.float32, device=g.device)
            grad_sw = torch.empty(T, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[4] else None
            d = nat.AggWeightedWgradDesc(grad_elem=_ELEM[g.dtype], rowptr_dev=_p(rowptr), col_dev=_p(col), num_targets=T,
                                         num_edges=E, grad_out_dev=_p(g), grad_out_stride_elems=gs,
                                         grad_w_dev=_p(grad_w), grad_self_w_dev=_p(grad_sw), **src)
            nat.check(L.spp_agg_weighted_wgrad(C.byref(d), _stream()))
            if not ctx.needs_input_grad[3]:
                grad_w = None
        return grad_x, None, None, grad_w, grad_sw, None


def weighted_aggregate(x, rowptr, col, weight, num_targets, self_weight=None):
    """The edge-weighted neighbour sum ``out[t] = sum_k weight[k] * x[col[k]]`` over the entries k of target t's row,
    ``+ self_weight[t] * x[t]`` when ``self_weight`` is given: [num_targets, F], fp32 (bf16 under bf16 autocast).

    ``x``: an fp32 / fp16 / bf16 matrix, a TableRows or a RowRefs (read in place, no gradient); the targets are its first
    ``num_targets`` rows.  ``weight`` fp32 [E] and ``self_weight`` fp32 [num_targets]: one value per entry / target;
    both are differentiable.  On the GPU this is one autograd node on HIP kernels; CPU tensors take the plain torch
    restatement."""
    what = "weighted_aggregate"
    _check_weighted_source(what, x)
    _check_hop(what, rowptr, col, num_targets)
    _check_weights(what, "weight", weight, col.numel())
    if self_weight is not None:
        _check_weights(what, "self_weight", self_weight, num_targets)
        if num_targets > x.size(0):
            raise ValueError(f"{what}: the targets are the first rows of x: {num_targets} targets, {x.size(0)} rows")
    if not x.is_cuda:
        if not isinstance(x, torch.Tensor):
            x = x.materialize()
        return _weighted_reference(x, rowptr, col, weight, num_targets, self_weight)
    return _WeightedAggregate.apply(x, rowptr, col, weight, self_weight, num_targets)


def gcn_norm(rowptr, col, num_targets, edge_weight=None, *, add_self_loops=True, improved=False):
    """PyG's ``gcn_norm`` of an MFG hop: ``(coef [E], self_coef [num_targets])``, fp32, with
    ``coef[k] = deg[t]^-1/2 * w[k] * deg[col[k]]^-1/2`` and ``self_coef[t] = fill / deg[t]``, where ``deg`` is the row sum
    of ``A + fill * I`` on the hop padded to a square: ``fill + sum_row w`` for a target, ``fill`` for a source that is no
    target (``fill`` = 1, 2 with ``improved``, 0 without self loops).  When the hop is a whole graph (targets = sources)
    this is PyG's normalisation.  Not differentiable: an ``edge_weight`` that requires grad is refused."""
    what = "gcn_norm"
    _check_hop(what, rowptr, col, num_targets)
    if edge_weight is not None:
        _check_weights(what, "edge_weight", edge_weight, col.numel())
        if edge_weight.requires_grad:
            raise ValueError(f"{what}: edge_weight requires grad, and gcn_norm is not differentiable; pass "
                             "edge_weight.detach(), or normalise differentiable weights in torch")
    if not rowptr.is_cuda:
        return _gcn_norm_reference(rowptr, col, num_targets, edge_weight, add_self_loops=add_self_loops,
                                   improved=improved, dtype=torch.float32)
    nat.require_device()
    T, E = num_targets, col.numel()
    w = edge_weight.contiguous() if edge_weight is not None else None
    dinv = torch.empty(T, dtype=torch.float32, device=rowptr.device)
    coef = torch.empty(E, dtype=torch.float32, device=rowptr.device)
    self_coef = torch.empty(T, dtype=torch.float32, device=rowptr.device)
    d = nat.GcnNormDesc(fill=_gcn_fill(add_self_loops, improved), rowptr_dev=_p(rowptr), col_dev=_p(col), num_targets=T,
                        num_sources=T, num_edges=E, w_dev=_p(w),       # (a source beyond T is never read: S = T will do)
                        dinv_dev=_p(dinv), coef_dev=_p(coef), self_coef_dev=_p(self_coef))
    nat.check(nat.load().spp_gcn_norm(C.byref(d), _stream()))
    return coef, self_coef


class GCNConv(torch.nn.Module):
    """torch_geometric.nn.GCNConv(in, out, improved=..., add_self_loops=..., normalize=..., bias=...) on an MFG hop
    ``adj_t`` ([T, S] CSR; the targets are the first T source rows): ``lin(sum_k w_k x_k [+ self_coef * x_target]) + bias``.

    The entry weights are ``adj_t``'s values if it has any, else ones.  ``normalize=True`` passes them through
    ``gcn_norm`` (PyG's symmetric normalisation of the hop padded to a square) and adds the self term;
    ``normalize=False`` -- the reference model's setting -- is the bare weighted sum, without a self term.  The rows are
    aggregated FIRST and projected second (the GEMM has T rows instead of S); PyG projects first: the same value up to
    rounding.  Parameters: ``lin.weight`` and ``bias``, as in PyG.

    ``forward(x, adj_t, size)`` with a single ``x`` (a matrix, TableRows or RowRefs) takes the first size[1] rows as the
    targets; ``forward((x, x_target), adj_t)`` takes ``x_target`` for the self term."""

    def __init__(self, in_channels, out_channels, bias=True, *, normalize=True, improved=False, add_self_loops=True):
        super().__init__()
        self.normalize, self.improved, self.add_self_loops = bool(normalize), bool(improved), bool(add_self_loops)
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.lin.weight)                   # PyG: glorot weight, zero bias
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x, adj_t, size=None):
        rowptr, col, value = adj_t.csr()
        x_target = None
        if isinstance(x, tuple):
            x, x_target = x
        if x_target is not None:
            T = x_target.size(0)
        else:
            T = int(size[1]) if size is not None else int(adj_t.sparse_sizes()[0])
        if isinstance(x, torch.Tensor) and x.dtype not in _ELEM:
            x = x.to(torch.float32)
        prefix = x_target is None or (isinstance(x, torch.Tensor) and _is_prefix(x, x_target) and
                                      x_target.size(1) == x.size(1))
        w = value.to(torch.float32) if value is not None else None
        self_w = None
        if self.normalize:
            w, self_w = gcn_norm(rowptr, col, T, w, add_self_loops=self.add_self_loops, improved=self.improved)
            if not self.add_self_loops:
                self_w = None                                                # (all zeros)
        elif w is None:
            w = torch.ones(col.numel(), dtype=torch.float32, device=col.device)
        if prefix or self_w is None:
            h = weighted_aggregate(x, rowptr, col, w, T, self_w)
        else:                                                                # a foreign target matrix
            h = weighted_aggregate(x, rowptr, col, w, T)
            h = h + self_w.unsqueeze(1).to(h.dtype) * x_target.to(h.dtype)
        out = _tall_linear(h, self.lin.weight)
        return out if self.bias is None else out + self.bias


class GCN(_LayerwiseInference, _ConvModel):
    """The reference's GCN (driver/models.py:343-381): ``num_layers`` GCNConv(bias=False, improved=False), each but the
    last followed by BatchNorm1d, ReLU and dropout 0.5, then log_softmax; ``bns`` holds ``num_layers`` BatchNorm1d(hidden)
    of which the last is unused, as in the reference.  ``normalize`` (keyword only; the reference: False) is handed to
    every conv.  ``fused_norm=True`` runs each tail as ``batch_norm_act(act="relu", p=0.5)`` (same modules, same state
    dict).  The first layer reads a TableRows / RowRefs input in place."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, *, normalize=False, fused_norm=False):
        super().__init__()
        kwargs = dict(normalize=normalize, bias=False, improved=False)
        self.num_layers = num_layers
        self.hidden_channels = hidden_channels
        self.normalize = bool(normalize)
        self.fused_norm = fused_norm
        self.convs = torch.nn.ModuleList()
        self.bns = torch.nn.ModuleList()
        self.convs.append(GCNConv(in_channels, hidden_channels, **kwargs))
        self.bns.append(torch.nn.BatchNorm1d(hidden_channels))
        for _ in range(num_layers - 2):
            self.convs.append(GCNConv(hidden_channels, hidden_channels, **kwargs))
            self.bns.append(torch.nn.BatchNorm1d(hidden_channels))
        self.convs.append(GCNConv(hidden_channels, out_channels, **kwargs))
        self.bns.append(torch.nn.BatchNorm1d(hidden_channels))
        self.reset_parameters()

    def forward(self, x, adjs):
        # the reference converts the features to fp32 first (models.py:372); the sum reads fp16 rows directly (exact)
        for i, (adj_t, _e_id, size) in enumerate(adjs):
            x = self.convs[i](x, adj_t, size)
            if i != self.num_layers - 1:
                if self.fused_norm:
                    x = batch_norm_act(x, self.bns[i], act="relu", p=0.5)
                else:
                    x = F.dropout(F.relu(self.bns[i](x)), p=0.5, training=self.training)
        return torch.log_softmax(x, dim=-1)


# --------------------------------------------------------------------------------------------
# SAGEResInception  (driver/models.py:95-192)
# --------------------------------------------------------------------------------------------
class MLP(torch.nn.Module):
    """driver/models.py:95-125: ``num_layers`` Linears (input -> hidden -> ... -> embed), each followed by
    [BatchNorm1d] + activation unless ``end_up_with_fc``, which skips both for EVERY layer (the reference's
    ``continue``): SAGEResInception's MLP is two bare Linears."""

    def __init__(self, input_dim, hidden_dim, embed_dim, num_layers, act="ReLU", bn=False, end_up_with_fc=False,
                 bias=True):
        super().__init__()
        layers = []
        for i in range(num_layers):
            d_in = input_dim if i == 0 else hidden_dim
            d_out = embed_dim if i == num_layers - 1 else hidden_dim
            layers.append(torch.nn.Linear(d_in, d_out, bias=bias))
            if not end_up_with_fc:
                if bn:
                    layers.append(torch.nn.BatchNorm1d(d_out))
                layers.append(getattr(torch.nn, act)(True))
        self.module_list = torch.nn.Sequential(*layers)

    def reset_parameters(self):
        for m in self.module_list:
            if hasattr(m, "reset_parameters"):
                m.reset_parameters()

    def forward(self, x):
        return self.module_list(x)


def _dropout(x, p, training):
    return F.dropout(x, p=p, training=True) if (training and p > 0) else x


class SAGEResInception(_LayerwiseInference, _ConvModel):
    """SAGEConv layers (in -> hidden, then hidden -> hidden: the last one outputs hidden too), each followed by
    BatchNorm1d, leaky_relu and dropout, with a residual (Linear for the first layer, identity after); the input
    and every layer's rows of the final targets are concatenated into a two-Linear MLP head.  ``fused_norm=True`` runs
    each layer's BatchNorm1d, leaky_relu, dropout and residual add as ``batch_norm_act`` (same modules, same state
    dict; the dropouts of the conv's inputs stay torch's)."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, *, dropout=0.1, fused_norm=False):
        super().__init__()
        self.num_layers = num_layers
        self.hidden_channels = hidden_channels
        self.dropout = dropout
        self.fused_norm = fused_norm
        self.convs = torch.nn.ModuleList()
        self.bns = torch.nn.ModuleList()
        self.res_linears = torch.nn.ModuleList()
        for i in range(num_layers):
            d_in = in_channels if i == 0 else hidden_channels
            self.convs.append(SAGEConv(d_in, hidden_channels, bias=False))
            self.bns.append(torch.nn.BatchNorm1d(hidden_channels))
            self.res_linears.append(torch.nn.Linear(in_channels, hidden_channels) if i == 0 else torch.nn.Identity())
        self.mlp = MLP(in_channels + hidden_channels * num_layers, 2 * out_channels, out_channels, num_layers=2, bn=True,
                       end_up_with_fc=True, act="LeakyReLU")
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        for m in self.res_linears:
            if isinstance(m, torch.nn.Linear):
                m.reset_parameters()
        for bn in self.bns:
            bn.reset_parameters()
        self.mlp.reset_parameters()

    def forward(self, x, adjs):
        if isinstance(x, (TableRows, RowRefs)):          # every layer-0 row is dropped out first: nothing to fuse
            x = x.materialize()
        p, tr = self.dropout, self.training
        x = _dropout(x.to(torch.float32), p, tr)
        end_size = adjs[-1][-1][1]
        collect = [x[:end_size]]
        for i, (adj_t, _e_id, size) in enumerate(adjs):
            x_target = x[:size[1]]
            h = self.convs[i]((_dropout(x, p, tr), _dropout(x_target, p, tr)), adj_t)
            # the reference stores the view h[:end_size] and then adds the residual to h IN PLACE, which writes through
            # the view: what is concatenated are the rows after the residual add
            if self.fused_norm:
                x = batch_norm_act(h, self.bns[i], act="leaky_relu", p=p, residual=self.res_linears[i](x_target))
            else:
                h = _dropout(F.leaky_relu(self.bns[i](h)), p, tr)
                x = h + self.res_linears[i](x_target)
            collect.append(x[:end_size])
        return torch.log_softmax(self.mlp(torch.cat(collect, -1)), dim=-1)


_UNSUPPORTED_MODELS = {"sageclassic": "not used in the paper", "jknet": "not used in the paper",
                       "arma": "broken in the reference"}


def get_model_type(model_name):
    """driver/main.py:74-95 for the four models the reference marks as working (names case-insensitive), "gcn" (GCN,
    which the reference leaves unused), "gatv2" (GATv2) and "transformer" (GraphTransformer), which the reference does
    not have"""
    name = model_name.lower()
    models = {"sage": SAGE, "gat": GAT, "gin": GIN, "sageresinception": SAGEResInception, "gcn": GCN, "gatv2": GATv2,
              "transformer": GraphTransformer}
    if name in models:
        return models[name]
    if name in _UNSUPPORTED_MODELS:
        raise NotImplementedError(f"model {model_name!r} is not implemented here ({_UNSUPPORTED_MODELS[name]} per the "
                                  "reference); the working models are SAGE, GAT, GIN and SAGEResInception")
    raise ValueError(f"unknown model {model_name!r}")
