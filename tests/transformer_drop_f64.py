"""Float64 restatement of the TransformerConv kernels WITH attention dropout (csrc/transformer_conv.hip: k_transformer_fwd
/ k_transformer_bwd with kDrop; spp.h f4a) and a per-element first-order rounding bound next to every value.  A helper:
no tests in here.  The entry list (Entries), the regimes, scale32, the logits, the softmax and every constant are
tests/transformer_f64.py's; the mask is the numpy restatement models._attn_keep_reference(E, 0, H, p, seed) -- no
self-loop draws -- and CSR entry k of the entry list is row k of it.

The formulas (d_ij = keep_ij * ds, ds = 1 / (1 - p) with p the C float the entries receive):
  forward   alpha as transformer_f64 (over ALL entries),  out'[i,h,:] = sum_j d_ij alpha_ij v[j,h,:]
            n_i = 0: out' = 0; every entry of (i, h) dropped: out'[i,h,:] = 0
  backward  go'_i = g_i . out'_i,  gh_ij = g_i . v[j],  ge_ij = alpha_ij (d_ij gh_ij - go'_i),  ges = ge scale,
            grad_q[i,h,c] = sum_j ges_ij k[j,h,c],  grad_k[j,h,c] = sum_i ges_ij q[i,h,c],
            grad_v[j,h,c] = sum_i d_ij alpha_ij g[i,h,c]

The bounds are NOT transformer_f64's times ds (its b_go uses |out|, and a dropped out' can be large where the full one
cancels): each is rebuilt by transformer_f64's own rule on the dropped quantity, as tests/gatv2_drop_f64.py does.
  row_max, row_sum and their bounds: transformer_f64.forward's own -- the kernel's softmax state takes every entry.
  weight:   bw_ij = w_ij delta_ij + (R_i + 2) FLUSH, transformer_f64's, recomputed here from the fields forward() returns.
  out':     M' = sum_j d alpha |v|.  The kernel's accumulator holds the KEPT entries' w v; the denominator s holds all of
            them; the result is acc * fl(ds32 / s), ds32 = fl32(ds):
            sum_j d |v| bw_ij / s_i + M' (sum_j bw_ij / s_i + (2 n_i + 4) u + 2 u)
            (transformer_f64's rel -- the division stands where its reciprocal stood -- plus one u for ds32 against the
            float64 ds and one for the multiplication by it).  Zero for a row without entries and for a (target, head)
            with every entry dropped: M' = 0 and no kept |v|.
  go':      (C + 1) u sum_c |g out'| + sum_c |g| b_out'.      gh: transformer_f64's gv bound.
  d gh:     d b_gh + 2 u |d gh|   (ds32, and the product).
  ges:      scale (alpha (b_dgh + b_go') + (b_alpha + 4 u alpha)(|d gh| + |go'|)) + FLUSH     (b_alpha: transformer_f64's).
  grad_q, grad_k: transformer_f64's rules on this ges and b_ges.
  grad_v:   the message weight is fl(alpha * d): b_da = d b_alpha + 2 u d alpha (ds32, and the product);
            sum_i b_da |g| + (cnt_j + 2) u sum_i d alpha |g|.
  Second order: G2 on every bound built from more than one rounding.
None of these constants comes from GPU output."""
import types

import numpy as np
import torch

import transformer_f64 as X
from transformer_f64 import EXP0, FLUSH, G2, U, _rows

F64 = torch.float64


def scale_of(p):
    """1 / (1 - p) with p the C float the entries receive, in float64"""
    return 1.0 / (1.0 - float(np.float32(p)))


def entry_keep(ent, keep, H):
    """the first E * H bytes of a mask (models._attn_keep_reference(E, 0, H, ...), or what spp_gat_mh_attn_keep wrote)
    per entry of the Entries, by CSR position -> [E, H] float64 of 0 / 1"""
    keep = torch.as_tensor(np.asarray(keep).reshape(-1)[:ent.E * H].copy()).reshape(ent.E, H)
    return keep.to(F64)


def mask(ent, H, p, seed):
    """([E, H] uint8, [E, H] float64) for the entry list from the numpy restatement of the keep rule"""
    from salient_plusplus_amd.models import _attn_keep_reference
    keep = _attn_keep_reference(ent.E, 0, H, p, seed)
    return keep, entry_keep(ent, keep, H)


def all_dropped(ent, keep):
    """[T, H] bool: (target, head) pairs that have entries and lose every one of them"""
    kept = _rows(ent.T, ent.row, keep.double())
    return (ent.n.unsqueeze(1) > 0) & (kept == 0)


def forward_drop(ent, q, k, v, scale, keep, p, fw=None):
    """keep [E, H]: the mask per entry (entry_keep)"""
    fw = fw or X.forward(ent, q, k, v, scale)
    v = v.double()
    T, r, s = ent.T, ent.row, ent.col
    d = keep.double() * scale_of(p)
    w = torch.exp(-fw.d)
    delta = (fw.R[r] + 1) * EXP0 + (EXP0 / 8 + U) * fw.d + U * fw.R[r] + fw.b_e + fw.bm[r]
    bw = w * delta + (fw.R[r] + 2) * FLUSH
    ssum = fw.row_sum
    n = ent.n.double().unsqueeze(1)
    da = (d * fw.alpha).unsqueeze(2)
    out = _rows(T, r, da * v[s])
    M = _rows(T, r, da * v[s].abs())
    has = (n > 0).double()
    rel = _rows(T, r, bw / ssum[r]) + ((2 * n + 4) * U + 2 * U) * has
    b_out = G2 * (_rows(T, r, (d * bw / ssum[r]).unsqueeze(2) * v[s].abs()) + M * rel.unsqueeze(2))
    return types.SimpleNamespace(out=out, b_out=b_out, row_max=fw.row_max, bm=fw.bm, row_sum=ssum, bs=fw.bs,
                                 alpha=fw.alpha, dq=d, full=fw, M=M)


def backward_drop(ent, q, k, v, g, scale, keep, p, fw=None, keep_bwd=None):
    """closed-form gradients of sum(out' * g) and their bounds.  keep_bwd: another mask for the backward alone (a planted
    fault of the host test; the saved out' stays the forward's)"""
    fd = forward_drop(ent, q, k, v, scale, keep, p, fw)
    full = fd.full
    q, k, v, g = q.double(), k.double(), v.double(), g.double()
    (T, H, C), S = q.shape, k.size(0)
    r, s = ent.row, ent.col
    ga, alpha = g.abs(), full.alpha
    d = fd.dq if keep_bwd is None else keep_bwd.double() * scale_of(p)
    go = (g * fd.out).sum(2)
    b_go = (C + 1) * U * (ga * fd.out.abs()).sum(2) + (ga * fd.b_out).sum(2)
    gh = (g[r] * v[s]).sum(2)
    b_gh = (C + 1) * U * (ga[r] * v[s].abs()).sum(2)
    dgh = d * gh
    b_dgh = d * b_gh + 2 * U * dgh.abs()
    d_alpha = (full.b_e + full.bm[r] + U * full.d + EXP0 * torch.clamp(full.d / 8, min=1.0)
               + full.bs[r] / full.row_sum[r] + 3 * U)
    b_alpha = G2 * alpha * d_alpha + 2 * FLUSH
    ges = alpha * (dgh - go[r]) * scale
    b_ges = G2 * scale * (alpha * (b_dgh + b_go[r]) + (b_alpha + 4 * U * alpha) * (dgh.abs() + go[r].abs())) + FLUSH
    n = ent.n.double().view(T, 1, 1)
    named = ent.named.double().view(S, 1, 1)
    g3, b3 = ges.unsqueeze(2), b_ges.unsqueeze(2)
    da = (d * alpha).unsqueeze(2)
    b_da = (d * b_alpha + 2 * U * d * alpha).unsqueeze(2)
    out = types.SimpleNamespace(fw=fd, ges=ges, b_ges=b_ges, b_alpha=b_alpha)
    out.gq = _rows(T, r, g3 * k[s])
    out.b_gq = G2 * (_rows(T, r, b3 * k[s].abs()) + (n + 2) * U * _rows(T, r, (g3 * k[s]).abs()))
    out.gk = _rows(S, s, g3 * q[r])
    out.b_gk = G2 * (_rows(S, s, b3 * q[r].abs()) + (named + 2) * U * _rows(S, s, (g3 * q[r]).abs()))
    out.gv = _rows(S, s, da * g[r])
    out.b_gv = G2 * (_rows(S, s, b_da * ga[r]) + (named + 2) * U * _rows(S, s, da * ga[r]))
    return out
