"""Float64 restatement of the GATv2 kernels WITH attention dropout (csrc/gatv2.hip: k_gatv2_fwd / k_gatv2_bwd with kDrop;
spp.h f3x) and a per-element first-order rounding bound next to every value.  A helper: no tests in here.  The hop, the
entry list, the logits, the softmax and every constant are tests/gatv2_f64.py's; the mask is the numpy restatement
models._attn_keep_reference(E, T, H, p, seed), mapped from [(E + T), H] to the entry list (kept CSR entries by their CSR
position hop.eid, then the T self loops at E + t).

The formulas (q_ij = keep_ij * scale, scale = 1 / (1 - p) with p the C float the entries receive):
  forward   alpha as gatv2_f64 (over ALL entries),  out'[i,h,:] = sum_j q_ij alpha_ij x_l[j,h,:]
  backward  go'_i = g_i . out'_i,  gh_ij = g_i . x_l[j],  ge_ij = alpha_ij (q_ij gh_ij - go'_i),
            grad_xl[j,h,c] = sum_i q_ij alpha_ij g[i,h,c] + ge_ij att[h,c] d_ijc,   grad_xr, grad_att from ge as gatv2_f64.

The bounds are NOT gatv2_f64's times scale (its b_go uses |out|, and a dropped out' can be large where the full one
cancels): each is rebuilt by gatv2_f64's own rule on the dropped quantity.
  row_max, row_sum and their bounds: gatv2_f64.forward's own -- the kernel's softmax state takes every entry.
  weight:   bw_ij = w_ij delta_ij + (R_i + 2) FLUSH, gatv2_f64's, recomputed here from the fields forward() returns.
  out':     M' = sum_j q alpha |x_l|.  The kernel's accumulator holds the KEPT entries' w x_l; the denominator s holds all
            of them; the result is acc * fl(scale32 / s), scale32 = fl32(scale):
            sum_j q |x_l| bw_ij / s_i + M' (sum_j bw_ij / s_i + (2 n_i + 4) u + 2 u)
            (gatv2_f64's rel -- the division stands where its reciprocal stood -- plus one u for scale32 against the
            float64 scale and one for the multiplication by it).
  go':      (C + 1) u sum_c |g out'| + sum_c |g| b_out'.      gh: gatv2_f64's.
  q gh:     q b_gh + 2 u |q gh|   (scale32, and the product).
  ge:       alpha (b_qgh + b_go') + (b_alpha + 3 u alpha)(|q gh| + |go'|) + FLUSH     (b_alpha: gatv2_f64's).
  grad_xr, grad_att: gatv2_f64's rules on this ge and b_ge.
  grad_xl:  the message weight is fl(alpha * q): b_qa = q b_alpha + 2 u q alpha (scale32, and the product);
            sum_i (b_qa |g| + b_ge |att| d) + (cnt_j + 4) u sum_i (q alpha |g| + |ge att| d).
  Second order: G2 on every bound built from more than one rounding.
None of these constants comes from GPU output."""
import types

import numpy as np
import torch

import gatv2_f64 as G
from gatv2_f64 import EXP0, FLUSH, G2, U, _rows

F64 = torch.float64


def scale_of(p):
    """1 / (1 - p) with p the C float the entries receive, in float64"""
    return 1.0 / (1.0 - float(np.float32(p)))


def entry_keep(hop, keep):
    """keep [(E + T), H] (models._attn_keep_reference, or the bytes spp_gat_mh_attn_keep wrote) per softmax entry of the
    Hop: the kept CSR entries by their CSR position, then the self loops.  -> [N, H] float64 of 0 / 1"""
    keep = torch.as_tensor(np.asarray(keep)).reshape(hop.E + hop.T, -1)
    return keep[torch.cat([hop.eid, hop.E + torch.arange(hop.T)])].to(F64)


def mask(hop, H, p, seed):
    """([(E + T), H] uint8, [N, H] float64) for the hop from the numpy restatement of the keep rule"""
    from salient_plusplus_amd.models import _attn_keep_reference
    keep = _attn_keep_reference(hop.E, hop.T, H, p, seed)
    return keep, entry_keep(hop, keep)


def forward_drop(hop, x_l, x_r, att, slope, keep, p, fw=None):
    """keep [N, H]: the mask per softmax entry (entry_keep)"""
    fw = fw or G.forward(hop, x_l, x_r, att, slope)
    x_l = x_l.double()
    T, r, s = hop.T, hop.r, hop.s
    q = keep.double() * scale_of(p)
    w = torch.exp(-fw.d)
    delta = (fw.R[r] + 1) * EXP0 + (EXP0 / 8 + U) * fw.d + U * fw.R[r] + fw.b_e + fw.bm[r]
    bw = w * delta + (fw.R[r] + 2) * FLUSH
    ssum = fw.row_sum
    n = hop.n.double().unsqueeze(1)
    qa = (q * fw.alpha).unsqueeze(2)
    out = _rows(T, r, qa * x_l[s])
    M = _rows(T, r, qa * x_l[s].abs())
    rel = _rows(T, r, bw / ssum[r]) + (2 * n + 4) * U + 2 * U
    b_out = G2 * (_rows(T, r, (q * bw / ssum[r]).unsqueeze(2) * x_l[s].abs()) + M * rel.unsqueeze(2))
    return types.SimpleNamespace(out=out, b_out=b_out, row_max=fw.row_max, bm=fw.bm, row_sum=ssum, bs=fw.bs,
                                 alpha=fw.alpha, q=q, full=fw, M=M)


def backward_drop(hop, x_l, x_r, att, g, slope, keep, p, fw=None, keep_bwd=None):
    """closed-form gradients of sum(out' * g) and their bounds.  keep_bwd: another mask for the backward alone (a planted
    fault of the host test; the saved out' stays the forward's)"""
    fd = forward_drop(hop, x_l, x_r, att, slope, keep, p, fw)
    full = fd.full
    x_l, att, g = x_l.double(), att.double(), g.double()
    T, S, (H, C), r, s = hop.T, hop.S, att.shape, hop.r, hop.s
    ga, alpha = g.abs(), full.alpha
    q = fd.q if keep_bwd is None else keep_bwd.double() * scale_of(p)
    go = (g * fd.out).sum(2)
    b_go = (C + 1) * U * (ga * fd.out.abs()).sum(2) + (ga * fd.b_out).sum(2)
    gh = (g[r] * x_l[s]).sum(2)
    b_gh = (C + 1) * U * (ga[r] * x_l[s].abs()).sum(2)
    qgh = q * gh
    b_qgh = q * b_gh + 2 * U * qgh.abs()
    d_alpha = (full.b_e + full.bm[r] + U * full.d + EXP0 * torch.clamp(full.d / 8, min=1.0)
               + full.bs[r] / full.row_sum[r] + 3 * U)
    b_alpha = G2 * alpha * d_alpha + 2 * FLUSH
    ge = alpha * (qgh - go[r])
    b_ge = G2 * (alpha * (b_qgh + b_go[r]) + (b_alpha + 3 * U * alpha) * (qgh.abs() + go[r].abs())) + FLUSH
    dl = torch.where(full.pre > 0, 1.0, slope).double()
    t_r = ge.unsqueeze(2) * att * dl
    bt_r = b_ge.unsqueeze(2) * att.abs() * dl
    n = hop.n.double().view(T, 1, 1)
    named = hop.named.double().view(S, 1, 1)
    out = types.SimpleNamespace(fw=fd, ge=ge, b_ge=b_ge, b_alpha=b_alpha)
    out.gxr = _rows(T, r, t_r)
    out.b_gxr = G2 * (_rows(T, r, bt_r) + (n + 3) * U * _rows(T, r, t_r.abs()))
    qa = (q * alpha).unsqueeze(2)
    b_qa = (q * b_alpha + 2 * U * q * alpha).unsqueeze(2)
    out.gxl = _rows(S, s, qa * g[r] + t_r)
    out.b_gxl = G2 * (_rows(S, s, b_qa * ga[r] + bt_r) + (named + 4) * U * _rows(S, s, qa * ga[r] + t_r.abs()))
    t_a = ge.unsqueeze(2) * full.lr
    N = float(r.numel())
    out.gatt = t_a.sum(0)
    out.b_gatt = G2 * ((b_ge.unsqueeze(2) * full.lr.abs()).sum(0) + (N + 4) * U * t_a.abs().sum(0))
    return out
