"""Float64 restatement of the GATv2 kernels (csrc/gatv2.hip: k_gatv2_fwd, k_gatv2_bwd; spp.h f3v) with a per-element
first-order rounding bound next to every value, and the inputs the tests run them on.  A helper: no tests in here.
Everything is on the CPU, vectorised, in float64; fp32 / fp16 / bf16 inputs convert to float64 exactly.  The hop, the
entry list (kept CSR entries, then the T self loops) and the constants are tests/gat_f64.py's.

The formulas (x_l [S, H, C], x_r [T, H, C], att [H, C], g [T, H, C]; entry (i, j) of row i, n_i entries):
  forward   pre_ijc = x_l[j,h,c] + x_r[i,h,c],  lr = pre > 0 ? pre : pre * slope,  e_ij = sum_c att[h,c] lr_ijc,
            m_i = max_j e_ij,  w_ij = exp(e_ij - m_i),  s_i = sum_j w_ij,  alpha = w / s,  out[i,h,:] = sum_j alpha_ij x_l[j,h,:]
  backward  go_i = g_i . out_i,  gh_ij = g_i . x_l[j],  ge_ij = alpha_ij (gh_ij - go_i),  d_ijc = pre > 0 ? 1 : slope,
            grad_xl[j,h,c] = sum_i alpha_ij g[i,h,c] + ge_ij att[h,c] d_ijc,   grad_xr[i,h,c] = sum_j ge_ij att[h,c] d_ijc,
            grad_att[h,c] = sum_ij ge_ij lr_ijc
The slope is the fp32 number the kernel receives (gat_f64.SLOPES).

The bounds, built as gat_f64.py builds its own.  u = U = 2^-24; a sum of n fp32 terms, each a rounded product, added in ANY
order is within n u sum|term| of the exact sum to first order; M is the reference expression over absolute values.
  logit:    every term att * lr meets the rounding of pre (fl(a + b) has the exact sign and is 0 only when a + b is, so the
            LeakyReLU branch is the exact one), of the product by the slope, of the product by att, and at most C - 1
            additions: b_e = (C + 2) u sum_c |att lr|.  row_max is the maximum of such numbers: within bm_i = max_j b_e_ij.
  weight:   the online softmax holds w_ij as a product of at most R_i + 1 factors exp(.) whose arguments add up to the
            COMPUTED e_ij - m_i.  R_i counts the rises of the running maximum in the kernel's order (self loop, then CSR);
            a dot product's rounding is not monotone, so a position counts as a rise whenever its exact logit comes within
            2 bm_i of the running maximum of the exact logits: an upper bound on what the kernel can do.
            delta_ij = (R_i + 1) EXP0 + (EXP0 / 8 + u) d_ij + u R_i + b_e_ij + bm_i,   d_ij = m_i - e_ij
            (EXP0 = 1e-6: __expf's relative accuracy at |arg| <= 8, scaled linearly beyond; each rescale one product);
            bw_ij = w_ij delta_ij + (R_i + 2) FLUSH   (FLUSH = 2^-126 per operation that can underflow).
  out:      sum_j |x_l[j]| bw_ij / s_i + M_out (sum_j bw_ij / s_i + (2 n_i + 4) u);      row_sum: sum_j bw_ij + n_i u s_i.
  alpha in the backward (e recomputed, the forward's fp32 row_max and row_sum read):
            dalpha_ij = b_e_ij + bm_i + u d_ij + EXP0 max(1, d_ij / 8) + b_s_i / s_i + 3 u;   b_alpha = alpha dalpha + 2 FLUSH.
  go:       (C + 1) u sum_c |g out| + sum_c |g| b_out;      gh: (C + 1) u sum_c |g x_l|.
  ge:       alpha (b_gh + b_go) + (b_alpha + 3 u alpha)(|gh| + |go|) + FLUSH.
  grad_xr:  sum_j b_ge |att| d + (n_i + 3) u sum_j |ge att d|        (two products per term, a chain of n_i).
  grad_xl:  sum_i (b_alpha |g| + b_ge |att| d) + (cnt_j + 4) u sum_i (alpha |g| + |ge att| d)   (cnt_j entries name j:
            three products and one addition per term, cnt_j atomics in any order).
  grad_att: sum_ij b_ge |lr| + (N + 4) u sum_ij |ge lr|,  N the number of entries (registers, shuffles, LDS, atomics: any order;
            lr carries the roundings of pre and of the slope).
  Second order: G2 = 1 + 2^-10 on every bound built from more than one rounding, as in gat_f64.py.
  Layer level (layer_bounds): the mean over H heads adds (H + 1) u mean|out|, a bias u |out + bias|; a gradient cast back
  to bf16 rows adds 2^-8 |value| (fp16: 2^-11): the format's unit roundoff (8 and 11 significand bits).
None of these constants comes from GPU output."""
import types

import torch

from gat_f64 import COUNTS, EXP0, FLUSH, G2, SLOPES, U, Hop, planted_hop, regime as _gat_regime, worst  # noqa: F401

F64 = torch.float64
REGIMES = ["model", "equal", "ascending", "descending", "selfmax", "selfmin", "wide", "zero"]


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def inputs(name, hop, H, C, dtype, seed=0):
    """(x_l [S, H, C] and x_r [T, H, C] in dtype, att [H, C] and g [T, H, C] in fp32) for a logit regime.
    "model": random rows and att.  The planted ones put gat_f64.regime's a_src / a_dst (multiples of 2^-10 below 128) into
    the EVEN columns of x_l / x_r with att = 2 / C there and 0 in the odd columns, whose rows are random: every even
    column carries the same pre-activation, so e_ij = lrelu(a_src[j] + a_dst[i]) up to rounding that is the same for equal
    inputs ("equal": equal bits), and the messages still differ per column.  "zero": small integers / 2 in every column, so
    pre is exactly 0, positive and negative within every head; att random."""
    S, T = hop.S, hop.T
    gen = torch.Generator().manual_seed(seed + 1000 * C + H)
    x_l = 0.5 * torch.randn((S, H, C), generator=gen)
    x_r = 0.5 * torch.randn((T, H, C), generator=gen)
    att = torch.randn((H, C), generator=gen) / C ** 0.5
    g = torch.randn((T, H, C), generator=gen)
    if name == "zero":
        s, t = torch.arange(S).view(S, 1, 1), torch.arange(T).view(T, 1, 1)
        h, c = torch.arange(H).view(1, H, 1), torch.arange(C).view(1, 1, C)
        x_l = (((s + c + h) % 3) - 1).float() * 0.5
        x_r = (((t + 2 * c + h) % 3) - 1).float() * 0.5
    elif name != "model":
        a_src, a_dst = _gat_regime(name, hop, H)
        x_l[:, :, 0::2] = a_src.unsqueeze(2)
        x_r[:, :, 0::2] = a_dst.unsqueeze(2)
        att = torch.zeros((H, C))
        att[:, 0::2] = 2.0 / C
    return x_l.to(dtype), x_r.to(dtype), att, g


def _rows(n, idx, v):
    return torch.zeros((n,) + tuple(v.shape[1:]), dtype=F64).index_add_(0, idx, v)


def forward(hop, x_l, x_r, att, slope):
    x_l, x_r, att = x_l.double(), x_r.double(), att.double()
    T, (H, C), r, s = hop.T, att.shape, hop.r, hop.s
    pre = x_l[s] + x_r[r]                                                   # [N, H, C]
    lr = lrelu(pre, slope)
    e = (att * lr).sum(2)
    b_e = G2 * (C + 2) * U * (att.abs() * lr.abs()).sum(2)
    idx = r.unsqueeze(1).expand(-1, H)
    m = torch.full((T, H), -float("inf"), dtype=F64).scatter_reduce(0, idx, e, "amax")
    bm = torch.zeros((T, H), dtype=F64).scatter_reduce(0, idx, b_e, "amax")
    d = m[r] - e
    w = torch.exp(-d)
    ssum = _rows(T, r, w)
    alpha = w / ssum[r]
    ep = torch.cat([e, torch.full((1, H), -float("inf"), dtype=F64)])[hop.seq]       # [T, L, H]
    on = (hop.seq[:, 1:] >= 0).unsqueeze(2)
    R = (on & (ep[:, 1:] > torch.cummax(ep, 1).values[:, :-1] - 2 * bm.unsqueeze(1))).sum(1).double()
    n = hop.n.double().unsqueeze(1)
    delta = (R[r] + 1) * EXP0 + (EXP0 / 8 + U) * d + U * R[r] + b_e + bm[r]
    bw = w * delta + (R[r] + 2) * FLUSH
    a3, b3 = alpha.unsqueeze(2), (bw / ssum[r]).unsqueeze(2)
    out = _rows(T, r, a3 * x_l[s])
    M = _rows(T, r, a3 * x_l[s].abs())
    rel = _rows(T, r, bw / ssum[r]) + (2 * n + 4) * U
    b_out = G2 * (_rows(T, r, b3 * x_l[s].abs()) + M * rel.unsqueeze(2))
    bs = G2 * (_rows(T, r, bw) + n * U * ssum)
    return types.SimpleNamespace(out=out, b_out=b_out, row_max=m, bm=bm, row_sum=ssum, bs=bs, alpha=alpha, e=e, b_e=b_e,
                                 d=d, R=R, pre=pre, lr=lr)


def backward(hop, x_l, x_r, att, g, slope, fw=None):
    """closed-form gradients of sum(out * g) and their bounds"""
    fw = fw or forward(hop, x_l, x_r, att, slope)
    x_l, att, g = x_l.double(), att.double(), g.double()
    T, S, (H, C), r, s = hop.T, hop.S, att.shape, hop.r, hop.s
    ga, alpha = g.abs(), fw.alpha
    go = (g * fw.out).sum(2)
    b_go = (C + 1) * U * (ga * fw.out.abs()).sum(2) + (ga * fw.b_out).sum(2)
    gh = (g[r] * x_l[s]).sum(2)
    b_gh = (C + 1) * U * (ga[r] * x_l[s].abs()).sum(2)
    d_alpha = (fw.b_e + fw.bm[r] + U * fw.d + EXP0 * torch.clamp(fw.d / 8, min=1.0) + fw.bs[r] / fw.row_sum[r] + 3 * U)
    b_alpha = G2 * alpha * d_alpha + 2 * FLUSH
    ge = alpha * (gh - go[r])
    b_ge = G2 * (alpha * (b_gh + b_go[r]) + (b_alpha + 3 * U * alpha) * (gh.abs() + go[r].abs())) + FLUSH
    dl = torch.where(fw.pre > 0, 1.0, slope).double()                       # [N, H, C]
    t_r = ge.unsqueeze(2) * att * dl                                        # ge att d
    bt_r = b_ge.unsqueeze(2) * att.abs() * dl
    n = hop.n.double().view(T, 1, 1)
    named = hop.named.double().view(S, 1, 1)
    out = types.SimpleNamespace(fw=fw, ge=ge, b_ge=b_ge, b_alpha=b_alpha)
    out.gxr = _rows(T, r, t_r)
    out.b_gxr = G2 * (_rows(T, r, bt_r) + (n + 3) * U * _rows(T, r, t_r.abs()))
    a3 = alpha.unsqueeze(2)
    out.gxl = _rows(S, s, a3 * g[r] + t_r)
    out.b_gxl = G2 * (_rows(S, s, b_alpha.unsqueeze(2) * ga[r] + bt_r)
                      + (named + 4) * U * _rows(S, s, a3 * ga[r] + t_r.abs()))
    t_a = ge.unsqueeze(2) * fw.lr
    N = float(r.numel())
    out.gatt = t_a.sum(0)
    out.b_gatt = G2 * ((b_ge.unsqueeze(2) * fw.lr.abs()).sum(0) + (N + 4) * U * t_a.abs().sum(0))
    return out


def layer_bounds(bw, concat, bias, rows_dtype):
    """the layer's output and the rows' gradients as GATv2Conv returns them, from backward()'s kernel-level values:
    (out, b_out, cast) -- out [T, H * C] or the mean over heads [T, C], plus bias; cast: the relative half ulp a
    gradient cast back to the rows' dtype adds (0 for fp32 rows)"""
    fw = bw.fw
    T, H, C = fw.out.shape
    if concat:
        out, b = fw.out.reshape(T, H * C), fw.b_out.reshape(T, H * C)
    else:
        out, b = fw.out.mean(1), fw.b_out.mean(1) + (H + 1) * U * fw.out.abs().mean(1)
    if bias is not None:
        out = out + bias.double()
        b = b + U * out.abs()
    cast = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[rows_dtype]
    return out, G2 * b, cast


def sampled_batch(num_nodes=400, seeds=8, fanouts=(6, 5, 4), feat=16, classes=5, seed=0):
    """a three-hop neighbour-sampled batch of a small synthetic graph, as the data path delivers it: x [S0, feat] fp32,
    y [seeds], and [(rowptr, col, T, S)] outermost hop first (the targets of a hop are its first T sources)"""
    gen = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 12, (num_nodes,), generator=gen)
    nbrs = [torch.randint(0, num_nodes, (int(d),), generator=gen).tolist() for d in deg]
    n_id = torch.randperm(num_nodes, generator=gen)[:seeds].tolist()
    hops = []
    for k in reversed(fanouts):                            # innermost hop first
        T, pos = len(n_id), {v: i for i, v in enumerate(n_id)}
        rowptr, col = [0], []
        for t in range(T):
            cand = nbrs[n_id[t]]
            pick = [cand[i] for i in torch.randperm(len(cand), generator=gen)[:k].tolist()]
            for v in pick:
                if v not in pos:
                    pos[v] = len(n_id)
                    n_id.append(v)
                col.append(pos[v])
            rowptr.append(len(col))
        hops.append((torch.tensor(rowptr, dtype=torch.int64), torch.tensor(col, dtype=torch.int64), T, len(n_id)))
    x = torch.randn((num_nodes, feat), generator=gen)[torch.tensor(n_id)]
    y = torch.randint(0, classes, (seeds,), generator=gen)
    return x, y, hops[::-1]
