"""GPU: the aggregation kernels' bf16 forms (spp_agg_forward / spp_agg_backward, the GAT kernels' element code) against
their fp32 forms.  The rule under test (include/spp.h): loads convert exactly, every sum runs in fp32 in the fp32
kernels' order, and each stored bf16 element is rounded once, to nearest even -- so a bf16 output is the fp32 output
.to(torch.bfloat16) bit for bit, and a bf16 input gives the fp32 kernel's result on x.float() bit for bit.

The backward checks use gradients that are small multiples of 1/16 over hops whose degrees are powers of two: every
product and partial sum is then exact in fp32, so the gather's and the atomics' summation orders cannot change a bit and
the comparisons can be exact too."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


@pytest.fixture(autouse=True)
def _entries_exist():
    """first: the descriptor entries exist (nothing below launches a kernel otherwise)"""
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    assert hasattr(L, "spp_agg_forward") and hasattr(L, "spp_agg_backward"), "spp_agg_forward is not exported"


def _nat():
    from salient_plusplus_amd import _native as nat
    return nat, nat.load()


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hop(T, S, maxdeg, seed, pow2=False):
    g = torch.Generator().manual_seed(seed)
    if pow2:
        deg = torch.tensor([0, 1, 2, 4, 8])[torch.randint(0, 5, (T,), generator=g)]
    else:
        deg = torch.randint(0, maxdeg + 1, (T,), generator=g)
        deg[::7] = 0
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, S, (int(rowptr[-1]),), generator=g)
    col[:T // 3] = torch.arange(T // 3) % S                  # self edges among them
    return rowptr.cuda(), col.cuda()


def _exact(shape, seed, dtype=F32):
    """multiples of 1/16 in [-4, 4]: exact in bf16, products with 1/deg (deg a power of two) and short sums exact in fp32"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-64, 65, shape, generator=g).float() / 16).to(dtype).cuda()


def _fwd(source, epilogue, rowptr, col, T, F, x, out_dtype, *, table=None, n_id=None, scale=1.0, act=(0.0, 0, 0)):
    """spp_agg_forward into a fresh [T, F or 2F] tensor; x: the dense matrix, or the table (TABLE / ROWS)"""
    nat, L = _nat()
    width = 2 * F if epilogue in (nat.SPP_AGG_OPERAND, nat.SPP_AGG_OPERAND_ACT) else F
    out = torch.full((T, width), float("nan"), dtype=out_dtype, device="cuda")
    rows = table if table is not None else x
    if source == nat.SPP_AGG_ROWS:
        ids = (rows.data_ptr() + n_id * rows.stride(0) * rows.element_size()).contiguous()
    else:
        ids = n_id
    d = nat.AggFwdDesc(source=source, epilogue=epilogue, x_elem={F32: 0, F16: 1, BF16: 2}[rows.dtype],
                       out_elem={F32: 0, BF16: 2}[out_dtype], rowptr_dev=rowptr.data_ptr(),
                       col_dev=col.data_ptr() if col.numel() else None, num_targets=T,
                       x_dev=rows.data_ptr() if source != nat.SPP_AGG_ROWS else None, x_stride_elems=rows.stride(0),
                       x_rows=rows.size(0) if source == nat.SPP_AGG_TABLE else 0,
                       n_id_dev=ids.data_ptr() if ids is not None else None, F=F, out_dev=out.data_ptr(),
                       out_stride_elems=0, self_scale=scale, p=act[0], training=act[1], seed=act[2])
    nat.check(L.spp_agg_forward(C.byref(d), _st()))
    torch.cuda.synchronize()
    return out


def _bwd(form, epilogue, rowptr, col, T, S, g, F, out_dtype, *, z=None, scale=1.0, act=(0.0, 0, 0)):
    nat, L = _nat()
    gx = torch.full((S, F), float("nan"), dtype=out_dtype, device="cuda")
    E = col.numel()
    if form == nat.SPP_AGG_GATHER:
        nbytes = int(L.spp_sage_operand_backward_workspace_bytes(T, S, E))
    else:
        nbytes = 4 * S * F if out_dtype != F32 else 0
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    d = nat.AggBwdDesc(form=form, epilogue=epilogue, grad_elem={F32: 0, BF16: 2}[g.dtype],
                       out_elem={F32: 0, BF16: 2}[out_dtype], z_elem={F32: 0, BF16: 2}[z.dtype] if z is not None else 0,
                       rowptr_dev=rowptr.data_ptr(), col_dev=col.data_ptr(), num_targets=T, num_sources=S, num_edges=E,
                       grad_out_dev=g.data_ptr(), grad_out_stride_elems=g.stride(0), F=F, grad_x_dev=gx.data_ptr(),
                       z_dev=z.data_ptr() if z is not None else None, self_scale=scale, p=act[0], training=act[1],
                       seed=act[2])
    nat.check(L.spp_agg_backward(C.byref(d), C.c_void_p(ws.data_ptr()), nbytes, _st()))
    torch.cuda.synchronize()
    return gx


SOURCES = ["dense", "table", "rows"]


@pytest.mark.parametrize("F", [128, 47])
@pytest.mark.parametrize("tin", [F32, F16, BF16])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("epi", ["mean", "operand", "sum"])
def test_forward_bf16_output_is_the_fp32_output_rounded(epi, source, tin, F):
    from test_gpu_gin_sage_ri import _seq_sum
    from test_gpu_model_step import _seq_mean
    nat, _L = _nat()
    T, S, R = 1500, 4000, 6000
    rowptr, col = _hop(T, S, 13, F)
    table = torch.randn((R, F), generator=torch.Generator().manual_seed(F + 1)).to(tin).cuda()
    n_id = torch.randint(0, R, (S,), generator=torch.Generator().manual_seed(2)).cuda()
    x = table[n_id].contiguous()                               # the batch's rows as a dense matrix
    code = {"mean": nat.SPP_AGG_MEAN, "operand": nat.SPP_AGG_OPERAND, "sum": nat.SPP_AGG_SUM}[epi]
    src = {"dense": nat.SPP_AGG_DENSE, "table": nat.SPP_AGG_TABLE, "rows": nat.SPP_AGG_ROWS}[source]
    kw = dict(table=table, n_id=n_id) if source != "dense" else {}
    got32 = _fwd(src, code, rowptr, col, T, F, x, F32, **kw)
    got16 = _fwd(src, code, rowptr, col, T, F, x, BF16, **kw)
    # the fp32 output is the sequential fp32 restatement of the fp32 kernel, bit for bit
    if epi == "sum":
        want = _seq_sum(x, rowptr, col, T, 1.0)
    else:
        want = _seq_mean(x, rowptr, col, T)
        if epi == "operand":
            want = torch.cat([want, x[:T].float()], dim=1)
    assert torch.equal(got32, want)
    assert got16.dtype == BF16 and torch.equal(got16, got32.to(BF16))
    if tin == BF16:                                            # bf16 rows: the fp32 kernel on x.float(), bit for bit
        kw32 = dict(table=table.float(), n_id=n_id) if source != "dense" else {}
        assert torch.equal(got32, _fwd(src, code, rowptr, col, T, F, x.float(), F32, **kw32))


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("tin", [F32, BF16])
def test_activation_on_load_from_bf16_keeps_the_fp32_mask(tin, training):
    """OPERAND_ACT on a bf16 pre-activation: the fp32 kernel on z.float() (spp_sage_operand_forward_act), bit for bit,
    so the dropout decisions at one seed are those of the fp32 path; the bf16 output is that rounded"""
    nat, L = _nat()
    T, S, F, p, seed = 1700, 6100, 256, 0.5, 0x1234567890ABCDEF >> 1
    rowptr, col = _hop(T, S, 11, 99)
    z = torch.randn((S, F), generator=torch.Generator().manual_seed(3)).to(tin).cuda()
    ref = torch.empty((T, 2 * F), device="cuda")
    zf = z.float().contiguous()
    nat.check(L.spp_sage_operand_forward_act(_P(rowptr), _P(col), T, _P(zf), F, _P(ref), 2 * F, p, training, seed, _st()))
    torch.cuda.synchronize()
    act = (p, training, seed)
    got32 = _fwd(nat.SPP_AGG_DENSE, nat.SPP_AGG_OPERAND_ACT, rowptr, col, T, F, z, F32, act=act)
    got16 = _fwd(nat.SPP_AGG_DENSE, nat.SPP_AGG_OPERAND_ACT, rowptr, col, T, F, z, BF16, act=act)
    assert torch.equal(got32, ref)
    assert torch.equal(got16, ref.to(BF16))
    if training:
        assert 0.3 < float((ref[:, F:] == 0).float().mean()) < 0.9        # relu and dropout both acted


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("gout", [F32, BF16])
@pytest.mark.parametrize("gin", [F32, BF16])
@pytest.mark.parametrize("epi", ["operand", "operand_act", "sum"])
def test_gather_backward_equals_the_fp32_gather_rounded(epi, gin, gout):
    nat, L = _nat()
    T, S, F, p, seed = 2100, 5200, 128, 0.5, 77
    rowptr, col = _hop(T, S, 0, 5, pow2=True)
    E = col.numel()
    width = 2 * F if epi != "sum" else F
    g = _exact((T, width), 11, gin)
    gf = g.float().contiguous()
    ref = torch.empty((S, F), device="cuda")
    nbytes = int(L.spp_sage_operand_backward_workspace_bytes(T, S, E))
    ws = _ws(nbytes)
    zs = [None]
    if epi == "operand":
        nat.check(L.spp_sage_operand_backward_gather(_P(rowptr), _P(col), T, S, E, _P(gf), width, F, _P(ref), _P(ws),
                                                     nbytes, _st()))
    elif epi == "sum":
        nat.check(L.spp_csr_sum_backward_gather(_P(rowptr), _P(col), T, S, E, _P(gf), width, F, 2.0, _P(ref), _P(ws),
                                                nbytes, _st()))
    else:
        zs = [torch.randn((S, F), generator=torch.Generator().manual_seed(4)).to(zd).cuda() for zd in (F32, BF16)]
    torch.cuda.synchronize()
    code = {"operand": nat.SPP_AGG_OPERAND, "operand_act": nat.SPP_AGG_OPERAND_ACT, "sum": nat.SPP_AGG_SUM}[epi]
    for z in zs:
        if z is not None:                                      # the fp32 entry on z.float()
            zf = z.float().contiguous()
            nat.check(L.spp_sage_operand_backward_gather_act(_P(rowptr), _P(col), T, S, E, _P(gf), width, F, _P(ref),
                                                             _P(ws), nbytes, _P(zf), p, 1, seed, _st()))
            torch.cuda.synchronize()
        got = _bwd(nat.SPP_AGG_GATHER, code, rowptr, col, T, S, g, F, gout, z=z, scale=2.0, act=(p, 1, seed))
        assert got.dtype == gout and torch.equal(got, ref.to(gout))


@pytest.mark.parametrize("gout", [F32, BF16])
@pytest.mark.parametrize("gin", [F32, BF16])
@pytest.mark.parametrize("epi,F", [("mean", 128), ("mean", 47), ("operand", 128), ("operand_act", 128), ("sum", 128),
                                   ("sum", 47)])
def test_scatter_backward_matches_the_fp32_scatter(epi, F, gin, gout):
    """fp32 atomics into an fp32 buffer, one rounding pass after: exact inputs give the fp32 entries' result rounded,
    bit for bit; random inputs agree within the existing backward tolerance"""
    nat, L = _nat()
    T, S, p, seed = 1900, 4700, 0.5, 5
    rowptr, col = _hop(T, S, 0, 8, pow2=True)
    width = 2 * F if epi.startswith("operand") else F
    code = {"mean": nat.SPP_AGG_MEAN, "operand": nat.SPP_AGG_OPERAND, "operand_act": nat.SPP_AGG_OPERAND_ACT,
            "sum": nat.SPP_AGG_SUM}[epi]
    z = torch.randn((S, F), generator=torch.Generator().manual_seed(6)).to(gin).cuda() if epi == "operand_act" else None
    for g in (_exact((T, width), 12, gin), torch.randn((T, width), generator=torch.Generator().manual_seed(7)).to(gin).cuda()):
        gf = g.float().contiguous()
        ref = torch.zeros((S, F), device="cuda")
        if epi == "mean":
            nat.check(L.spp_csr_mean_backward(_P(rowptr), _P(col), T, _P(gf), width, F, _P(ref), _st()))
        elif epi == "sum":
            nat.check(L.spp_csr_sum_backward(_P(rowptr), _P(col), T, S, _P(gf), width, F, 2.0, _P(ref), _st()))
        else:
            nat.check(L.spp_sage_operand_backward(_P(rowptr), _P(col), T, S, _P(gf), width, F, _P(ref), _st()))
            if z is not None:
                zf = z.float().contiguous()
                nat.check(L.spp_relu_dropout_backward_pre(_P(ref), _P(zf), ref.numel(), p, 1, seed, _P(ref), _st()))
        torch.cuda.synchronize()
        got = _bwd(nat.SPP_AGG_SCATTER, code, rowptr, col, T, S, g, F, gout, z=z, scale=2.0, act=(p, 1, seed))
        assert got.dtype == gout
        if float(g.float().mul(16).frac().abs().max()) == 0:      # the exact inputs
            assert torch.equal(got, ref.to(gout))
        else:
            torch.testing.assert_close(got.float(), ref.to(gout).float(), rtol=1e-4 if gout == F32 else 8e-3, atol=1e-5)


@pytest.mark.parametrize("K", [128, 100])
def test_gat_kernels_on_bf16_rows_equal_the_fp32_kernels_on_x_float(K):
    nat, L = _nat()
    S, T, slope = 5000, 1600, 0.2
    rowptr, col = _hop(T, S, 12, 21)
    E = col.numel()
    x = torch.randn((S, K), generator=torch.Generator().manual_seed(8)).to(BF16).cuda()
    xf = x.float().contiguous()
    v = torch.randn((2, K), device="cuda") * 0.2
    g_z = torch.randn((T, K), device="cuda")

    def run(xx, code):
        a_src, a_dst = torch.empty(S, device="cuda"), torch.empty(T, device="cuda")
        nat.check(L.spp_gat_logits(_P(xx), code, K, S, T, K, _P(v[0]), _P(v[1]), _P(a_src), _P(a_dst), _st()))
        z, rmax, rsum = torch.empty((T, K), device="cuda"), torch.empty(T, device="cuda"), torch.empty(T, device="cuda")
        nat.check(L.spp_gat_aggregate_forward(_P(rowptr), _P(col), T, _P(xx), code, K, K, _P(a_src), _P(a_dst), slope,
                                              _P(z), _P(rmax), _P(rsum), _st()))
        g_as, g_ad = torch.zeros(S, device="cuda"), torch.empty(T, device="cuda")
        g_x = torch.empty((S, K), device="cuda")
        nbytes = int(L.spp_gat_aggregate_backward_gather_workspace_bytes(T, S, E))
        ws = _ws(nbytes)
        nat.check(L.spp_gat_aggregate_backward_gather(_P(rowptr), _P(col), T, S, E, _P(xx), code, K, K, _P(a_src),
                                                      _P(a_dst), slope, _P(z), _P(rmax), _P(rsum), _P(g_z), _P(v[0]),
                                                      _P(v[1]), _P(g_x), _P(g_as), _P(g_ad), _P(ws), nbytes, _st()))
        g_xa = torch.zeros((S, K), device="cuda")
        g_as2, g_ad2 = torch.zeros(S, device="cuda"), torch.empty(T, device="cuda")
        nat.check(L.spp_gat_aggregate_backward(_P(rowptr), _P(col), T, _P(xx), code, K, K, _P(a_src), _P(a_dst), slope,
                                               _P(z), _P(rmax), _P(rsum), _P(g_z), _P(g_xa), _P(g_as2), _P(g_ad2), _st()))
        g_v = torch.empty((2, K), device="cuda")
        nat.check(L.spp_gat_logits_backward(_P(xx), code, K, S, T, K, _P(g_as), _P(g_ad), _P(g_v[0]), _P(g_v[1]), _st()))
        torch.cuda.synchronize()
        return (a_src, a_dst, z, rmax, rsum), (g_as, g_ad, g_x, g_xa, g_as2, g_ad2, g_v)

    det16, nd16 = run(x, nat.SPP_ELEM_BF16)
    det32, nd32 = run(xf, nat.SPP_ELEM_F32)
    for a, b in zip(det16, det32):                             # logits, z, softmax statistics: deterministic kernels
        assert torch.equal(a, b)
    for a, b in zip(nd16, nd32):                               # fp32 atomics in the backward: order not fixed
        assert float((a - b).norm() / b.norm()) < 1e-5


def test_unknown_element_codes_and_forms_are_refused():
    nat, L = _nat()
    T, S, F = 64, 128, 16
    rowptr, col = _hop(T, S, 4, 1)
    x = torch.randn((S, F), device="cuda")
    out = torch.empty((T, 2 * F), device="cuda")

    def fwd(**kw):
        d = dict(source=0, epilogue=nat.SPP_AGG_MEAN, x_elem=0, out_elem=0, rowptr_dev=rowptr.data_ptr(),
                 col_dev=col.data_ptr(), num_targets=T, x_dev=x.data_ptr(), x_stride_elems=F, F=F,
                 out_dev=out.data_ptr())
        d.update(kw)
        return L.spp_agg_forward(C.byref(nat.AggFwdDesc(**d)), _st())

    assert fwd() == 0
    for bad in (dict(x_elem=3), dict(x_elem=-1), dict(out_elem=1), dict(out_elem=7), dict(source=3), dict(epilogue=4),
                dict(epilogue=nat.SPP_AGG_OPERAND_ACT, x_elem=nat.SPP_ELEM_F16, p=0.5)):
        assert fwd(**bad) < 0, bad
    assert b"element code" in L.spp_last_error() or b"activated operand" in L.spp_last_error()
    g = torch.randn((T, F), device="cuda")
    gx = torch.empty((S, F), device="cuda")

    def bwd(**kw):
        d = dict(form=nat.SPP_AGG_SCATTER, epilogue=nat.SPP_AGG_MEAN, grad_elem=0, out_elem=0, z_elem=0,
                 rowptr_dev=rowptr.data_ptr(), col_dev=col.data_ptr(), num_targets=T, num_sources=S,
                 num_edges=col.numel(), grad_out_dev=g.data_ptr(), grad_out_stride_elems=F, F=F,
                 grad_x_dev=gx.data_ptr())
        d.update(kw)
        return L.spp_agg_backward(C.byref(nat.AggBwdDesc(**d)), None, 0, _st())

    assert bwd() == 0
    for bad in (dict(grad_elem=1), dict(grad_elem=5), dict(out_elem=1), dict(z_elem=9), dict(form=2), dict(epilogue=-1),
                dict(form=nat.SPP_AGG_GATHER), dict(out_elem=nat.SPP_ELEM_BF16)):  # the last two: plain mean gather,
        assert bwd(**bad) < 0, bad                                                   # bf16 scatter without workspace
    xs = torch.randn((S, 8), device="cuda")
    a = torch.empty(S, device="cuda")
    assert L.spp_gat_logits(_P(xs), 3, 8, S, T, 8, _P(a), _P(a), _P(a), _P(a), _st()) < 0
    torch.cuda.synchronize()
