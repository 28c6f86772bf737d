"""GPU: the thirteen aggregation entries that predate the descriptors (spp_csr_mean_forward ... spp_csr_sum_backward_gather)
are fixed-type spellings of spp_agg_forward / spp_agg_backward: each fills a descriptor from its arguments.  What that
can get wrong is one argument landing in the wrong field, so every call here uses arguments that differ from each
other and from the defaults -- self_scale 1.5, the fp16 flag as 2 ("any non-zero") and as 0, a table stride of F + 4 over
a 500-row table with random node ids, a dense row stride of F + 8, output and gradient strides 4 wider than the row
with NaN in the spare columns, p = 0.5 in training mode at a fixed seed -- and is held to a reference that does not go
through this code.

Exactness.  The forwards are compared bit for bit with the sequential restatements _seq_mean / _seq_sum; the sum's
fmaf(s, x_t, acc) equals their "acc + s * x_t" only when s * x_t is exact in fp32, so the fp32 rows hold fp16 values
(1.5 * an 11-bit significand is exact).  The scatter backwards are compared bit for bit with the gather form on a hop
whose col entries are all distinct: every source then receives at most one atomic add after the init pass.  The two
forms still round differently (the gather fuses w * g into its add, the scatter rounds the product first, and the
sum's self term s * g is an fmaf in one and a product in the other), so that hop's degrees are 0, 1, 2 or 4 and its
gradients small multiples of 1/16: every product and sum is then exact in fp32 and no rounding can tell the forms
apart.  On the general hop (degrees 0..5) both forms are held to float64 autograd within rtol 1e-4 / atol 1e-5, the
tolerance of test_gpu_gin_sage_ri.py for these kernels."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

T, S, R = 70, 200, 500
SCALE, P_DROP, SEED = 1.5, 0.5, 0x5EED5EED
NAN = float("nan")


def _nat():
    from salient_plusplus_amd import _native as nat
    return nat, nat.load()


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def hop():
    """degrees 0..5, every seventh row empty, repeated columns and self / target edges"""
    from test_gpu_gin_sage_ri import _hop
    rowptr, col = _hop(T, S, 5, 17, dup=True)
    deg = rowptr[1:] - rowptr[:-1]
    assert int(deg.max()) == 5 and bool((deg[::7] == 0).all()) and bool((col < T).any())
    return rowptr, col


@pytest.fixture(scope="module")
def distinct_hop():
    """every col entry distinct (so E <= S), degrees 0 / 1 / 2 / 4 with every seventh row empty"""
    g = torch.Generator().manual_seed(23)
    deg = torch.tensor([0, 1, 2, 4])[torch.randint(0, 4, (T,), generator=g)]
    deg[::7] = 0
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    E = int(rowptr[-1])
    assert T < E <= S
    col = torch.randperm(S, generator=g)[:E]
    assert bool((col < T).any()) and bool((col >= T).any())
    return rowptr.cuda(), col.cuda()


def _features(F, half):
    """the table [R, F] (row stride F + 4), the batch's node ids, and the batch's rows as a dense matrix (row stride
    F + 8); fp16, or fp32 holding the same fp16 values"""
    dtype = torch.float16 if half else torch.float32
    table = _randn((R, F + 4), 100 + F).half().to(dtype).cuda()[:, :F]
    n_id = torch.randint(0, R, (S,), generator=torch.Generator().manual_seed(3)).cuda()
    x = torch.full((S, F + 8), NAN, dtype=dtype, device="cuda")[:, :F]
    x.copy_(table[n_id])
    return table, n_id, x


def _out(width):
    """[T, width] inside a NaN-filled buffer whose rows are 4 elements wider"""
    buf = torch.full((T, width + 4), NAN, device="cuda")
    return buf, buf[:, :width]


def _spare_is_nan(buf, width):
    return bool(buf[:, width:].isnan().all())


# ---------------------------------------------------------------------------------------------- forwards
@pytest.mark.parametrize("flag", [2, 0])
@pytest.mark.parametrize("entry,F", [("mean", 8), ("mean", 7), ("operand", 8), ("operand", 7), ("operand_table", 8),
                                     ("operand_table", 7), ("operand_rows", 8), ("sum", 8), ("sum", 7), ("sum_table", 8),
                                     ("sum_table", 7), ("sum_rows", 8), ("sum_rows", 7)])
def test_forward_entries_equal_the_sequential_restatements(hop, entry, F, flag):
    from test_gpu_gin_sage_ri import _seq_sum
    from test_gpu_model_step import _seq_mean
    nat, L = _nat()
    rowptr, col = hop
    table, n_id, x = _features(F, half=bool(flag))
    addr = (table.data_ptr() + n_id * table.stride(0) * table.element_size()).contiguous()
    width = F if entry in ("mean", "sum", "sum_table", "sum_rows") else 2 * F
    buf, out = _out(width)
    a = (_P(rowptr), _P(col), T)
    dense = (_P(x), flag, x.stride(0), F)
    tab = (_P(table), flag, table.stride(0), R, _P(n_id), F)
    tail = (_P(buf), buf.stride(0), _st())
    if entry == "mean":
        rc = L.spp_csr_mean_forward(*a, *dense, *tail)
    elif entry == "operand":
        rc = L.spp_sage_operand_forward(*a, *dense, *tail)
    elif entry == "operand_table":
        rc = L.spp_sage_operand_forward_table(*a, *tab, *tail)
    elif entry == "operand_rows":
        rc = L.spp_sage_operand_forward_rows(*a, _P(addr), flag, F, *tail)
    elif entry == "sum":
        rc = L.spp_csr_sum_forward(*a, *dense, SCALE, *tail)
    elif entry == "sum_table":
        rc = L.spp_csr_sum_forward_table(*a, *tab, SCALE, *tail)
    else:
        rc = L.spp_csr_sum_forward_rows(*a, _P(addr), flag, F, SCALE, *tail)
    nat.check(rc)
    torch.cuda.synchronize()
    rows = x.contiguous()                                      # = table[n_id], the rows every source names
    if entry.startswith("sum"):
        want = _seq_sum(rows, rowptr, col, T, SCALE)
    else:
        want = _seq_mean(rows, rowptr, col, T)
        if entry != "mean":
            want = torch.cat([want, rows[:T].float()], dim=1)
    assert torch.equal(out, want)
    assert _spare_is_nan(buf, width)


@pytest.mark.parametrize("training", [1, 0])
def test_forward_act_equals_the_activation_followed_by_the_operand(hop, training):
    nat, L = _nat()
    rowptr, col = hop
    F = 8
    z = _randn((S, F), 5).cuda()
    y = torch.empty_like(z)
    nat.check(L.spp_relu_dropout_forward(_P(z), z.numel(), P_DROP, training, SEED, _P(y), _st()))
    ref_buf, ref = _out(2 * F)
    nat.check(L.spp_sage_operand_forward(_P(rowptr), _P(col), T, _P(y), 0, F, F, _P(ref_buf), ref_buf.stride(0), _st()))
    buf, out = _out(2 * F)
    nat.check(L.spp_sage_operand_forward_act(_P(rowptr), _P(col), T, _P(z), F, _P(buf), buf.stride(0), P_DROP, training,
                                             SEED, _st()))
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and not bool(out.isnan().any())
    assert _spare_is_nan(buf, 2 * F)
    if training:
        assert 0.3 < float((y == 0).float().mean()) < 0.95     # relu and dropout both acted


# ---------------------------------------------------------------------------------------------- backwards
def _grad(width, seed, exact=False):
    """the gradient [T, width] inside a buffer 4 elements wider whose spare columns hold NaN"""
    buf = torch.full((T, width + 4), NAN, device="cuda")
    if exact:                                                  # multiples of 1/16 in [-4, 4]
        g = torch.randint(-64, 65, (T, width), generator=torch.Generator().manual_seed(seed)).float() / 16
    else:
        g = _randn((T, width), seed)
    buf[:, :width] = g.cuda()
    return buf, buf[:, :width]


def _ref_grad(kind, rowptr, col, g, F, y=None, training=1):
    """torch autograd of the float64 restatement: the gradient w.r.t. x (or, kind 'act', the pre-activation z)"""
    from test_gpu_gin_sage_ri import _ref_sum
    x = torch.zeros((S, F), dtype=torch.float64, device="cuda", requires_grad=True)
    if kind == "sum":
        out = _ref_sum(x, rowptr, col, T, SCALE)
    else:
        xa = x
        if kind == "act":                                      # y = relu_dropout(z): y > 0 where z > 0 and kept
            xa = x * (y > 0).double() * (1.0 / (1.0 - P_DROP) if training else 1.0)
        deg = (rowptr[1:] - rowptr[:-1])
        mean = _ref_sum(xa, rowptr, col, T, 0.0) / deg.clamp(min=1).double().unsqueeze(-1)
        out = torch.cat([mean, xa[:T]], dim=1)
    (out * g.double()).sum().backward()
    return x.grad.float()


def _ws(L, rowptr, col):
    nbytes = int(L.spp_sage_operand_backward_workspace_bytes(T, S, col.numel()))
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


def _desc_backward(form, epilogue, rowptr, col, gbuf, F, ws, nbytes, z=None):
    nat, L = _nat()
    gx = torch.full((S, F), NAN, device="cuda")
    d = nat.AggBwdDesc(form=form, epilogue=epilogue, grad_elem=0, out_elem=0, z_elem=0, rowptr_dev=rowptr.data_ptr(),
                       col_dev=col.data_ptr(), num_targets=T, num_sources=S, num_edges=col.numel(),
                       grad_out_dev=gbuf.data_ptr(), grad_out_stride_elems=gbuf.stride(0), F=F, grad_x_dev=gx.data_ptr(),
                       z_dev=z.data_ptr() if z is not None else None, self_scale=SCALE, p=P_DROP, training=1, seed=SEED)
    nat.check(L.spp_agg_backward(C.byref(d), _P(ws), nbytes, _st()))
    return gx


@pytest.mark.parametrize("entry,F", [("operand", 8), ("act", 8), ("sum", 8), ("sum", 7)])
def test_gather_backward_entries_match_autograd_and_the_descriptor(hop, entry, F):
    nat, L = _nat()
    rowptr, col = hop
    E = col.numel()
    width = F if entry == "sum" else 2 * F
    gbuf, g = _grad(width, 31 + F)
    ws, nbytes = _ws(L, rowptr, col)
    gx = torch.full((S, F), NAN, device="cuda")
    a = (_P(rowptr), _P(col), T, S, E, _P(gbuf), gbuf.stride(0), F)
    z = y = None
    if entry == "operand":
        nat.check(L.spp_sage_operand_backward_gather(*a, _P(gx), _P(ws), nbytes, _st()))
        code = nat.SPP_AGG_OPERAND
    elif entry == "act":
        z = _randn((S, F), 6).cuda()
        y = torch.empty_like(z)
        nat.check(L.spp_relu_dropout_forward(_P(z), z.numel(), P_DROP, 1, SEED, _P(y), _st()))
        nat.check(L.spp_sage_operand_backward_gather_act(*a, _P(gx), _P(ws), nbytes, _P(z), P_DROP, 1, SEED, _st()))
        code = nat.SPP_AGG_OPERAND_ACT
    else:
        nat.check(L.spp_csr_sum_backward_gather(*a, SCALE, _P(gx), _P(ws), nbytes, _st()))
        code = nat.SPP_AGG_SUM
    torch.cuda.synchronize()
    torch.testing.assert_close(gx, _ref_grad(entry, rowptr, col, g, F, y), rtol=1e-4, atol=1e-5)
    by_desc = _desc_backward(nat.SPP_AGG_GATHER, code, rowptr, col, gbuf, F, ws, nbytes, z)
    torch.cuda.synchronize()
    assert torch.equal(gx, by_desc)


@pytest.mark.parametrize("entry,F", [("operand", 8), ("sum", 8), ("sum", 7)])
def test_scatter_backward_entries_match_the_gather_form_and_autograd(hop, distinct_hop, entry, F):
    nat, L = _nat()
    width = F if entry == "sum" else 2 * F

    def both(rowptr, col, gbuf):
        ws, nbytes = _ws(L, rowptr, col)
        sc, ga = torch.full((S, F), NAN, device="cuda"), torch.full((S, F), NAN, device="cuda")
        a = (_P(rowptr), _P(col), T, S)
        gr = (_P(gbuf), gbuf.stride(0), F)
        if entry == "operand":
            nat.check(L.spp_sage_operand_backward(*a, *gr, _P(sc), _st()))
            nat.check(L.spp_sage_operand_backward_gather(*a, col.numel(), *gr, _P(ga), _P(ws), nbytes, _st()))
        else:
            nat.check(L.spp_csr_sum_backward(*a, *gr, SCALE, _P(sc), _st()))
            nat.check(L.spp_csr_sum_backward_gather(*a, col.numel(), *gr, SCALE, _P(ga), _P(ws), nbytes, _st()))
        torch.cuda.synchronize()
        return sc, ga

    rowptr, col = distinct_hop                                 # one order of summation, exact arithmetic: bit-equal
    gbuf, g = _grad(width, 41 + F, exact=True)
    sc, ga = both(rowptr, col, gbuf)
    assert torch.equal(sc, ga) and not bool(sc.isnan().any())
    assert torch.equal(sc, _ref_grad(entry, rowptr, col, g, F))    # (exact in fp32, so float64 autograd agrees too)
    rowptr, col = hop                                          # atomics in any order: the kernels' tolerance
    gbuf, g = _grad(width, 51 + F)
    sc, ga = both(rowptr, col, gbuf)
    want = _ref_grad(entry, rowptr, col, g, F)
    torch.testing.assert_close(sc, want, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(ga, want, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------- refusals
REFUSALS = ["operand_forward_narrow_out", "operand_forward_rows_F6", "operand_forward_act_p1", "sum_backward_S_lt_T",
            "sum_backward_gather_small_ws", "sum_forward_table_no_n_id", "operand_forward_narrow_rows",
            "operand_backward_gather_act_p1"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refused_calls_launch_nothing_and_name_the_entry_called(hop, case):
    """each call returns SPP_ERR_INVALID, leaves its NaN-filled output untouched, and spp_last_error() starts with the
    name of the entry that was called (the last two cases reported as another entry before)"""
    nat, L = _nat()
    rowptr, col = hop
    E = col.numel()
    F = 6 if case == "operand_forward_rows_F6" else 8
    x = _randn((S, F), 7).cuda()
    g = _randn((T, 2 * F), 8).cuda()
    out = torch.full((S, 2 * F + 4), NAN, device="cuda")       # large enough for every output below
    ws, nbytes = _ws(L, rowptr, col)
    a = (_P(rowptr), _P(col), T)
    if case == "operand_forward_narrow_out":
        who = "spp_sage_operand_forward"
        rc = L.spp_sage_operand_forward(*a, _P(x), 0, F, F, _P(out), F, _st())
    elif case == "operand_forward_rows_F6":
        who = "spp_sage_operand_forward_rows"
        addr = (x.data_ptr() + torch.arange(S, device="cuda") * F * 4).contiguous()
        rc = L.spp_sage_operand_forward_rows(*a, _P(addr), 0, F, _P(out), out.stride(0), _st())
    elif case == "operand_forward_act_p1":
        who = "spp_sage_operand_forward_act"
        rc = L.spp_sage_operand_forward_act(*a, _P(x), F, _P(out), out.stride(0), 1.0, 1, SEED, _st())
    elif case == "sum_backward_S_lt_T":
        who = "spp_csr_sum_backward"
        rc = L.spp_csr_sum_backward(*a, T - 1, _P(g), g.stride(0), F, SCALE, _P(out), _st())
    elif case == "sum_backward_gather_small_ws":
        who = "spp_csr_sum_backward_gather"
        rc = L.spp_csr_sum_backward_gather(*a, S, E, _P(g), g.stride(0), F, SCALE, _P(out), _P(ws), 16, _st())
    elif case == "sum_forward_table_no_n_id":
        who = "spp_csr_sum_forward_table"
        rc = L.spp_csr_sum_forward_table(*a, _P(x), 0, F, S, None, F, SCALE, _P(out), out.stride(0), _st())
    elif case == "operand_forward_narrow_rows":
        who = "spp_sage_operand_forward"
        rc = L.spp_sage_operand_forward(*a, _P(x), 0, F - 4, F, _P(out), out.stride(0), _st())
    else:
        who = "spp_sage_operand_backward_gather_act"
        rc = L.spp_sage_operand_backward_gather_act(*a, S, E, _P(g), g.stride(0), F, _P(out), _P(ws), nbytes, _P(x), 1.0,
                                                    1, SEED, _st())
    err = L.spp_last_error().decode()
    torch.cuda.synchronize()
    assert rc < 0
    assert bool(out.isnan().all())
    assert err.startswith(who + ":"), err
    if case == "sum_forward_table_no_n_id":
        assert "node ids" in err
    if case == "sum_backward_gather_small_ws":
        assert "workspace too small" in err
    if case == "sum_backward_S_lt_T":
        assert "bad sizes" in err
