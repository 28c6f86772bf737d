"""spp_graph_agg_forward (csrc/graph_aggregate.hip) through inference.graph_aggregate: the summation contract of
include/spp.h pinned bit for bit where it can be (rows of at most C entries against spp_agg_forward, long rows against an
fp32 restatement of the contract on the CPU) and by the derived bound of the two-level sum against float64."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FS = [1, 3, 4, 32, 100, 128, 256]
XDTYPES = [torch.float32, torch.float16, torch.bfloat16]
OUT_DTYPES = [torch.float32, torch.bfloat16]
EPILOGUES = [("mean", 0.0), ("operand", 0.0), ("sum", 1.5), ("sum", 0.0)]
U = 2.0 ** -24


def _chunk():
    from salient_plusplus_amd.inference import graph_agg_chunk
    return graph_agg_chunk()


@functools.lru_cache(maxsize=None)
def _graph():
    """~400 nodes: degrees 0, 1, 2, C-1, C, C+1, 2C, 3C+5, a hub of 20C+3, self-loops, repeated neighbours and ordinary
    rows of 3..15 entries; (rowptr, col) on the CPU"""
    Cc = _chunk()
    assert Cc >= 32
    g = torch.Generator().manual_seed(7)
    N = 401
    deg = torch.randint(3, 16, (N,), generator=g)
    special = {0: 0, 5: 1, 9: 2, 17: Cc - 1, 33: Cc, 64: Cc + 1, 130: 2 * Cc, 131: 3 * Cc + 5, 200: 20 * Cc + 3, 259: 0,
               260: Cc + 1, N - 1: 2 * Cc + 1}
    for k, v in special.items():
        deg[k] = v
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    for t in (5, 9, 17, 64, 131, 200, 300):                    # self-loops
        col[rowptr[t]] = t
    for t in (9, 33, 130, 200, 301):                           # repeated neighbours, side by side
        col[rowptr[t + 1] - 1] = col[rowptr[t + 1] - 2]
    return rowptr, col


@functools.lru_cache(maxsize=None)
def _dev_graph():
    rowptr, col = _graph()
    return rowptr.cuda(), col.cuda()


@functools.lru_cache(maxsize=None)
def _x(F_, dtype):
    N = _graph()[0].numel() - 1
    x = torch.randn((N, F_), generator=torch.Generator().manual_seed(100 + F_)) * 2.0
    return x.to(dtype)


def _sums64(x, rowptr, col):
    """(sum, sum of magnitudes) of every row's neighbour rows in float64 on the CPU"""
    N = rowptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(N), rowptr[1:] - rowptr[:-1])
    xd = x.double()
    s = torch.zeros((N, x.size(1)), dtype=torch.float64).index_add_(0, rows, xd[col])
    m = torch.zeros((N, x.size(1)), dtype=torch.float64).index_add_(0, rows, xd[col].abs())
    return s, m


@functools.lru_cache(maxsize=None)
def _ref64(F_, dtype):
    return _sums64(_x(F_, dtype), *_graph())


def _contract_sum32(x, rowptr, col, t, Cc):
    """the contract itself in fp32 on the CPU: chunks of C summed in CSR order from zero, chunk sums added in chunk order"""
    xf = x.float()
    b, e = int(rowptr[t]), int(rowptr[t + 1])
    total = torch.zeros(x.size(1), dtype=torch.float32)
    for cb in range(b, e, Cc):
        acc = torch.zeros(x.size(1), dtype=torch.float32)
        for k in range(cb, min(e, cb + Cc)):
            acc = acc + xf[int(col[k])]
        total = total + acc
    return total


@functools.lru_cache(maxsize=None)
def _ref_contract(F_, dtype):
    rowptr, col = _graph()
    Cc = _chunk()
    deg = rowptr[1:] - rowptr[:-1]
    long_rows = torch.nonzero(deg > Cc).flatten().tolist()
    return long_rows, torch.stack([_contract_sum32(_x(F_, dtype), rowptr, col, t, Cc) for t in long_rows])


def _expected64(epilogue, scale, x, s64, m64, deg, targets):
    """(float64 result, magnitude sum the error bound scales with) of the left F columns for `targets`"""
    xt = x.double()[targets]
    if epilogue == "sum":
        return s64[targets] + scale * xt, m64[targets] + abs(scale) * xt.abs()
    d = deg[targets].clamp(min=1).double().unsqueeze(1)
    return s64[targets] / d, m64[targets] / d


def _assert_within_bound(got, want, mag, deg, Cc, what):
    """|error| <= (C + ceil(d / C) + 2) * 2^-24 * sum |x_j| (the two-level fp32 sum: C - 1 roundings in a chunk,
    ceil(d / C) - 1 across chunks, plus the scale or the self term), and 2^-8 |result| more for a bf16 output"""
    n = (Cc + torch.ceil(deg.double() / Cc) + 2).unsqueeze(1)
    bound = n * U * mag
    if got.dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * want.abs()
    err = (got.double().cpu() - want).abs()
    print(f"{what}: max err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


def _agg(x, epilogue, scale, out_dtype, **tgt):
    from salient_plusplus_amd.inference import graph_aggregate
    rowptr, col = _dev_graph()
    return graph_aggregate(x, rowptr, col, epilogue=epilogue, self_scale=scale, out_dtype=out_dtype, **tgt)


@pytest.mark.parametrize("xdtype", XDTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("F_", FS)
def test_rows_match_the_hop_kernel_and_the_contract(F_, xdtype):
    """items 1 and 2: rows of d <= C are bit-identical to spp_agg_forward over the whole graph as one hop (fp32 out, and
    bf16 out = that rounded once); longer rows hold the two-level bound against float64, and the plain sum equals the
    fp32 restatement of the contract bit for bit"""
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd.models import _agg_forward
    Cc = _chunk()
    rowptr_c, col_c = _graph()
    rowptr, col = _dev_graph()
    N = rowptr_c.numel() - 1
    deg = rowptr_c[1:] - rowptr_c[:-1]
    short = (deg <= Cc).cuda()
    assert int((~short).sum()) >= 6 and int(deg.max()) == 20 * Cc + 3
    xc = _x(F_, xdtype)
    x = xc.cuda()
    s64, m64 = _ref64(F_, xdtype)
    long_rows, contract = _ref_contract(F_, xdtype)
    codes = {"mean": nat.SPP_AGG_MEAN, "operand": nat.SPP_AGG_OPERAND, "sum": nat.SPP_AGG_SUM}
    everyone = torch.arange(N)
    for epilogue, scale in EPILOGUES:
        hop32 = _agg_forward(codes[epilogue], rowptr, col, N, x, torch.float32, scale=scale)
        for odt in OUT_DTYPES:
            got = _agg(x, epilogue, scale, odt, row0=0, num_targets=N)
            assert got.dtype == odt and got.shape == hop32.shape
            what = f"F={F_} {xdtype} {epilogue} s={scale} -> {odt}"
            if odt == torch.float32:
                assert torch.equal(got[short], hop32[short]), what
            else:
                hop16 = _agg_forward(codes[epilogue], rowptr, col, N, x, torch.bfloat16, scale=scale)
                assert torch.equal(got[short], hop16[short]), what
                assert torch.equal(got[short], hop32[short].to(torch.bfloat16)), what + " (rounded once)"
            want, mag = _expected64(epilogue, scale, xc, s64, m64, deg, everyone)
            _assert_within_bound(got[:, :F_], want, mag, deg, Cc, what)
            if epilogue == "operand":
                assert torch.equal(got[:, F_:], x.float().to(odt)), what + " (right half)"
            if epilogue == "sum" and scale == 0.0:
                want32 = contract.cuda()
                assert torch.equal(got[long_rows], want32 if odt == torch.float32 else want32.to(odt)), what + " (contract)"


@pytest.mark.parametrize("xdtype", XDTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("F_", FS)
def test_result_is_independent_of_the_launch(F_, xdtype):
    """item 3: one slab, slabs of 1 / 7 / 130 rows (row0 != 0, the last one ending at N), a shuffled list with
    duplicates and a second run all give the same bits for every row"""
    rowptr_c, _ = _graph()
    N = rowptr_c.numel() - 1
    x = _x(F_, xdtype).cuda()
    g = torch.Generator().manual_seed(3)
    ids = torch.cat([torch.randperm(N, generator=g), torch.randint(0, N, (57,), generator=g)]).cuda()
    for epilogue, scale in EPILOGUES[:3]:
        for odt in OUT_DTYPES:
            full = _agg(x, epilogue, scale, odt, row0=0, num_targets=N)
            assert torch.equal(_agg(x, epilogue, scale, odt, row0=0, num_targets=N), full)
            listed = _agg(x, epilogue, scale, odt, target_ids=ids)
            assert torch.equal(listed, full[ids]), (epilogue, odt)
            assert torch.equal(_agg(x, epilogue, scale, odt, target_ids=ids), listed)
            for rows in (1, 7, 130):
                parts = [_agg(x, epilogue, scale, odt, row0=s, num_targets=min(rows, N - s)) for s in range(0, N, rows)]
                assert torch.equal(torch.cat(parts), full), (epilogue, odt, rows)


@pytest.mark.parametrize("xdtype", XDTYPES, ids=lambda d: str(d).split(".")[-1])
def test_operand_of_a_slab_carries_the_slab_rows(xdtype):
    """item 4: row0 = 123 -- the right half is x[123 : 123 + T] as fp32, exactly; a strided view of a wider table reads
    the same"""
    for F_ in (3, 32, 100):
        xc = _x(F_, xdtype)
        x = xc.cuda()
        T = 200
        got = _agg(x, "operand", 0.0, torch.float32, row0=123, num_targets=T)
        assert torch.equal(got[:, F_:], x[123:123 + T].float())
        full = _agg(x, "operand", 0.0, torch.float32, row0=0, num_targets=x.size(0))
        assert torch.equal(got, full[123:123 + T])
        wide = torch.zeros((x.size(0), F_ + 28), dtype=xdtype, device="cuda")
        wide[:, :F_] = x
        assert torch.equal(_agg(wide[:, :F_], "operand", 0.0, torch.float32, row0=123, num_targets=T), got)


def test_rows_beyond_a_4_gib_offset():
    """item 5: x is a [4100, 32] view of a [4100, 2^20] fp16 allocation (8.6 GB): rows past 2048 start beyond a 2^32 byte
    offset, and most edges point there"""
    from salient_plusplus_amd.inference import graph_aggregate
    free, _total = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip(f"needs 12 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    Cc = _chunk()
    N, F_ = 4100, 32
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(0, 21, (N,), generator=g)
    deg[7], deg[2049], deg[4099] = Cc + 6, 3 * Cc + 1, 2 * Cc
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    E = int(rowptr[-1])
    col = torch.randint(3000, N, (E,), generator=g)
    col[::9] = torch.randint(0, N, (col[::9].numel(),), generator=g)
    col[-1] = N - 1
    xc = (torch.randn((N, F_), generator=g) * 2.0).to(torch.float16)
    big = torch.zeros((N, 1 << 20), dtype=torch.float16, device="cuda")
    x = big[:, :F_]
    x.copy_(xc)
    assert x.stride(0) == 1 << 20 and (N - 1) * x.stride(0) * 2 > 2 ** 32
    s64, m64 = _sums64(xc, rowptr, col)
    everyone = torch.arange(N)
    rp, cl = rowptr.cuda(), col.cuda()
    for epilogue, scale in (("mean", 0.0), ("sum", 1.0)):
        got = graph_aggregate(x, rp, cl, row0=0, num_targets=N, epilogue=epilogue, self_scale=scale)
        want, mag = _expected64(epilogue, scale, xc, s64, m64, deg, everyone)
        _assert_within_bound(got, want, mag, deg, Cc, f"4 GiB {epilogue}")
    ids = torch.tensor([4099, 2049, 7, 4099, 3000], dtype=torch.int64).cuda()
    got = graph_aggregate(x, rp, cl, target_ids=ids, epilogue="operand")
    assert torch.equal(got[:, F_:], xc[ids.cpu()].float().cuda())
    want, mag = _expected64("mean", 0.0, xc, s64, m64, deg, ids.cpu())
    _assert_within_bound(got[:, :F_], want, mag, deg[ids.cpu()], Cc, "4 GiB list")
    del big, x, got
    torch.cuda.empty_cache()


def test_ids_that_leave_the_graph():
    """the documented rule: a col entry outside [0, x_rows) reads row 0, a target id outside gives a row of zeros"""
    from salient_plusplus_amd.inference import graph_aggregate
    x = torch.arange(1, 13, dtype=torch.float32).reshape(3, 4).cuda()
    rowptr = torch.tensor([0, 2, 3, 3]).cuda()
    col = torch.tensor([1, 99, -5]).cuda()
    got = graph_aggregate(x, rowptr, col, target_ids=torch.tensor([0, 1, 7, -1, 2]).cuda(), epilogue="operand")
    want = torch.zeros((5, 8), device="cuda")
    want[0, :4], want[0, 4:] = (x[1] + x[0]) * 0.5, x[0]
    want[1, :4], want[1, 4:] = x[0], x[1]
    want[4, 4:] = x[2]
    assert torch.equal(got, want)


def test_refusals_return_a_status_and_launch_nothing():
    """item 6"""
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    rowptr, col = _dev_graph()
    N, F_ = rowptr.numel() - 1, 4
    x = _x(F_, torch.float32).cuda()
    out = torch.full((N + 1, F_), -7.0, device="cuda")
    ids = torch.arange(N).cuda()
    nbytes = int(L.spp_graph_agg_workspace_bytes(N))
    assert nbytes >= 8 * N and int(L.spp_graph_agg_workspace_bytes(0)) >= 16
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                          # noqa: E731

    def call(ws_ptr=None, ws_bytes=nbytes, **kw):
        f = dict(epilogue=nat.SPP_AGG_MEAN, x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, rowptr_dev=p(rowptr),
                 col_dev=p(col), x_dev=p(x), x_stride_elems=F_, x_rows=N, F=F_, target_row0=0, target_ids_dev=None,
                 num_targets=N, out_dev=p(out), out_stride_elems=0, self_scale=0.0)
        f.update(kw)
        d = nat.GraphAggDesc(**f)
        return L.spp_graph_agg_forward(C.byref(d), p(ws) if ws_ptr is None else ws_ptr, ws_bytes, None)

    refused = {
        "both target forms": dict(target_ids_dev=p(ids)),
        "neither target form": dict(target_row0=-1),
        "slab past the graph": dict(target_row0=1, num_targets=N),
        "unknown x element code": dict(x_elem=7),
        "fp16 output": dict(out_elem=nat.SPP_ELEM_F16),
        "fp8 rows": dict(x_elem=nat.SPP_ELEM_FP8_E4M3),
        "activation on load": dict(epilogue=nat.SPP_AGG_OPERAND_ACT),
        "unknown epilogue": dict(epilogue=9),
        "misaligned output": dict(out_dev=C.c_void_p(out.data_ptr() + 4)),
        "misaligned output stride": dict(out_stride_elems=F_ + 1),
        "workspace too small": dict(ws_bytes=nbytes - 1),
        "no workspace": dict(ws_ptr=C.c_void_p(0)),
        "misaligned workspace": dict(ws_ptr=C.c_void_p(ws.data_ptr() + 8)),
    }
    for what, kw in refused.items():
        assert call(**kw) == -1, what                       # SPP_ERR_INVALID
        assert L.spp_last_error(), what
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and not bool(ws.any()), "a refused call wrote something"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[:N] != -7.0).all()) and bool((out[N] == -7.0).all())


def test_wrapper_is_forward_only():
    from salient_plusplus_amd.inference import graph_aggregate
    rowptr, col = _dev_graph()
    x = _x(4, torch.float32).cuda()
    out = graph_aggregate(x, rowptr, col, row0=0, num_targets=5)
    assert out.grad_fn is None and not out.requires_grad
    with pytest.raises(RuntimeError, match="requires grad"):
        graph_aggregate(x.clone().requires_grad_(), rowptr, col, row0=0, num_targets=5)
    small = torch.empty(8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="workspace"):
        graph_aggregate(x, rowptr, col, row0=0, num_targets=5, workspace=small)
