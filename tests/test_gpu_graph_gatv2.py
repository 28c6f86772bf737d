"""spp_graph_gatv2_forward (inference.graph_gatv2_aggregate; csrc/graph_gatv2.hip, spp.h f3w) on the planted graph of
tests/graph_gatv2_f64.py: every element against the float64 restatement within its first-order bound, the short rows
bit for bit against spp_gatv2_forward, a row's bits against slabs, lists and repeated calls, the fused ReLU, ids that
leave the graph, and the refusals on device tensors.  The bounds come from the arithmetic (graph_gatv2_f64.py), never
from what the kernel gives; every test prints the largest err / bound it saw (DESIGN section 7 f3w records them)."""
import functools

import pytest
import torch

import gatv2_f64
import graph_gatv2_f64 as gg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4), (4, 16), (8, 128), (2, 256)]               # <NQ, CPH> = <1,1>, <1,1> (4 heads a chunk), <4,1>, <2,1>;
MORE_SHAPES = [(1, 512), (1, 1024), (2, 512)]                 # <2,2>, <4,4>, <4,2>: the families with CPH > 1
ROW_DTYPES = [torch.float32, torch.bfloat16]
N = gg.N


def _name(d):
    return str(d).split(".")[-1]


@functools.lru_cache(maxsize=None)
def _cg():
    from salient_plusplus_amd.inference import graph_gatv2_chunk
    return graph_gatv2_chunk()


@functools.lru_cache(maxsize=None)
def _graph():
    hop = gg.planted_graph(_cg())
    return hop, hop.rowptr.cuda(), hop.col.cuda()


@functools.lru_cache(maxsize=None)
def _case(regime, H, Cc, dtype, alias):
    """CPU inputs [N, H, C] and their CUDA copies [N, H * C]; aliased: x_r IS x_l"""
    hop = _graph()[0]
    x_l, x_r, att, _g = gatv2_f64.inputs(regime, hop, H, Cc, dtype)
    if alias:
        x_r = x_l
    dl = x_l.reshape(N, H * Cc).cuda()
    dr = dl if alias else x_r.reshape(N, H * Cc).cuda()
    return x_l, x_r, att, dl, dr, att.cuda()


def _run(regime, H, Cc, dtype, alias, slope, **kw):
    from salient_plusplus_amd.inference import graph_gatv2_aggregate
    _hop, rowptr, col = _graph()
    _xl, _xr, _att, dl, dr, datt = _case(regime, H, Cc, dtype, alias)
    if not any(k in kw for k in ("row0", "target_ids")):
        kw.update(row0=0, num_targets=N)
    return graph_gatv2_aggregate(dl, dr, datt, rowptr, col, negative_slope=slope, **kw)


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "aliased"])
@pytest.mark.parametrize("dtype", ROW_DTYPES, ids=_name)
@pytest.mark.parametrize("H,Cc", SHAPES + MORE_SHAPES)
def test_every_element_is_within_its_float64_bound(H, Cc, dtype, alias):
    hop = _graph()[0]
    regimes = gatv2_f64.REGIMES if (H, Cc) in SHAPES else ["model", "wide"]
    top, top_bf = (0.0, ""), (0.0, "")
    for slope in gatv2_f64.SLOPES:
        for regime in regimes:
            x_l, x_r, att = _case(regime, H, Cc, dtype, alias)[:3]
            ref = gg.reference(hop, x_l, x_r, att, slope, _cg())
            got = _run(regime, H, Cc, dtype, alias, slope).view(N, H, Cc)
            ratio, where = gatv2_f64.worst(got, ref.out, ref.b_out, hop)
            top = max(top, (ratio, f"{regime} slope {slope:.3g}: {where}"))
            assert ratio <= 1.0, (regime, slope, where)
            if regime in ("model", "wide"):               # the bf16 output: one more rounding
                got = _run(regime, H, Cc, dtype, alias, slope, out_dtype=torch.bfloat16)
                assert got.dtype == torch.bfloat16
                ratio, where = gatv2_f64.worst(got.view(N, H, Cc), ref.out, gg.widen_bf16(ref.out, ref.b_out), hop)
                top_bf = max(top_bf, (ratio, f"{regime} slope {slope:.3g}: {where}"))
                assert ratio <= 1.0, ("bf16 out", regime, slope, where)
    print(f"GRAPH_GATV2 H={H} C={Cc} rows={_name(dtype)} {'aliased' if alias else 'distinct'}: largest err / bound "
          f"{top[0]:.3f} ({top[1]}); bf16 output {top_bf[0]:.3f}")


def test_rows_without_neighbours_return_their_own_row():
    got = _run("model", 4, 16, torch.float32, False, 0.2)
    x_l = _case("model", 4, 16, torch.float32, False)[3]
    for t in (0, gg.ISOLATED, gg.ONLY_SELF):
        assert torch.equal(got[t], x_l[t]), t


@pytest.mark.parametrize("alias", [False, True], ids=["distinct", "aliased"])
@pytest.mark.parametrize("dtype", ROW_DTYPES + [torch.float16], ids=_name)
@pytest.mark.parametrize("H,Cc", SHAPES + MORE_SHAPES)
def test_short_rows_are_the_bits_of_the_training_forward(H, Cc, dtype, alias):
    """rows of at most C_g raw entries, fp32 output, relu = 0: spp_gatv2_forward over the whole graph as one hop
    (T = S = N) runs the same body (csrc/gatv2_core.hip.h)"""
    from salient_plusplus_amd.models import _GATv2Layer
    hop, rowptr, col = _graph()
    short = (hop.raw <= _cg()).cuda()
    assert int(short.sum()) > 600 and int((~short).sum()) >= 5
    for slope in gatv2_f64.SLOPES:
        for regime in ("model", "wide", "zero"):
            _xl, _xr, _att, dl, dr, datt = _case(regime, H, Cc, dtype, alias)
            want = _GATv2Layer.apply(dl, dr, datt, rowptr, col, slope).reshape(N, H * Cc)
            got = _run(regime, H, Cc, dtype, alias, slope)
            assert torch.equal(got[short].view(torch.int32), want[short].view(torch.int32)), (regime, slope)


@pytest.mark.parametrize("dtype", ROW_DTYPES + [torch.float16], ids=_name)
@pytest.mark.parametrize("H,Cc", SHAPES + MORE_SHAPES)
def test_the_long_kernel_gives_the_bits_of_the_short_walk(H, Cc, dtype):
    """rows kernel against long kernel.  Row 12 has C_g + 1 raw entries and the last one, all of chunk 1, is 12 itself:
    the long kernel merges chunk 0's state with an empty one (f1 = expf(0) = 1, f2 = expf(-inf) = 0: exact), so it must
    return what the rows kernel returns for the row cut to its first C_g entries.  Row 9 likewise: its chunk 1 is empty,
    so it equals the long row made of its chunks 0 and 2 alone -- two merges against one, the empty one changing nothing."""
    from salient_plusplus_amd.inference import graph_gatv2_aggregate
    hop, rowptr, col = _graph()
    Cg = _cg()
    _xl, _xr, _att, dl, dr, datt = _case("model", H, Cc, dtype, False)
    ids = torch.tensor([12, gg.EMPTY_CHUNK_ROW], device="cuda")
    got = graph_gatv2_aggregate(dl, dr, datt, rowptr, col, target_ids=ids)
    b12, b9, e9 = int(hop.rowptr[12]), int(hop.rowptr[gg.EMPTY_CHUNK_ROW]), int(hop.rowptr[gg.EMPTY_CHUNK_ROW + 1])
    cut = torch.cat([hop.col[:b12 + Cg], hop.col[b12 + Cg + 1:]])
    deg = hop.raw.clone()
    deg[12] = Cg
    cut_ptr = torch.zeros(N + 1, dtype=torch.int64)
    cut_ptr[1:] = torch.cumsum(deg, 0)
    short = graph_gatv2_aggregate(dl, dr, datt, cut_ptr.cuda(), cut.cuda(), target_ids=ids[:1])
    assert torch.equal(got[0].view(torch.int32), short[0].view(torch.int32))
    cut = torch.cat([hop.col[:b9 + Cg], hop.col[b9 + 2 * Cg:]])
    deg = hop.raw.clone()
    deg[gg.EMPTY_CHUNK_ROW] = e9 - b9 - Cg
    cut_ptr[1:] = torch.cumsum(deg, 0)
    two = graph_gatv2_aggregate(dl, dr, datt, cut_ptr.cuda(), cut.cuda(), target_ids=ids[1:])
    assert torch.equal(got[1].view(torch.int32), two[0].view(torch.int32))


@pytest.mark.parametrize("H,Cc,dtype,alias", [(4, 16, torch.float32, False), (8, 128, torch.bfloat16, True),
                                              (1, 4, torch.float32, True), (2, 256, torch.bfloat16, False),
                                              (1, 1024, torch.float32, False)])
def test_a_rows_bits_depend_on_the_row_alone(H, Cc, dtype, alias):
    from salient_plusplus_amd.inference import graph_gatv2_workspace_bytes
    hop = _graph()[0]
    call = functools.partial(_run, "model", H, Cc, dtype, alias, 0.2)
    whole = call()
    for rows in (64, 1000, 1 << 20):
        parts = [call(row0=s, num_targets=min(rows, N - s)) for s in range(0, N, rows)]
        assert torch.equal(torch.cat(parts), whole), rows
    assert torch.equal(call(target_ids=torch.arange(N, device="cuda")), whole)
    g = torch.Generator().manual_seed(2)
    ids = torch.cat([torch.randperm(N, generator=g)[:90], torch.tensor(hop.planted + [8, 7, 8, gg.EMPTY_CHUNK_ROW])])
    ids = ids[torch.randperm(ids.numel(), generator=g)].cuda()
    assert torch.equal(call(target_ids=ids), whole[ids])
    ws = torch.empty(graph_gatv2_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    first, second = call(workspace=ws), call(workspace=ws)
    assert torch.equal(first, second) and torch.equal(first, whole)
    assert torch.equal(call(target_ids=ids, workspace=ws), whole[ids])
    out = torch.full((N + 2, H * Cc + 4), 7.0, device="cuda")         # rows of a larger matrix; the rest is not touched
    call(out=out[1:N + 1, :H * Cc])
    assert torch.equal(out[1:N + 1, :H * Cc], whole) and bool((out[:, H * Cc:] == 7).all()) and bool((out[0] == 7).all())


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=_name)
@pytest.mark.parametrize("H,Cc", [(4, 16), (2, 256)])
def test_relu_is_the_maximum_with_zero_bit_for_bit(H, Cc, out_dtype):
    plain = _run("model", H, Cc, torch.float32, False, 0.2, out_dtype=out_dtype)
    fused = _run("model", H, Cc, torch.float32, False, 0.2, out_dtype=out_dtype, relu=True)
    assert bool((plain < 0).any()) and torch.equal(fused, torch.clamp(plain, min=0))


@pytest.mark.parametrize("H,Cc", [(4, 16), (8, 128)])
def test_ids_that_leave_the_graph(H, Cc):
    """what the contract defines and nothing beyond it: an entry outside [0, N) reads node 0 (and is skipped in row 0),
    a target outside gives zeros"""
    from salient_plusplus_amd.inference import graph_gatv2_aggregate
    hop, rowptr, col = _graph()
    Cg = _cg()
    _xl, _xr, _att, dl, dr, datt = _case("model", H, Cc, torch.float32, False)
    bad = col.clone()
    for t, k, j in ((10, 1, N), (30, 0, -3), (7, 5, N + 5), (7, Cg + 3, 1 << 40), (8, 7 * Cg + 1, -1), (1, 0, N),
                    (gg.EMPTY_CHUNK_ROW, Cg + 2, N + 1)):
        if int(hop.raw[t]) > k:
            bad[rowptr[t] + k] = j
    as_node0 = torch.where((bad >= 0) & (bad < N), bad, torch.zeros_like(bad))
    call = functools.partial(graph_gatv2_aggregate, dl, dr, datt, rowptr, negative_slope=0.2)
    got = call(bad, row0=0, num_targets=N)
    assert torch.equal(got, call(as_node0, row0=0, num_targets=N))
    assert not torch.equal(got, call(col, row0=0, num_targets=N))     # (the planted ids did change rows)
    ids = torch.tensor([3, N, 7, -1, N + 100, 8, 1 << 40, gg.ISOLATED], device="cuda")
    inside = (ids >= 0) & (ids < N)
    out = call(bad, target_ids=ids)
    assert torch.equal(out[~inside], torch.zeros_like(out[~inside]))
    assert torch.equal(out[inside], got[ids[inside]])


def test_an_entry_outside_the_graph_is_skipped_in_node_zeros_own_row():
    """node 0 in EVERY respect: in target 0's row such an entry equals t and is dropped"""
    from salient_plusplus_amd.inference import graph_gatv2_aggregate
    g = torch.Generator().manual_seed(4)
    x = torch.randn((8, 16), generator=g).cuda()
    att = torch.randn((4, 4), generator=g).cuda()
    rowptr = torch.tensor([0, 3, 3, 3, 3, 3, 3, 3, 3]).cuda()
    call = functools.partial(graph_gatv2_aggregate, x, x, att, row0=0, num_targets=8)
    got = call(rowptr, torch.tensor([99, 5, -1]).cuda())
    assert torch.equal(got, call(rowptr, torch.tensor([0, 5, 0]).cuda()))
    assert torch.equal(got, call(torch.tensor([0, 1, 1, 1, 1, 1, 1, 1, 1]).cuda(), torch.tensor([5]).cuda()))


def test_refusals_on_device_tensors():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd.inference import graph_gatv2_aggregate as agg, graph_gatv2_workspace_bytes
    _hop, rowptr, col = _graph()
    _xl, _xr, _att, dl, dr, datt = _case("model", 4, 16, torch.float32, False)
    slab = dict(row0=0, num_targets=N)
    with pytest.raises(ValueError, match="1, 2, 4 or 8"):
        agg(dl[:, :48], dr[:, :48], datt[:3].contiguous(), rowptr, col, **slab)
    with pytest.raises(ValueError, match="power of two"):
        agg(dl[:, :48], dr[:, :48], torch.zeros((4, 12), device="cuda"), rowptr, col, **slab)
    with pytest.raises(ValueError, match="aligned to 4 elements"):
        agg(torch.zeros((N, 65), device="cuda")[:, 1:], torch.zeros((N, 64), device="cuda"), datt, rowptr, col, **slab)
    with pytest.raises(ValueError, match="x_r must have x_l's shape"):
        agg(dl, dr.bfloat16(), datt, rowptr, col, **slab)
    with pytest.raises(ValueError, match="must live on one CUDA device"):
        agg(dl, dr, datt.cpu(), rowptr, col, **slab)
    with pytest.raises(ValueError, match="workspace"):
        agg(dl, dr, datt, rowptr, col, workspace=torch.empty(graph_gatv2_workspace_bytes(N) - 8, dtype=torch.uint8,
                                                             device="cuda"), **slab)
    with pytest.raises(ValueError, match="aligned to 4 elements"):
        agg(dl, dr, datt, rowptr, col, out=torch.zeros((N, 66), device="cuda")[:, 1:65], **slab)
    # the entry itself, past the wrapper: a workspace that is too small is refused before anything is enqueued
    from salient_plusplus_amd.inference import _gatv2_launch
    with pytest.raises(nat.SppError, match="workspace"):
        _gatv2_launch(dl, dr, datt, rowptr, col, 0.2, False, 0, None, N, torch.empty((N, 64), device="cuda"),
                      torch.empty(64, dtype=torch.uint8, device="cuda"))
    assert agg(dl, dr, datt, rowptr, col, row0=5, num_targets=0).shape == (0, 64)
