"""spp_graph_transformer_forward (inference.graph_transformer_aggregate; csrc/graph_transformer.hip, spp.h f3z) on the
planted graph of tests/graph_transformer_f64.py: every element against the float64 restatement within its first-order
bound (bare and with the skip / ReLU / bf16 epilogue), the short rows bit for bit against spp_transformer_forward, the
long kernel's merge to the bit on a doubled chunk, the epilogue and the aliased skip to the bit, a row's bits against
slabs, lists and repeated calls, ids that leave the graph, and the refusals on device tensors.  The bounds come from
the arithmetic (graph_transformer_f64.py), never from what the kernel gives; every test prints the largest err / bound
it saw (DESIGN section 7 f3z records them)."""
import functools

import pytest
import torch

import graph_transformer_f64 as gt
import transformer_f64 as tf

pytestmark = pytest.mark.gpu

# <NQ, CPH> = <1,1> three times (1, 16 and 16 lanes a row), <4,1>, <2,1>, <2,2>, <4,2>; FAMILIES adds <4,4>
SHAPES = [(1, 4), (4, 16), (8, 8), (8, 128), (2, 256), (1, 512), (2, 512)]
FAMILIES = [(4, 16), (2, 256), (1, 512), (8, 128), (2, 512), (1, 1024)]
ROW_DTYPES = [torch.float32, torch.bfloat16]
N = gt.N


def _name(d):
    return str(d).split(".")[-1]


@functools.lru_cache(maxsize=None)
def _cg():
    from salient_plusplus_amd.inference import graph_transformer_chunk
    return graph_transformer_chunk()


@functools.lru_cache(maxsize=None)
def _graph(D):
    """the planted graph with the hub of width D, its rowptr and the col the KERNEL gets (one entry outside the graph)"""
    ent = gt.planted_graph(_cg(), gt.hub_length(D, _cg()))
    return ent, ent.rowptr.cuda(), ent.col_raw.cuda()


@functools.lru_cache(maxsize=4)
def _case(regime, H, Cc, dtype):
    """CPU inputs [N, H, C] (DOUBLED asks with CHUNK's q) and CUDA copies [N, H * C]: q, k, v apart, [k | v] as one
    matrix, skip"""
    ent = _graph(H * Cc)[0]
    q, k, v, skip = gt.inputs(regime, ent, H, Cc, dtype)
    q[gt.DOUBLED] = q[gt.CHUNK]
    flat = lambda t: t.reshape(N, H * Cc).cuda()
    kv = torch.cat([flat(k), flat(v)], 1)
    return (q, k, v, skip), (flat(q), flat(k), flat(v), kv, flat(skip))


def _run(regime, H, Cc, dtype, fused_kv=False, skip=False, **kw):
    from salient_plusplus_amd.inference import graph_transformer_aggregate
    _ent, rowptr, col = _graph(H * Cc)
    dq, dk, dv, kv, dskip = _case(regime, H, Cc, dtype)[1]
    if fused_kv:
        dk, dv = kv[:, :H * Cc], kv[:, H * Cc:]
    if not any(k in kw for k in ("row0", "target_ids")):
        kw.update(row0=0, num_targets=N)
    return graph_transformer_aggregate(dq, dk, dv, rowptr, col, heads=H, scale=tf.scale32(Cc),
                                       skip=dskip if skip else None, **kw)


@pytest.mark.parametrize("dtype", ROW_DTYPES, ids=_name)
@pytest.mark.parametrize("H,Cc", SHAPES)
def test_every_element_is_within_its_float64_bound(H, Cc, dtype):
    """f3y's six regimes and the two whose logits rise / fall from chunk to chunk; per regime the bare fp32 call with k
    and v apart, and the call with skip, ReLU and bf16 output on [k | v] as one matrix"""
    ent = _graph(H * Cc)[0]
    scale = tf.scale32(Cc)
    top, top_tail = (0.0, ""), (0.0, "")
    for regime in gt.REGIMES:
        q, k, v, skip = _case(regime, H, Cc, dtype)[0]
        ref = gt.reference(ent, q, k, v, scale, _cg())
        got = _run(regime, H, Cc, dtype).view(N, H, Cc)
        ratio, where = tf.worst(got, ref.out, ref.b_out)
        top = max(top, (ratio, f"{regime}: {where}"))
        assert ratio <= 1.0, (regime, where)
        ref = gt.reference(ent, q, k, v, scale, _cg(), skip=skip, relu=True)
        got = _run(regime, H, Cc, dtype, fused_kv=True, skip=True, relu=True, out_dtype=torch.bfloat16)
        assert got.dtype == torch.bfloat16
        ratio, where = tf.worst(got.view(N, H, Cc), ref.out, gt.widen_bf16(ref.out, ref.b_out))
        top_tail = max(top_tail, (ratio, f"{regime}: {where}"))
        assert ratio <= 1.0, ("skip, relu, bf16 out", regime, where)
    print(f"GRAPH_TRANSFORMER H={H} C={Cc} rows={_name(dtype)}: largest err / bound {top[0]:.3f} ({top[1]}); "
          f"skip + relu + bf16 output {top_tail[0]:.3f} ({top_tail[1]})")


@pytest.mark.parametrize("dtype", ROW_DTYPES + [torch.float16], ids=_name)
@pytest.mark.parametrize("H,Cc", FAMILIES)
def test_short_rows_are_the_bits_of_the_training_forward(H, Cc, dtype):
    """rows of at most C_g entries, fp32 output, no skip, relu = 0: spp_transformer_forward over the whole graph as one
    hop (T = S = N) runs the same body (csrc/transformer_core.hip.h); it takes ids as they are, so it gets the col with
    the entry outside the graph already written as node 0"""
    from salient_plusplus_amd.models import _TransformerLayer
    ent, rowptr, _col = _graph(H * Cc)
    short = (ent.raw <= _cg()).cuda()
    assert int(short.sum()) > 600 and int((~short).sum()) >= 4
    clean = ent.col.cuda()
    for regime in ("model", "wide", "zero"):
        dq, dk, dv, kv, _s = _case(regime, H, Cc, dtype)[1]
        want = _TransformerLayer.apply(dq, dk, dv, rowptr, clean, H, tf.scale32(Cc)).reshape(N, H * Cc)
        for fused in (False, True):
            got = _run(regime, H, Cc, dtype, fused_kv=fused)
            assert torch.equal(got[short].view(torch.int32), want[short].view(torch.int32)), (regime, fused)


@pytest.mark.parametrize("dtype", ROW_DTYPES + [torch.float16], ids=_name)
@pytest.mark.parametrize("H,Cc", FAMILIES + [(1, 4)])
def test_the_doubled_chunk_is_the_bits_of_its_chunk(H, Cc, dtype):
    """the long kernel and the merge to the bit: row DOUBLED is row CHUNK (C_g entries, a short row) written twice and
    asks with the same q.  Both chunk states are equal, so m' = m, f1 = f2 = expf(0) = 1, s' = fma(s, 1, s * 1) = 2 s and
    acc' = 2 acc exactly, 1 / (2 s) is exactly half of 1 / s, and the products acc' * (1 / s') are the short row's."""
    for regime in ("model", "wide", "rising"):
        got = _run(regime, H, Cc, dtype, target_ids=torch.tensor([gt.DOUBLED, gt.CHUNK], device="cuda"))
        assert bool(got[1].abs().sum() > 0) and torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), regime


@pytest.mark.parametrize("dtype", ROW_DTYPES, ids=_name)
@pytest.mark.parametrize("H,Cc", [(4, 16), (8, 128), (1, 512)])
def test_the_epilogue_is_skip_then_relu_then_one_rounding(H, Cc, dtype):
    ent = _graph(H * Cc)[0]
    dskip = _case("model", H, Cc, dtype)[1][4]
    plain = _run("model", H, Cc, dtype)
    assert plain.dtype == torch.float32
    empty = torch.tensor([gt.EMPTY, gt.ISOLATED], device="cuda")
    assert torch.equal(plain[empty], torch.zeros_like(plain[empty]))
    with_skip = plain + dskip.float()                          # one rounded fp32 addition per column
    for relu in (False, True):
        want = torch.relu(with_skip) if relu else with_skip
        for out_dtype in (torch.float32, torch.bfloat16):
            got = _run("model", H, Cc, dtype, skip=True, relu=relu, out_dtype=out_dtype)
            assert torch.equal(got, want.to(out_dtype)), (relu, out_dtype)
            assert torch.equal(got[empty], (torch.relu(dskip[empty].float()) if relu else dskip[empty].float()).to(out_dtype))
    assert bool((with_skip < 0).any()) and int(ent.raw[gt.HUB]) > 2 * _cg()
    assert torch.equal(_run("model", H, Cc, dtype, relu=True), torch.relu(plain))


@pytest.mark.parametrize("dtype", ROW_DTYPES, ids=_name)
@pytest.mark.parametrize("H,Cc", [(4, 16), (8, 128), (1, 4)])
def test_a_skip_that_is_the_output_matrix_changes_no_bit(H, Cc, dtype):
    """skip aliases out (same element type; the skip row of target t and output row i are the same addresses): a lane
    reads its columns before it writes them.  Slab by slab over the one matrix, long rows included."""
    from salient_plusplus_amd.inference import graph_transformer_aggregate
    _ent, rowptr, col = _graph(H * Cc)
    dq, dk, dv, _kv, dskip = _case("model", H, Cc, dtype)[1]
    want = _run("model", H, Cc, dtype, skip=True, relu=True, out_dtype=dtype)
    for rows in (N, 96):
        buf = dskip.clone()
        for s in range(0, N, rows):
            T = min(rows, N - s)
            graph_transformer_aggregate(dq, dk, dv, rowptr, col, heads=H, scale=tf.scale32(Cc), skip=buf, relu=True, row0=s,
                                        num_targets=T, out_dtype=dtype, out=buf[s:s + T])
        assert torch.equal(buf, want), rows


@pytest.mark.parametrize("H,Cc,dtype", [(4, 16, torch.float32), (8, 128, torch.bfloat16), (1, 4, torch.float32),
                                        (2, 256, torch.bfloat16), (1, 1024, torch.float32)])
def test_a_rows_bits_depend_on_the_row_alone(H, Cc, dtype):
    from salient_plusplus_amd.inference import graph_transformer_workspace_bytes
    ent = _graph(H * Cc)[0]
    call = functools.partial(_run, "model", H, Cc, dtype, skip=True, relu=True)
    whole = call()
    for rows in (64, 1000, 1 << 20):
        parts = [call(row0=s, num_targets=min(rows, N - s)) for s in range(0, N, rows)]
        assert torch.equal(torch.cat(parts), whole), rows
    assert torch.equal(call(target_ids=torch.arange(N, device="cuda")), whole)
    g = torch.Generator().manual_seed(2)
    ids = torch.cat([torch.randperm(N, generator=g)[:90], torch.tensor(ent.planted + [gt.HUB, gt.MID, gt.HUB, gt.DOUBLED])])
    ids = ids[torch.randperm(ids.numel(), generator=g)].cuda()
    assert torch.equal(call(target_ids=ids), whole[ids])
    ws = torch.empty(graph_transformer_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    first, second = call(workspace=ws), call(workspace=ws)
    assert torch.equal(first, second) and torch.equal(first, whole)
    assert torch.equal(call(target_ids=ids, workspace=ws), whole[ids])
    out = torch.full((N + 2, H * Cc + 4), 7.0, device="cuda")         # rows of a larger matrix; the rest is not touched
    call(out=out[1:N + 1, :H * Cc])
    assert torch.equal(out[1:N + 1, :H * Cc], whole) and bool((out[:, H * Cc:] == 7).all()) and bool((out[0] == 7).all())


@pytest.mark.parametrize("H,Cc", [(4, 16), (8, 128)])
def test_ids_that_leave_the_graph(H, Cc):
    """what the contract defines and nothing beyond it: an entry outside [0, N) reads node 0, a target outside gives
    zeros and no skip"""
    from salient_plusplus_amd.inference import graph_transformer_aggregate
    ent, rowptr, col = _graph(H * Cc)
    Cg = _cg()
    dq, dk, dv, _kv, dskip = _case("model", H, Cc, torch.float32)[1]
    bad = col.clone()
    for t, k, j in ((gt.REPEATS, 1, N), (30, 0, -3), (gt.MID, 5, N + 5), (gt.MID, Cg + 3, 1 << 40), (gt.HUB, 2 * Cg + 1, -1),
                    (gt.ONE, 0, N), (gt.DOUBLED, Cg + 2, N + 1)):
        if int(ent.raw[t]) > k:
            bad[rowptr[t] + k] = j
    as_node0 = torch.where((bad >= 0) & (bad < N), bad, torch.zeros_like(bad))
    call = functools.partial(graph_transformer_aggregate, dq, dk, dv, rowptr, heads=H, scale=tf.scale32(Cc), skip=dskip)
    got = call(bad, row0=0, num_targets=N)
    assert torch.equal(got, call(as_node0, row0=0, num_targets=N))
    assert not torch.equal(got, call(ent.col.cuda(), row0=0, num_targets=N))     # (the planted ids did change rows)
    ids = torch.tensor([3, N, gt.MID, -1, N + 100, gt.HUB, 1 << 40, gt.ISOLATED], device="cuda")
    inside = (ids >= 0) & (ids < N)
    out = call(bad, target_ids=ids)
    assert torch.equal(out[~inside], torch.zeros_like(out[~inside]))
    assert torch.equal(out[inside], got[ids[inside]]) and torch.equal(out[-1], dskip[gt.ISOLATED])


def test_refusals_on_device_tensors():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd.inference import _transformer_launch, graph_transformer_aggregate as agg, \
        graph_transformer_workspace_bytes
    _ent, rowptr, col = _graph(64)
    dq, dk, dv, _kv, dskip = _case("model", 4, 16, torch.float32)[1]
    kw = dict(heads=4, scale=0.25, row0=0, num_targets=N)
    with pytest.raises(ValueError, match="1, 2, 4 or 8"):
        agg(dq[:, :48], dk[:, :48], dv[:, :48], rowptr, col, **dict(kw, heads=3))
    with pytest.raises(ValueError, match="power of two"):
        agg(dq[:, :48], dk[:, :48], dv[:, :48], rowptr, col, **kw)
    with pytest.raises(ValueError, match="aligned to 4 elements"):
        agg(torch.zeros((N, 65), device="cuda")[:, 1:], dk, dv, rowptr, col, **kw)
    with pytest.raises(ValueError, match="v must have q's shape and dtype"):
        agg(dq, dk, dv.bfloat16(), rowptr, col, **kw)
    with pytest.raises(ValueError, match="must live on one CUDA device"):
        agg(dq, dk, dv, rowptr, col, skip=dskip.cpu(), **kw)
    with pytest.raises(ValueError, match="scale"):
        agg(dq, dk, dv, rowptr, col, **dict(kw, scale=0.0))
    with pytest.raises(ValueError, match="workspace"):
        agg(dq, dk, dv, rowptr, col, workspace=torch.empty(graph_transformer_workspace_bytes(N) - 8, dtype=torch.uint8,
                                                            device="cuda"), **kw)
    with pytest.raises(ValueError, match="aligned to 4 elements"):
        agg(dq, dk, dv, rowptr, col, out=torch.zeros((N, 66), device="cuda")[:, 1:65], **kw)
    # the entry itself, past the wrapper, in the header's order: the workspace before the rows, the rows before the scale
    out, ws = torch.full((N, 64), 7.0, device="cuda"), torch.empty(graph_transformer_workspace_bytes(N), dtype=torch.uint8,
                                                                  device="cuda")
    launch = lambda q, scale, T, w: _transformer_launch(q, dk, dv, None, 4, scale, rowptr, col, False, 0, None, T, out, w)
    with pytest.raises(nat.SppError, match="workspace"):
        launch(torch.zeros((N, 66), device="cuda")[:, 1:65], 0.0, N, ws[:64])
    with pytest.raises(nat.SppError, match="misaligned"):
        launch(torch.zeros((N, 66), device="cuda")[:, 1:65], 0.0, N, ws)
    with pytest.raises(nat.SppError, match="scale"):
        launch(dq, 0.0, N, ws)
    launch(dq, 0.0, 0, ws)                                     # num_targets == 0: SPP_OK, and nothing is touched
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert agg(dq, dk, dv, rowptr, col, heads=4, scale=0.25, row0=5, num_targets=0).shape == (0, 64)
