"""The attention driver of ``inference`` against its own documentation: one whole ``layerwise_inference`` pass of GAT and
of GATv2 restated as the sequence of public calls the driver's docstrings give -- ``_row_tiles``, the projections in
``act_dtype``, GAT's fp32 logits from the layer's input rows, ``graph_gat_aggregate`` / ``graph_gatv2_aggregate`` with
``relu=`` on the hidden layers, the mean of the last layer's heads, ``log_softmax(dtype=torch.float32)`` -- and compared
with ``torch.equal``.  No tolerance: the restatement runs the same GEMM shapes and the same kernels, and a row's bits
depend on the row alone, so whatever the driver does between those calls (slabs, padded copies, which matrix a slab is
written into, what it frees and when) may not change one bit.

The graphs, features and models are the ones the two inference test files build (400 and 600 nodes, a node of degree
0, diagonal entries, hub rows longer than the kernels' chunk).  Every pass of the restatement is computed once."""
import functools

import pytest
import torch

import test_gpu_gat_inference as gat_case
import test_gpu_gatv2_inference as gatv2_case

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
GAT_CASES = [(1, 3, 16), (4, 2, 16)]                     # heads, layers, hidden
GATV2_CASES = [(4, 5, False), (1, 8, True)]              # heads, classes, share_weights: Cp = 8 != 5 padded; shared, unpadded
SLAB = 96                                                # below both N and no divisor of either: several slabs, a short last one


def _name(d):
    return str(d).split(".")[-1]


def _project(cur, Wt, act_dtype):
    """cur @ W^T over the fixed row tiles, in ``act_dtype``"""
    from salient_plusplus_amd.inference import _row_tiles
    out = torch.empty((cur.size(0), Wt.size(1)), dtype=act_dtype, device=cur.device)
    for r, n, tile in _row_tiles(cur):
        out[r:r + n] = (tile.to(act_dtype) @ Wt)[:n]
    return out


def _targets(last, nodes, n):
    """the last layer's targets are ``nodes`` when given; every other layer computes all rows"""
    if last and nodes is not None:
        return dict(target_ids=nodes)
    return dict(row0=0, num_targets=n)


def _gat_pass(model, x, rowptr, col, act_dtype, nodes=None):
    from salient_plusplus_amd.inference import _row_tiles, graph_gat_aggregate
    n_layers, cur = len(model.convs), x
    with torch.no_grad():
        for i, conv in enumerate(model.convs):
            last = i == n_layers - 1
            H, Cc = conv.heads, conv.out_channels
            W = conv.lin_src.weight
            att = torch.stack([conv.att_src.view(H, Cc), conv.att_dst.view(H, Cc)]).to(torch.float32)
            V = torch.einsum("shc,hck->shk", att, W.to(torch.float32).view(H, Cc, -1)).reshape(2 * H, -1)
            Vt = V.t().contiguous()
            h = _project(cur, W.to(act_dtype).t(), act_dtype)
            a_src, a_dst = (torch.empty((cur.size(0), H), dtype=torch.float32, device=x.device) for _ in range(2))
            for r, n, tile in _row_tiles(cur):           # the logits come from the INPUT rows in fp32, never from h
                a = tile.to(torch.float32) @ Vt
                a_src[r:r + n], a_dst[r:r + n] = a[:n, :H], a[:n, H:]
            out = graph_gat_aggregate(h, a_src, a_dst, rowptr, col, heads=H, negative_slope=conv.negative_slope,
                                      relu=not last, out_dtype=torch.float32 if last else act_dtype,
                                      **_targets(last, nodes, cur.size(0)))
            cur = out
        logits = cur.view(cur.size(0), H, Cc).mean(1) if H > 1 else cur
        return torch.log_softmax(logits, dim=-1, dtype=torch.float32)


def _gatv2_pass(model, x, rowptr, col, act_dtype, nodes=None):
    from salient_plusplus_amd.inference import _gatv2_pad, graph_gatv2_aggregate
    n_layers, cur = len(model.convs), x
    with torch.no_grad():
        for i, conv in enumerate(model.convs):
            last = i == n_layers - 1
            H, Cc = conv.heads, conv.out_channels
            Cp = _gatv2_pad(Cc)

            def padded_t(W):                             # zero rows behind each head's C channels, then W^T in act_dtype
                if Cp != Cc:
                    Wp = W.new_zeros((H, Cp, W.size(1)))
                    Wp[:, :Cc] = W.view(H, Cc, -1)
                    W = Wp.view(H * Cp, -1)
                return W.to(act_dtype).t()
            att = torch.zeros((H, Cp), dtype=torch.float32, device=x.device)
            att[:, :Cc] = conv.att.view(H, Cc)
            x_l = _project(cur, padded_t(conv.lin_l.weight), act_dtype)
            x_r = x_l if conv.lin_r is conv.lin_l else _project(cur, padded_t(conv.lin_r.weight), act_dtype)
            out = graph_gatv2_aggregate(x_l, x_r, att, rowptr, col, negative_slope=conv.negative_slope, relu=not last,
                                        out_dtype=torch.float32 if last else act_dtype,
                                        **_targets(last, nodes, cur.size(0)))
            out = out.view(out.size(0), H, Cp)[:, :, :Cc]           # the padded channels are sliced away
            cur = out.reshape(out.size(0), H * Cc)
        logits = out.mean(1) if H > 1 else cur
        return torch.log_softmax(logits, dim=-1, dtype=torch.float32)


def _nodes(n, planted):
    g = torch.Generator().manual_seed(1)
    return torch.cat([torch.randperm(n, generator=g)[:70], torch.tensor(planted)])     # (``planted`` holds a duplicate)


@functools.lru_cache(maxsize=None)
def _gat(heads, layers, hidden, act_dtype):
    """(model, graph, features, nodes, the restated pass over all nodes, the restated pass over ``nodes``)"""
    rowptr, col = gat_case._graph()
    x = gat_case._features()
    model = gat_case._model(heads, layers, hidden)
    nodes = _nodes(gat_case.N, [gat_case.N - 1, 300, 300, 0, 11, gat_case.EMPTY_CHUNK_ROW, gat_case.DEG0]).cuda()
    return (model, x, rowptr, col, nodes, _gat_pass(model, x, rowptr, col, act_dtype),
            _gat_pass(model, x, rowptr, col, act_dtype, nodes))


@functools.lru_cache(maxsize=None)
def _gatv2(H, classes, share, act_dtype):
    rowptr, col = gatv2_case._graph()
    x = gatv2_case._features()
    model = gatv2_case._model(H, classes, share)
    nodes = _nodes(gatv2_case.N, [gatv2_case.N - 1, gatv2_case.HUB, gatv2_case.HUB, 0, 3, gatv2_case.HUB]).cuda()
    return (model, x, rowptr, col, nodes, _gatv2_pass(model, x, rowptr, col, act_dtype),
            _gatv2_pass(model, x, rowptr, col, act_dtype, nodes))


def _assert_the_driver_returns_the_restated_bits(case, act_dtype):
    from salient_plusplus_amd.inference import layerwise_inference
    model, x, rowptr, col, nodes, want, want_nodes = case
    assert want.dtype == torch.float32 and bool(torch.isfinite(want).all())
    assert torch.equal(want_nodes, want[nodes])          # the restatement itself: a row's bits depend on the row alone
    for rows in (1 << 20, SLAB):
        got = layerwise_inference(model, x, rowptr, col, rows_per_slab=rows, act_dtype=act_dtype)
        assert got.shape == want.shape and torch.equal(got, want), rows
    for rows in (1 << 20, 32):                           # (77 nodes: three slabs of 32)
        got = layerwise_inference(model, x, rowptr, col, nodes=nodes, rows_per_slab=rows, act_dtype=act_dtype)
        assert got.shape == want_nodes.shape and torch.equal(got, want_nodes), rows


@pytest.mark.parametrize("act_dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("heads,layers,hidden", GAT_CASES)
def test_gat_pass_is_the_documented_sequence_of_public_calls(heads, layers, hidden, act_dtype):
    _assert_the_driver_returns_the_restated_bits(_gat(heads, layers, hidden, act_dtype), act_dtype)


@pytest.mark.parametrize("act_dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("H,classes,share", GATV2_CASES)
def test_gatv2_pass_is_the_documented_sequence_of_public_calls(H, classes, share, act_dtype):
    _assert_the_driver_returns_the_restated_bits(_gatv2(H, classes, share, act_dtype), act_dtype)
