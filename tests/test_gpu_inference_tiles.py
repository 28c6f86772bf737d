"""-m gpu: the inference drivers across a GEMM tile boundary.  Every other test graph has fewer rows than one fixed GEMM
tile (65 536), so the drivers' row arithmetic over several tiles of a slab (first row of the slab + first row of the tile)
runs only here: a graph of 65 536 + 703 nodes, two-layer SAGE, GAT with two heads and SAGEResInception in bf16.  One
result, bit for bit, whatever the slab size (two tiles a slab, one tile a slab, padded tiles only), for ``nodes`` on both
sides of row 65 536, and for two ranks of a partitioned table of which rank 0 owns one full tile and a one-row tile."""
import functools
import os
import sys
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TILE = 1 << 16
N, FIN, HID, CLASSES = TILE + 703, 8, 16, 5
OFFSETS = [0, TILE + 1, N]
KINDS = ["sage", "gat", "resinc"]
ACT = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _graph():
    """65 536 + 703 nodes, degrees 0..6 and one row longer than both kernels' chunks; fp16 features"""
    from salient_plusplus_amd.inference import graph_agg_chunk, graph_gat_chunk
    g = torch.Generator().manual_seed(17)
    deg = torch.randint(0, 7, (N,), generator=g)
    deg[TILE - 2] = max(graph_agg_chunk(), graph_gat_chunk()) + 9
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    x = torch.randn((N, FIN), generator=g).to(torch.float16)
    return x.cuda(), rowptr.cuda(), col.cuda()


@functools.lru_cache(maxsize=None)
def _model(kind):
    from salient_plusplus_amd.models import GAT, SAGE, SAGEResInception
    torch.manual_seed(23)
    if kind == "sage":
        return SAGE(FIN, HID, CLASSES, 2).cuda().eval()
    if kind == "gat":
        return GAT(FIN, HID, CLASSES, 2, heads=2).cuda().eval()
    m = SAGEResInception(FIN, HID, CLASSES, 2)
    g = torch.Generator().manual_seed(8)
    for mod in m.modules():                                    # non-trivial running statistics and affine terms
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.5)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 2.0 + 0.5)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _reference(kind):
    """all N rows with one slab: two tiles, one full and one padded; computed once and left unchanged"""
    from salient_plusplus_amd.inference import layerwise_inference
    x, rowptr, col = _graph()
    out = layerwise_inference(_model(kind), x, rowptr, col, rows_per_slab=1 << 20, act_dtype=ACT)
    assert out.shape == (N, CLASSES) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32),
                                                                                      b.view(torch.int32))


@pytest.mark.parametrize("rows_per_slab", [TILE, 40_000])      # one tile a slab (the last padded); padded tiles only
@pytest.mark.parametrize("kind", KINDS)
def test_the_slab_size_changes_no_bit(kind, rows_per_slab):
    from salient_plusplus_amd.inference import layerwise_inference
    x, rowptr, col = _graph()
    got = layerwise_inference(_model(kind), x, rowptr, col, rows_per_slab=rows_per_slab, act_dtype=ACT)
    assert _same_bits(got, _reference(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_nodes_on_both_sides_of_the_tile_boundary(kind):
    from salient_plusplus_amd.inference import layerwise_inference
    x, rowptr, col = _graph()
    g = torch.Generator().manual_seed(3)
    pick = torch.randint(0, N, (300,), generator=g)
    nodes = torch.cat([torch.tensor([TILE, N - 1, TILE - 1, 0, TILE - 2, TILE, TILE + 1]), pick, pick[:20]])
    assert bool((nodes < TILE).any()) and bool((nodes >= TILE).any())
    got = layerwise_inference(_model(kind), x, rowptr, col, nodes=nodes, act_dtype=ACT)
    assert _same_bits(got, _reference(kind)[nodes.cuda()])


def _partition(x, lo, hi):
    """rows [lo, hi) of x as a rank holds them: an allocation of its own, rows padded by the resident tables' rule"""
    from salient_plusplus_amd import fast_sampler as fs
    part = torch.empty((hi - lo, fs._row_stride_elems(x.size(1), x.element_size())), dtype=x.dtype,
                       device=x.device)[:, :x.size(1)]
    part.copy_(x[lo:hi])
    return part


@pytest.mark.parametrize("kind", KINDS)
def test_two_ranks_of_which_one_owns_a_full_tile_and_one_row(kind):
    from salient_plusplus_amd.inference import LocalPeers, partitioned_inference
    x, rowptr, col = _graph()
    want, model = _reference(kind), _model(kind)
    parts = [_partition(x, OFFSETS[r], OFFSETS[r + 1]) for r in range(2)]
    peers = LocalPeers(2, timeout=60.0)
    got, errors = [None, None], {}

    def run(r):
        try:
            torch.cuda.set_device(0)
            got[r] = partitioned_inference(model, parts[r], rowptr, col, part_offsets=OFFSETS, rank=r, peers=peers,
                                           act_dtype=ACT)
        except BaseException as e:  # noqa: BLE001
            errors[r] = e

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts), "rank(s) hung"
    assert not errors, errors
    for r in range(2):
        assert _same_bits(got[r], want[OFFSETS[r]:OFFSETS[r + 1]]), (kind, r)
