"""-m gpu: spp_graph_agg_parts_forward (inference.graph_aggregate_parts) against spp_graph_agg_forward
(inference.graph_aggregate) on the concatenation of the parts, bit for bit: the contract says the partitioned result IS
the unpartitioned one, so there is no tolerance.

The graph (about 3 000 nodes): degrees 0, 1, C and C + 1, random rows between them, one ``col`` entry outside the graph,
and one hub whose row spans every part and needs more than two rounds of k_graph_agg_long at the width under test (2.5
times C * 256 / lpr entries: 40 997 at F = 4, 677 at F = 256).  The parts are separate allocations made in shuffled order with
a padded row stride and different contents, so that a wrong owner or a wrong local row reads wrong data."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3001
PARTS = [1, 2, 3, 8, 16]
WIDTHS = [4, 100, 128, 130, 256]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _graph(hub_entries):
    """(rowptr, col) on the GPU; node 7 is the hub, nodes 0..3 have the degrees 0, 1, C, C + 1"""
    from salient_plusplus_amd.inference import graph_agg_chunk
    Cc = graph_agg_chunk()
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(0, 20, (N,), generator=g)
    deg[0], deg[1], deg[2], deg[3] = 0, 1, Cc, Cc + 1
    deg[N - 1] = Cc + 1                                        # (the last node of the last part is a long row too)
    deg[7] = hub_entries
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    k = min(N, hub_entries)                                    # the hub reads rows of every part
    col[int(rowptr[7]):int(rowptr[7]) + k] = torch.randperm(N, generator=g)[:k]
    col[int(rowptr[2]) + 5] = N + 12                           # outside the graph: global row 0
    col[int(rowptr[7]) + 70] = -3
    return rowptr.cuda(), col.cuda()


def _hub_entries(F):
    """two and a half times C * 256 / lpr entries (lpr = lanes per row; the vector form has F / 4 pieces per row): more
    than two rounds of the long-row kernel -- 40 997 entries at F = 4, 677 at F = 256"""
    from salient_plusplus_amd.inference import graph_agg_chunk
    pieces = F // 4 if F % 4 == 0 else F
    lpr = 1
    while lpr < pieces and lpr < 64:
        lpr *= 2
    return graph_agg_chunk() * 256 // lpr * 5 // 2 + 37


def _offsets(P):
    """P = 2: a one-row first part.  P >= 3: an EMPTY first part and a one-row last part; P >= 5: an empty part in the
    middle as well; the cuts between them are uneven"""
    if P == 1:
        return [0, N]
    if P == 2:
        return [0, 1, N]
    g = torch.Generator().manual_seed(P)
    cuts = sorted(torch.randperm(N - 80, generator=g)[:max(P - 4, 0)].add(40).tolist())
    if P >= 4:
        cuts.insert(len(cuts) // 2, cuts[len(cuts) // 2] if cuts else 1500)
    off = [0, 0] + cuts + [N - 1, N]
    assert len(off) == P + 1 and off == sorted(off)
    return off


def _split(x, off, stride, misalign=None):
    """the rows of x as separate allocations, made in shuffled order, rows ``stride`` elements apart; ``misalign``: that
    part's base is moved one element off the vector form's alignment"""
    P = len(off) - 1
    parts = [None] * P
    for p in torch.randperm(P, generator=torch.Generator().manual_seed(3)).tolist():
        rows = off[p + 1] - off[p]
        if rows == 0:
            parts[p] = None if p % 2 else x[:0]
            continue
        buf = torch.full((rows * stride + 8,), float("nan"), dtype=x.dtype, device=x.device)
        skew = 1 if p == misalign else 0
        view = buf[skew:skew + rows * stride].view(rows, stride)[:, :x.size(1)]
        view.copy_(x[off[p]:off[p + 1]])
        parts[p] = view
    return parts


def _x(F, dtype, stride):
    g = torch.Generator().manual_seed(F)
    full = torch.zeros((N, stride), dtype=dtype)
    full[:, :F] = torch.randn((N, F), generator=g).to(dtype)
    return full.cuda()[:, :F]


def _targets():
    """a slab that crosses part boundaries and an id list with duplicates, the hub and out-of-graph ids"""
    ids = torch.tensor([7, 2, 2, N - 1, N, -1, 0, 3, 7, 1500, 1, N + 40, 2999], dtype=torch.int64).cuda()
    return [dict(row0=0, num_targets=N), dict(row0=5, num_targets=N - 900), dict(target_ids=ids)]


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("P", PARTS)
def test_parts_equal_the_concatenation_bit_for_bit(P, F):
    from salient_plusplus_amd.inference import graph_aggregate, graph_aggregate_parts
    rowptr, col = _graph(_hub_entries(F))
    stride = F + 4 if F % 4 == 0 else F + 3                    # padded (and, for F = 130, odd: the scalar form)
    x = _x(F, torch.float16, stride)
    off = _offsets(P)
    parts = _split(x, off, stride)
    epilogue, scale = [("mean", 0.0), ("operand", 0.0), ("sum", 1.25)][(P + F) % 3]
    for tgt in _targets():
        want = graph_aggregate(x, rowptr, col, epilogue=epilogue, self_scale=scale, **tgt)
        got = graph_aggregate_parts(parts, off, rowptr, col, epilogue=epilogue, self_scale=scale, **tgt)
        assert _same(got, want), (P, F, epilogue, sorted(tgt))
    torch.cuda.synchronize()


@pytest.mark.parametrize("epilogue,scale", [("mean", 0.0), ("operand", 0.0), ("sum", 1.25)])
@pytest.mark.parametrize("x_dtype,out_dtype", [(torch.float16, torch.bfloat16), (torch.float32, torch.float32),
                                               (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32),
                                               (torch.bfloat16, torch.bfloat16)])
def test_element_types_and_epilogues(x_dtype, out_dtype, epilogue, scale):
    from salient_plusplus_amd.inference import graph_aggregate, graph_aggregate_parts
    F, P = 128, 3
    rowptr, col = _graph(_hub_entries(F))
    x = _x(F, x_dtype, F + 4)
    off = _offsets(P)
    parts = _split(x, off, F + 4)
    for tgt in _targets():
        want = graph_aggregate(x, rowptr, col, epilogue=epilogue, self_scale=scale, out_dtype=out_dtype, **tgt)
        got = graph_aggregate_parts(parts, off, rowptr, col, epilogue=epilogue, self_scale=scale, out_dtype=out_dtype,
                                    **tgt)
        assert _same(got, want), (x_dtype, out_dtype, epilogue, sorted(tgt))


def test_one_misaligned_part_takes_the_scalar_form_with_the_same_bits():
    """F = 128 and a stride of 132 allow four columns per lane, but one part's base sits one element off: the whole call
    reads one column per lane, and nothing changes in the result"""
    from salient_plusplus_amd.inference import graph_aggregate, graph_aggregate_parts
    F, P = 128, 8
    rowptr, col = _graph(_hub_entries(F))
    x = _x(F, torch.float16, F + 4)
    off = _offsets(P)
    live = [p for p in range(P) if off[p + 1] - off[p] > 1]
    parts = _split(x, off, F + 4, misalign=live[-1])
    assert parts[live[-1]].data_ptr() % 8 == 2 and all(parts[p].data_ptr() % 8 == 0 for p in live[:-1])
    for epilogue, scale in (("operand", 0.0), ("sum", 0.5)):
        for tgt in _targets():
            want = graph_aggregate(x, rowptr, col, epilogue=epilogue, self_scale=scale, **tgt)
            assert _same(graph_aggregate_parts(parts, off, rowptr, col, epilogue=epilogue, self_scale=scale, **tgt), want)


def test_out_argument_peer_addresses_and_the_old_entry_around_the_new_one():
    """``out=`` rows of a larger matrix; the P2PPeers form (addresses, dtype=, F=); and spp_graph_agg_forward called
    before and after the new entry gives the same bits (the two share their kernels' template and the workspace)"""
    from salient_plusplus_amd.fast_sampler import P2PPeers
    from salient_plusplus_amd.inference import graph_agg_workspace_bytes, graph_aggregate, graph_aggregate_parts
    F, P = 100, 8
    rowptr, col = _graph(_hub_entries(F))
    x = _x(F, torch.float16, 104)
    off = _offsets(P)
    parts = _split(x, off, 104)
    ws = torch.empty(graph_agg_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    tgt = dict(row0=0, num_targets=N)
    before = graph_aggregate(x, rowptr, col, epilogue="operand", workspace=ws, **tgt)
    big = torch.full((N + 2, 2 * F + 8), 7.0, device="cuda")
    out = big[1:N + 1, 4:2 * F + 4]
    got = graph_aggregate_parts(parts, off, rowptr, col, epilogue="operand", workspace=ws, out=out, **tgt)
    after = graph_aggregate(x, rowptr, col, epilogue="operand", workspace=ws, **tgt)
    assert got.data_ptr() == out.data_ptr() and _same(out.contiguous(), before) and _same(after, before)
    assert bool((big[0] == 7).all() and (big[-1] == 7).all() and (big[:, :4] == 7).all() and (big[:, -4:] == 7).all())
    peers = P2PPeers([t.data_ptr() if t is not None and t.numel() else 0 for t in parts], 104 * 2, keep=parts)
    again = graph_aggregate_parts(peers, off, rowptr, col, dtype=torch.float16, F=F, epilogue="operand", workspace=ws,
                                  **tgt)
    assert _same(again, before)
