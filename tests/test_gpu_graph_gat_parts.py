"""-m gpu: inference.graph_gat_aggregate_parts (spp_graph_gat_parts_forward) against inference.graph_gat_aggregate on the
concatenated h and logits, bit for bit: the softmax contract fixes the order of every operation, so where a row and its
logit live changes nothing.  One graph of 600 nodes with rows on both sides of every chunk edge, self loops and ids
outside the graph; partitions with empty, one-row and sixteen parts; every element type, both lane forms, a part whose
rows are misaligned for the vector form; slabs and lists; dense and padded logits."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 600
HUBS = {11: 64, 12: 65, 299: 128, 300: 3 * 64 + 7, N - 1: 9 * 64}     # node -> raw row length (C_g = 64)
PARTITIONS = {
    "P1": [0, N],
    "P4-empty-first-one-row": [0, 0, 1, 300, N],               # global node 0 is the only row of part 1
    "P16": [0, 0, 7, 8, 50, 50, 120, 121, 299, 301, 302, 400, 401, 480, 555, 599, N],
    "P3-cut-at-a-hub": [0, 300, 301, N],                       # node 300 (a hub) alone; every hub's row spans all parts
}
DTYPES = [(torch.float32, torch.float32), (torch.float16, torch.bfloat16), (torch.bfloat16, torch.float32),
          (torch.bfloat16, torch.bfloat16)]
SHAPES = [(1, 8), (2, 8), (4, 8), (2, 6)]                      # (heads, C): C = 8 the vector form, C = 6 one column a lane


@functools.lru_cache(maxsize=None)
def _graph():
    from salient_plusplus_amd.inference import graph_gat_chunk
    assert graph_gat_chunk() == 64
    g = torch.Generator().manual_seed(17)
    deg = torch.randint(0, 13, (N,), generator=g)
    deg[5], deg[7], deg[20] = 4, 3, 5                         # (rows that get a self loop or an id outside the graph)
    for node, d in HUBS.items():
        deg[node] = d
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, N, (int(rowptr[-1]),), generator=g)
    for t in (5, 11, 12, 300, N - 1):                          # self loops: entries equal to the target, twice in a hub
        col[int(rowptr[t])] = t
        col[int(rowptr[t + 1]) - 1] = t
    b = int(rowptr[300])
    col[b + 70] = 300                                          # ... and one in a chunk that does not hold the self loop
    for k, bad in ((int(rowptr[7]), -1), (int(rowptr[12]) + 64, N), (int(rowptr[N - 1]) + 200, 1 << 40),
                   (int(rowptr[20]), -(1 << 35))):              # ids outside [0, N): node 0 in every respect
        col[k] = bad
    return rowptr.cuda(), col.cuda()


@functools.lru_cache(maxsize=None)
def _inputs(heads, C, dtype):
    """h [N, heads * C] and the logits [N, 2 * heads] = [a_src | a_dst]"""
    g = torch.Generator().manual_seed(100 * heads + C)
    h = torch.randn((N, heads * C), generator=g).to(dtype).cuda()
    a = (torch.randn((N, 2 * heads), generator=g) * 2.0).cuda()
    return h, a


@functools.lru_cache(maxsize=None)
def _targets():
    g = torch.Generator().manual_seed(3)
    ids = torch.cat([torch.randint(0, N, (90,), generator=g), torch.tensor(list(HUBS) + [0, 0, N - 1, 11, 5]),
                     torch.tensor([-1, N, N + 7, 1 << 40])])   # unsorted, duplicates, ids outside the graph
    return ids[torch.randperm(ids.numel(), generator=g)].cuda()


@functools.lru_cache(maxsize=None)
def _reference(heads, C, dtype, out_dtype, form, relu):
    """graph_gat_aggregate over the whole matrices, once per case; never modified"""
    from salient_plusplus_amd.inference import graph_gat_aggregate
    rowptr, col = _graph()
    h, a = _inputs(heads, C, dtype)
    tgt = dict(row0=37, num_targets=N - 37) if form == "slab" else dict(target_ids=_targets())
    return graph_gat_aggregate(h, a[:, :heads].contiguous(), a[:, heads:].contiguous(), rowptr, col, heads=heads,
                               negative_slope=0.2, relu=relu, out_dtype=out_dtype, **tgt)


def _split(m, off, stride, shift=None):
    """rows [off[p], off[p + 1]) of m, each in an allocation of its own with rows ``stride`` elements apart (None for
    an empty part); part ``shift`` starts one element into its allocation"""
    parts = []
    for p in range(len(off) - 1):
        rows = off[p + 1] - off[p]
        if rows == 0:
            parts.append(None)
            continue
        lead = 1 if p == shift else 0
        assert lead + m.size(1) <= stride
        t = torch.full((rows, stride), float("nan"), dtype=m.dtype, device=m.device)[:, lead:lead + m.size(1)]
        t.copy_(m[off[p]:off[p + 1]])
        parts.append(t)
    return parts


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(_bits(got), _bits(want)), what


@pytest.mark.parametrize("dtype,out_dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("heads,C", SHAPES)
@pytest.mark.parametrize("partition", list(PARTITIONS))
def test_parts_equal_the_whole_matrix(partition, heads, C, dtype, out_dtype):
    from salient_plusplus_amd.inference import graph_gat_aggregate_parts
    rowptr, col = _graph()
    h, a = _inputs(heads, C, dtype)
    off = PARTITIONS[partition]
    F = heads * C
    ids = _targets()
    for form, relu, a_stride in (("slab", True, 2 * heads), ("list", False, 2 * heads + 5)):   # dense / padded logits
        want = _reference(heads, C, dtype, out_dtype, form, relu)
        hp, ap = _split(h, off, F + 8), _split(a, off, a_stride)
        tgt = dict(row0=37, num_targets=N - 37) if form == "slab" else dict(target_ids=ids)
        got = graph_gat_aggregate_parts(hp, ap, off, rowptr, col, heads=heads, negative_slope=0.2, relu=relu,
                                        out_dtype=out_dtype, **tgt)
        _same(got, want, (partition, form))
        if form == "list":                                     # targets outside the graph: rows of zeros
            outside = (ids < 0) | (ids >= N)
            assert int(outside.sum()) == 4 and not bool(got[outside].float().any())
            assert bool(torch.isfinite(got.float()).all())


@pytest.mark.parametrize("dtype,out_dtype", DTYPES[:2], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("partition,shift", [("P4-empty-first-one-row", 2), ("P16", 8), ("P3-cut-at-a-hub", 1)])
def test_one_part_misaligned_for_the_vector_form_gives_the_same_bits(partition, shift, dtype, out_dtype):
    """C = 8 and a stride of a multiple of four would take the vector form; one part's rows start one element into a
    wider allocation of the same stride, so the call reads one column per lane"""
    from salient_plusplus_amd.inference import graph_gat_aggregate_parts
    rowptr, col = _graph()
    heads, C = 2, 8
    h, a = _inputs(heads, C, dtype)
    off = PARTITIONS[partition]
    hp = _split(h, off, heads * C + 8, shift=shift)
    assert hp[shift].data_ptr() % (4 * h.element_size()) != 0 and hp[shift].stride(0) % 4 == 0
    got = graph_gat_aggregate_parts(hp, _split(a, off, 2 * heads), off, rowptr, col, heads=heads, relu=True,
                                    out_dtype=out_dtype, row0=37, num_targets=N - 37)
    _same(got, _reference(heads, C, dtype, out_dtype, "slab", True), (partition, shift))


def test_a_repeated_call_a_reused_workspace_and_out_rows_of_a_larger_matrix():
    """the workspace's contents mean nothing between calls; ``out`` may be rows of a padded matrix"""
    from salient_plusplus_amd.inference import graph_gat_aggregate_parts, graph_gat_workspace_bytes
    rowptr, col = _graph()
    heads, C = 4, 8
    h, a = _inputs(heads, C, torch.bfloat16)
    off = PARTITIONS["P16"]
    hp, ap = _split(h, off, heads * C + 8), _split(a, off, 2 * heads)
    ids = _targets()
    ws = torch.empty(graph_gat_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    ws.fill_(0xFF)
    kw = dict(heads=heads, relu=False, out_dtype=torch.float32, workspace=ws)
    first = graph_gat_aggregate_parts(hp, ap, off, rowptr, col, target_ids=ids, **kw)
    slab = graph_gat_aggregate_parts(hp, ap, off, rowptr, col, row0=37, num_targets=N - 37, **{**kw, "relu": True})
    wide = torch.zeros((ids.numel(), heads * C + 4), dtype=torch.float32, device="cuda")
    again = graph_gat_aggregate_parts(hp, ap, off, rowptr, col, target_ids=ids, out=wide[:, :heads * C], **kw)
    assert again.data_ptr() == wide.data_ptr() and not bool(wide[:, heads * C:].any())
    _same(first, _reference(heads, C, torch.bfloat16, torch.float32, "list", False), "first")
    _same(again, first, "again")
    _same(slab, _reference(heads, C, torch.bfloat16, torch.float32, "slab", True), "slab")


def test_peer_addresses_with_a_view_of_a_wider_buffer():
    """the P2PPeers form as the driver uses it: h read as the leading F columns of a wider published buffer at the
    buffer's stride, the logits as the leading 2 * heads columns of theirs"""
    from salient_plusplus_amd.fast_sampler import P2PPeers
    from salient_plusplus_amd.inference import graph_gat_aggregate_parts
    rowptr, col = _graph()
    heads, C = 2, 8
    h, a = _inputs(heads, C, torch.bfloat16)
    off = PARTITIONS["P4-empty-first-one-row"]
    hp, ap = _split(h, off, 64), _split(a, off, 8)
    peers = P2PPeers([t.data_ptr() if t is not None else 0 for t in hp], 64 * 2, keep=hp)
    apeers = P2PPeers([t.data_ptr() if t is not None else 0 for t in ap], 8 * 4, keep=ap)
    got = graph_gat_aggregate_parts(peers, apeers, off, rowptr, col, heads=heads, relu=True, out_dtype=torch.bfloat16,
                                    row0=37, num_targets=N - 37, dtype=torch.bfloat16, F=heads * C)
    _same(got, _reference(heads, C, torch.bfloat16, torch.bfloat16, "slab", True), "peers")
