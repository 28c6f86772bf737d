"""-m gpu: the receptive field (f3n; inference.ReceptiveFields / receptive_field over csrc/field.hip) against a numpy
restatement of its definition: depth 0 is the distinct ids of ``nodes``, depth d every neighbour of a node of depth d - 1
that has no smaller depth; slots count depth by depth, in ascending id order within a depth; the field's CSR holds the
whole row of every node of depth <= h - 1 in CSR order, every entry replaced by its slot.  Everything is compared exactly.

The graph: 2 500 nodes in two disconnected components -- A = [0, 2460), sparse (0..5 entries a row), with a hub of 3 000
entries (47 times the kernels' cut of 64, so its row takes the long-row launch), a node with no edge at all, a self-loop
and a row of repeated entries; B = [2460, 2500), dense enough that two hops from any of its nodes reach all of it."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N, NA = 2500, 2460
HUB, HUB_DEG, LONE, LOOP, REPEAT, SINGLE, HUB_NB, IN_B = 7, 3000, 100, 5, 6, 1234, 300, 2470
HOPS = [0, 1, 2, 3]


@functools.lru_cache(maxsize=None)
def graph_np():
    """(rowptr, col) int64 on the host"""
    rng = np.random.default_rng(5)
    deg = rng.integers(0, 6, N)
    deg[NA:] = 20
    deg[HUB], deg[LONE], deg[LOOP], deg[REPEAT], deg[SINGLE], deg[HUB_NB] = HUB_DEG, 0, 3, 4, 5, 4
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = np.empty(rowptr[-1], dtype=np.int64)
    col[:rowptr[NA]] = rng.integers(0, NA, rowptr[NA])
    col[rowptr[NA]:] = rng.integers(NA, N, rowptr[-1] - rowptr[NA])
    col[col == LONE] = LONE + 1                               # nobody points at the node without a row
    col[rowptr[LOOP]] = LOOP                                  # a self-loop
    col[rowptr[REPEAT]:rowptr[REPEAT + 1]] = [9, 9, 12, 9]    # repeated entries
    col[rowptr[HUB] + 17] = HUB_NB
    return rowptr, col


@functools.lru_cache(maxsize=None)
def graph():
    rowptr, col = graph_np()
    return torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda()


@functools.lru_cache(maxsize=None)
def node_sets():
    rng = np.random.default_rng(6)
    return {
        "single": np.array([SINGLE]),
        "hub": np.array([HUB]),
        "hub_neighbour": np.array([HUB_NB]),
        "lone": np.array([LONE]),
        "in_b": np.array([IN_B]),
        "random300": rng.integers(0, N, 300),                # unsorted, with duplicates (birthday: 300 of 2 500)
    }


def field_oracle(rowptr, col, nodes, hops):
    """the definition, restated: a BFS with ascending-id numbering, rows copied in CSR order"""
    slot = np.full(len(rowptr) - 1, -1, dtype=np.int64)
    depths = [np.unique(nodes)]
    slot[depths[0]] = np.arange(len(depths[0]))
    sizes = [len(depths[0])]
    for _ in range(hops):
        rows = [col[rowptr[t]:rowptr[t + 1]] for t in depths[-1]]
        nb = np.concatenate(rows) if rows else np.empty(0, dtype=np.int64)
        new = np.unique(nb[slot[nb] < 0])
        slot[new] = sizes[-1] + np.arange(len(new))
        depths.append(new)
        sizes.append(sizes[-1] + len(new))
    ids = np.concatenate(depths)
    inner = ids[:sizes[hops - 1]] if hops else ids[:0]
    frowptr = np.zeros(len(inner) + 1, dtype=np.int64)
    frowptr[1:] = np.cumsum(rowptr[inner + 1] - rowptr[inner])
    rows = [slot[col[rowptr[t]:rowptr[t + 1]]] for t in inner]
    fcol = np.concatenate(rows) if rows else np.empty(0, dtype=np.int64)
    return dict(ids=ids, sizes=sizes, pos=slot[nodes], rowptr=frowptr, col=fcol)


def as_np(f):
    return dict(ids=f.ids.cpu().numpy(), sizes=list(f.sizes), pos=f.pos.cpu().numpy(), rowptr=f.rowptr.cpu().numpy(),
                col=f.col.cpu().numpy())


def assert_same(got, want):
    assert got["sizes"] == want["sizes"] and all(isinstance(v, int) for v in got["sizes"])
    for k in ("ids", "pos", "rowptr", "col"):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_the_graph_is_what_the_cases_need():
    from salient_plusplus_amd.inference import field_chunk
    rowptr, col = graph_np()
    deg = np.diff(rowptr)
    assert deg[HUB] == HUB_DEG > 40 * field_chunk() and deg[LONE] == 0 and LONE not in col
    assert LOOP in col[rowptr[LOOP]:rowptr[LOOP + 1]] and HUB_NB in col[rowptr[HUB]:rowptr[HUB + 1]]
    assert len(set(col[rowptr[REPEAT]:rowptr[REPEAT + 1]])) < deg[REPEAT]
    assert col[:rowptr[NA]].max() < NA <= col[rowptr[NA]:].min()            # two components, no edge between them
    sets = node_sets()
    assert len(np.unique(sets["random300"])) < 300 and not np.all(np.diff(sets["random300"]) >= 0)
    # one case stays small, one saturates its component: the suite cannot pass on whole-graph fields alone
    small = field_oracle(rowptr, col, sets["single"], 3)["sizes"]
    assert 1 < small[3] < N / 4
    full = field_oracle(rowptr, col, sets["in_b"], 3)["sizes"]
    assert full[1] < full[2] == full[3] == N - NA


@pytest.mark.parametrize("hops", HOPS)
@pytest.mark.parametrize("name", ["single", "hub", "hub_neighbour", "lone", "in_b", "random300"])
def test_field_equals_the_definition(name, hops):
    from salient_plusplus_amd.inference import Field, receptive_field
    rowptr, col = graph()
    nodes = node_sets()[name]
    f = receptive_field(rowptr, col, torch.from_numpy(nodes).cuda(), hops)
    assert isinstance(f, Field) and f.hops == hops and f.ids.is_cuda
    want = field_oracle(*graph_np(), nodes, hops)
    print(f"{name} hops={hops}: sizes {f.sizes}, edges {f.col.numel()}")
    assert_same(as_np(f), want)
    if hops == 0:
        assert f.rowptr.tolist() == [0] and f.col.numel() == 0
    # the nest of prefixes: the rows [0, sizes[d]) name only slots below sizes[d + 1]
    for d in range(hops):
        e = int(f.rowptr[f.sizes[d]])
        assert e == 0 or int(f.col[:e].max()) < f.sizes[d + 1]
    # and nodes given on the host build the same field
    assert_same(as_np(receptive_field(rowptr, col, torch.from_numpy(nodes), hops)), want)


def test_two_runs_give_identical_arrays():
    from salient_plusplus_amd.inference import ReceptiveFields
    rowptr, col = graph()
    nodes = torch.from_numpy(node_sets()["random300"]).cuda()
    fields = ReceptiveFields(rowptr, col)
    a, b = as_np(fields.field(nodes, 3)), as_np(fields.field(nodes, 3))
    assert_same(a, b)
    assert_same(as_np(ReceptiveFields(rowptr, col).field(nodes, 3)), a)


def _clean(fields):
    return bool((fields.slot == -1).all()) and bool((fields.flag == 0).all())


def test_a_reused_object_builds_what_a_fresh_one_builds_and_leaves_its_maps_clean(monkeypatch):
    from salient_plusplus_amd import inference as inf
    rowptr, col = graph()
    sets = node_sets()
    fields = inf.ReceptiveFields(rowptr, col)
    assert fields.slot.dtype == torch.int32 and fields.flag.dtype == torch.uint8 and fields.slot.shape == fields.flag.shape == (N,)
    assert _clean(fields)
    fields.field(torch.from_numpy(sets["hub"]).cuda(), 2)     # a large field first
    assert _clean(fields)
    second = fields.field(torch.from_numpy(sets["random300"]).cuda(), 3)
    assert _clean(fields)
    assert_same(as_np(second), field_oracle(*graph_np(), sets["random300"], 3))
    # a call that raises after it has marked and numbered: the maps are put back all the same
    def broken(*_a, **_k):
        raise RuntimeError("no rows today")
    with monkeypatch.context() as m:
        m.setattr(inf, "_field_rows", broken)
        with pytest.raises(RuntimeError, match="no rows today"):
            fields.field(torch.from_numpy(sets["hub"]).cuda(), 2)
    assert _clean(fields)
    mark = inf._field_mark

    def marks_then_raises(*a, **k):
        mark(*a, **k)
        raise RuntimeError("marked, not compacted")
    with monkeypatch.context() as m:
        m.setattr(inf, "_field_mark", marks_then_raises)
        with pytest.raises(RuntimeError, match="marked, not compacted"):
            fields.field(torch.from_numpy(sets["hub"]).cuda(), 1)
    assert _clean(fields)
    # refused arguments touch nothing
    with pytest.raises(ValueError, match="nodes outside the graph"):
        fields.field(torch.tensor([0, N]).cuda(), 1)
    with pytest.raises(ValueError, match="hops"):
        fields.field(torch.tensor([0]).cuda(), -1)
    assert _clean(fields)
    third = fields.field(torch.from_numpy(sets["single"]).cuda(), 3)
    assert_same(as_np(third), field_oracle(*graph_np(), sets["single"], 3))


def test_no_nodes_give_an_empty_field():
    from salient_plusplus_amd.inference import receptive_field
    rowptr, col = graph()
    f = receptive_field(rowptr, col, torch.empty(0, dtype=torch.int64), 2)
    assert f.sizes == [0, 0, 0] and f.ids.numel() == f.pos.numel() == f.col.numel() == 0 and f.rowptr.tolist() == [0]


def test_the_entries_take_an_id_outside_the_graph_as_an_empty_row():
    """include/spp.h, f3n: no fault and no error -- nothing is flagged for it, and its row of the field stays as it was"""
    from salient_plusplus_amd import inference as inf
    rowptr, col = graph()
    slot = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    flag = torch.zeros(N, dtype=torch.uint8, device="cuda")
    ids = torch.tensor([N, REPEAT, -1, 1 << 40], device="cuda")
    inf._field_mark(rowptr, col, N, ids, slot, flag)
    assert flag.nonzero().view(-1).tolist() == [9, 12]
    slot[9], slot[12] = 0, 1
    frowptr = torch.tensor([0, 4, 8, 12, 16], device="cuda")
    fcol = torch.full((16,), -7, dtype=torch.int64, device="cuda")
    inf._field_rows(rowptr, col, N, ids, slot, frowptr, fcol)
    assert fcol.tolist() == [-7] * 4 + [0, 0, 1, 0] + [-7] * 8
    # a row that frowptr gives less room than its degree is cut to the room: nothing is written past it
    fcol.fill_(-7)
    inf._field_rows(rowptr, col, N, ids[1:2], slot, torch.tensor([2, 4], device="cuda"), fcol[:5])
    assert fcol.tolist() == [-7, -7, 0, 0] + [-7] * 12
