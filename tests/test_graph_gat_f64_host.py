"""CPU-only: the float64 helper of the GAT long-row inference suite (tests/graph_gat_f64.py) checked against itself --
the planted graph has the rows it promises, the two float64 statements agree, the contract in fp32 torch ops stays inside
every bound with no element left out, and each of five planted faults leaves the bounds in the regime named for it.  The
regimes' own properties (last_chunk_max, dead_chunk) are asserted inside graph_gat_f64.regime; here they are run for every
head count of the GPU suite's shapes.

Each clean case prints the median and the maximum of  bound / (2e-4 |ref| + 2e-5 max|h|), the tolerance of
test_gpu_gat_inference.py::test_kernel_matches_the_float64_formula: a record of how the two compare, not asserted."""
import functools

import pytest
import torch

import gat_f64
import graph_gat_f64 as gg

SLOPE_IDS = ["slope0.2", "slope0.25"]


@functools.lru_cache(maxsize=None)
def _cg():
    """the helper is checked at the kernel's own chunk, so that the self-check follows C_g if it ever changes"""
    from salient_plusplus_amd import build
    from salient_plusplus_amd.inference import graph_gat_chunk
    build.build()
    return graph_gat_chunk()


@functools.lru_cache(maxsize=32)
def _ref(regime, H, C, slope):
    hop = gg.planted_graph(_cg())
    return gg.reference(hop, *gg.inputs(regime, H, C, _cg()), slope, _cg())


def test_the_planted_graph_has_the_rows_it_promises():
    CG = _cg()
    hop = gg.planted_graph(CG)
    raw = hop.raw.tolist()
    assert raw[:9] == [0, 1, 63, 64, 65, CG, CG + 1, 3 * CG + 7, 9 * CG] and raw[gg.ISOLATED] == 0
    assert 650 <= hop.T == gg.N <= 750 and not bool((hop.col == gg.ISOLATED).any())
    b = int(hop.rowptr[gg.EMPTY_CHUNK_ROW])
    assert hop.col[b + CG:b + 2 * CG].tolist() == [gg.EMPTY_CHUNK_ROW] * CG and raw[gg.EMPTY_CHUNK_ROW] > 2 * CG
    row10 = hop.col[hop.rowptr[10]:hop.rowptr[11]].tolist()
    assert row10[0] == row10[3] == row10[6] == 10 and row10[4] == row10[5] and len(row10) <= CG
    assert int(hop.kept[gg.ONLY_SELF]) == 0 and raw[gg.ONLY_SELF] == 3
    assert raw[gg.DROPPED_TAIL_ROW] == CG + 1 and int(hop.col[hop.rowptr[gg.DROPPED_TAIL_ROW] + CG]) == gg.DROPPED_TAIL_ROW
    deep = hop.col[hop.rowptr[gg.DEEP_ROW]:hop.rowptr[gg.DEEP_ROW + 1]]
    assert deep.numel() == 33 * CG + 1 and deep.unique().numel() < deep.numel()
    edges = [p for p in torch.nonzero(deep == gg.DEEP_ROW).flatten().tolist() if p % CG in (0, CG - 1)]
    assert len(edges) >= 2                                        # diagonal entries kept at two chunk edges
    others = torch.ones(gg.N, dtype=torch.bool)
    others[hop.planted] = False
    assert int(hop.raw[others].max()) <= 12 and hop.hub_hi == 52
    # the merge rounds the deep row is there for: 256 / lpr chunks a round (csrc/graph_gat.hip, k_graph_gat_long)
    rounds = lambda chunks, lpr: -(-chunks // (256 // lpr))       # noqa: E731
    assert rounds(-(-raw[gg.DEEP_ROW] // CG), 16) >= 3 and rounds(-(-raw[8] // CG), 64) >= 3


@pytest.mark.parametrize("H", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("name", ["last_chunk_max", "dead_chunk"])
def test_the_regimes_of_this_file_hold_their_conditions(name, H):
    """the assertions are inside gg.regime (every head, both slopes); the heads must also differ"""
    a_src, a_dst = gg.regime(name, gg.planted_graph(_cg()), H, _cg())
    assert a_src.shape == a_dst.shape == (gg.N, H) and a_src.dtype == torch.float32
    for k in range(1, H):
        assert not torch.equal(a_src[:, k], a_src[:, 0])


@pytest.mark.parametrize("H,C", [(4, 16), (3, 20)])
@pytest.mark.parametrize("regime", gg.REGIMES)
def test_the_two_float64_statements_agree(regime, H, C):
    hop = gg.planted_graph(_cg())
    h, a_src, a_dst = gg.inputs(regime, H, C, _cg())
    ref = _ref(regime, H, C, gat_f64.SLOPES[0])
    rows = gg.plain_rows(hop.rowptr, hop.col, h, a_src, a_dst, gat_f64.SLOPES[0])
    scale = torch.clamp(rows.abs(), min=1e-3)                     # (|h| is a multiple of 2^-6: 1e-3 is far below one step)
    assert float(((ref.out - rows).abs() / scale).max()) < 1e-12
    # (a bound is 0 only where every row of h that enters is 0 in that column: there the result is an exact 0)
    assert bool((ref.b_out >= 0).all()) and float(ref.b_out.max()) < 1e-3
    assert bool(((ref.b_out > 0) | (ref.out == 0)).all())
    M = ref.M.tolist()
    assert M[:14] == [0, 0, 0, 0, 1, 0, 1, 3, 8, 2, 0, 0, 1, 33] and max(M[14:]) == 0
    for t in (0, gg.ISOLATED, gg.ONLY_SELF):                      # rows that keep nothing: their own row, FLUSH-level
        assert torch.equal(ref.out[t], h[t].double()) and float(ref.b_out[t].max()) == gat_f64.FLUSH


CLEAN = [(H, C, r) for H, C in [(1, 4), (4, 16), (3, 20)] for r in gg.REGIMES] + [(2, 47, "model"), (2, 47, "wide")]


@pytest.mark.parametrize("slope", gat_f64.SLOPES, ids=SLOPE_IDS)
@pytest.mark.parametrize("H,C,regime", CLEAN)
def test_a_correct_chunked_fp32_computation_stays_inside_every_bound(H, C, regime, slope):
    hop = gg.planted_graph(_cg())
    h, a_src, a_dst = gg.inputs(regime, H, C, _cg())
    ref = _ref(regime, H, C, slope)
    got = gg.chunked_fp32(hop.rowptr, hop.col, h, a_src, a_dst, slope, _cg())
    ratio, where = gg.worst(got, ref.out, ref.b_out, hop)
    left_out = int((~torch.isfinite(ref.b_out) | (ref.b_out < 0)).sum())     # (worst() compares every element)
    old = 2e-4 * ref.out.abs() + 2e-5 * max(1.0, float(h.abs().max()))
    rel = (ref.b_out / old).flatten()
    print(f"GRAPH_GAT_F64_HOST H={H} C={C} {regime} slope {slope:.3g}: chunked fp32 err / bound {ratio:.3f} at {where}; "
          f"bound / old tolerance median {float(rel.median()):.2e} max {float(rel.max()):.2e}; left out {left_out}")
    assert left_out == 0 and got.shape == ref.out.shape
    assert ratio <= 1.0, where


# fault -> (regime, H, C), the pairing in which it must show; H > 1 wherever the fault is about heads
FAULT_CASES = [("no_rescale", "ascending", 4, 16), ("no_rescale", "last_chunk_max", 3, 20),
               ("self_everywhere", "model", 4, 16), ("self_everywhere", "selfmax", 1, 4),
               ("keep_diag", "model", 4, 16), ("keep_diag", "selfmax", 3, 20),
               ("head0_everywhere", "model", 4, 16), ("head0_everywhere", "last_chunk_max", 3, 20),
               ("head0_everywhere", "mixed", 4, 16),
               ("merge_skips_last", "last_chunk_max", 4, 16), ("merge_skips_last", "last_chunk_max", 1, 4)]


@pytest.mark.parametrize("fault,regime,H,C", FAULT_CASES)
def test_planted_faults_leave_the_bounds(fault, regime, H, C):
    hop = gg.planted_graph(_cg())
    CG, slope = _cg(), gat_f64.SLOPES[0]
    h, a_src, a_dst = gg.inputs(regime, H, C, CG)
    ref = _ref(regime, H, C, slope)
    got = gg.chunked_fp32(hop.rowptr, hop.col, h, a_src, a_dst, slope, CG, fault=fault)
    ratio, where = gg.worst(got, ref.out, ref.b_out, hop)
    print(f"GRAPH_GAT_F64_HOST fault {fault} in {regime} H={H} C={C}: largest err / bound {ratio:.3e} at {where}")
    assert ratio > 1.0, (fault, regime, where)
    bad = ((got.double() - ref.out).abs() > ref.b_out).flatten(1).any(1)            # and only where it can show
    can_show = {"keep_diag": hop.kept < hop.raw, "head0_everywhere": hop.n > 1,
                "merge_skips_last": hop.raw > 2 * CG}.get(fault, hop.raw > CG)
    assert bool(bad.any()) and not bool((bad & ~can_show).any())


def test_every_fault_has_a_case():
    assert sorted({f for f, *_ in FAULT_CASES}) == sorted(gg.FAULTS)
