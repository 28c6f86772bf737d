"""spp_graph_gat_forward and spp_graph_gat_parts_forward (inference.graph_gat_aggregate, graph_gat_aggregate_parts;
csrc/graph_gat.hip: k_graph_gat_rows, k_graph_gat_long; spp.h f3h / f3k) on the planted graph of tests/graph_gat_f64.py:
every element against the float64 restatement within its first-order bound, in ten logit regimes that differ by head, at
both slopes, for every row type; the short rows bit for bit against the training forward; a row's bits against slabs,
lists and a partitioned table.  The bounds come from the arithmetic (graph_gat_f64.py), never from what the kernel gives;
the tests print the largest err / bound they saw (GRAPH_GAT_F64_RATIO lines): a record, not an input to the bounds.

The shapes (H, C) and what they run: (1, 4) one lane a row, 256 targets a workgroup, the deep row's 34 chunks in one
round; (4, 16) four heads inside one group of 16 lanes, 16 chunks a round: the deep row takes three rounds and both LDS
buffers are written twice; (3, 20) the vector form with a head count that is no power of two; (8, 128) 64 lanes and four
full column steps, 4 chunks a round: the 9 C_g row takes three rounds in each step, the deep row nine, ``round`` carried
across steps and rows; (1, 260) the vector form with 65 pieces on 64 lanes: one active lane in the second step;
(2, 47) the scalar form; (4, 65) the scalar form with a partly active last step.

The training forward the short rows are compared with is spp_gat_forward (k_gat_fwd, through models._GatAggregate): one
head over fp32 rows, F = C columns, the same operations in the same order per column (rescale products, fma, one
division).  The multi-head training kernel (k_gat_mh_agg_fwd) aggregates whole rows of the UNPROJECTED x per head
([T, H, K]) and multiplies by a reciprocal where this kernel divides, so H > 1, fp16 and bf16 rows have no training
counterpart with the same bits: the comparison runs at the H = 1 shapes with fp32 rows.

Seen on an MI355X: the docstring of test_zz_largest_ratios_seen."""
import collections
import functools

import pytest
import torch

import gat_f64
import graph_gat_f64 as gg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4), (4, 16), (3, 20), (8, 128)]                 # every regime
MORE_SHAPES = [(1, 260), (2, 47), (4, 65)]                    # "model", "wide" and the two regimes of graph_gat_f64
FEW = ["model", "wide", "last_chunk_max", "dead_chunk"]
CASES = [(H, C, r) for H, C in SHAPES for r in gg.REGIMES] + [(H, C, r) for H, C in MORE_SHAPES for r in FEW]
ROW_DTYPES = [torch.float32, torch.float16, torch.bfloat16]
N = gg.N
SEEN = collections.defaultdict(float)


def _name(d):
    return str(d).split(".")[-1]


@functools.lru_cache(maxsize=None)
def _cg():
    from salient_plusplus_amd.inference import graph_gat_chunk
    return graph_gat_chunk()


@functools.lru_cache(maxsize=None)
def _graph():
    hop = gg.planted_graph(_cg())
    return hop, hop.rowptr.cuda(), hop.col.cuda()


@functools.lru_cache(maxsize=None)
def _ref(regime, H, C, slope):
    """computed once per case, shared by the row types (h holds the same numbers in all three) and never modified"""
    return gg.reference(_graph()[0], *gg.inputs(regime, H, C, _cg()), slope, _cg())


@functools.lru_cache(maxsize=8)
def _device(regime, H, C, dtype):
    h, a_src, a_dst = gg.inputs(regime, H, C, _cg())
    return h.reshape(N, H * C).to(dtype).cuda(), a_src.cuda(), a_dst.cuda()


def _run(regime, H, C, dtype, slope, **kw):
    from salient_plusplus_amd.inference import graph_gat_aggregate
    _hop, rowptr, col = _graph()
    if not any(k in kw for k in ("row0", "target_ids")):
        kw.update(row0=0, num_targets=N)
    return graph_gat_aggregate(*_device(regime, H, C, dtype), rowptr, col, heads=H, negative_slope=slope, **kw)


def _within(key, got, ref, bound, what):
    """every element compared; the largest err / bound over all rows, and over the long rows alone for the record (the
    largest of all tends to sit in a short row, at an element near 2^-126)"""
    hop = _graph()[0]
    ratio, where = gg.worst(got, ref, bound, hop)
    long_rows = hop.raw > _cg()
    SEEN[key] = max(SEEN[key], ratio)
    SEEN[key + ", long rows"] = max(SEEN[key + ", long rows"], gg.worst(got.cpu()[long_rows], ref[long_rows], bound[long_rows])[0])
    assert ratio <= 1.0, (what, where)
    return ratio, f"{what}: {where}"


@pytest.mark.parametrize("dtype", ROW_DTYPES, ids=_name)
@pytest.mark.parametrize("H,C,regime", CASES)
def test_every_element_is_within_its_float64_bound(H, C, regime, dtype):
    h = gg.inputs(regime, H, C, _cg())[0].double()
    top = {}
    for slope in gat_f64.SLOPES:
        ref = _ref(regime, H, C, slope)
        what = f"{regime} slope {slope:.3g}"
        got = _run(regime, H, C, dtype, slope)
        assert got.dtype == torch.float32 and got.shape == (N, H * C)
        got = got.view(N, H, C)
        top["fp32"] = max(top.get("fp32", (0.0, "")), _within(f"H={H} C={C} fp32 output", got, ref.out, ref.b_out, what))
        for t in (0, gg.ISOLATED, gg.ONLY_SELF):              # rows that keep nothing: h[t], to their FLUSH-level bound
            assert float(ref.b_out[t].max()) == gat_f64.FLUSH
            assert bool(((got[t].double().cpu() - h[t]).abs() <= ref.b_out[t]).all()), (what, t)
        if regime in ("model", "wide", "last_chunk_max"):
            wide = gg.widen_bf16(ref.out, ref.b_out)
            got = _run(regime, H, C, dtype, slope, out_dtype=torch.bfloat16)
            assert got.dtype == torch.bfloat16
            top["bf16"] = max(top.get("bf16", (0.0, "")),
                              _within(f"H={H} C={C} bf16 output", got.view(N, H, C), ref.out, wide, what + " bf16 output"))
            got = _run(regime, H, C, dtype, slope, relu=True)
            top["relu"] = max(top.get("relu", (0.0, "")),
                              _within(f"H={H} C={C} relu", got.view(N, H, C), torch.relu(ref.out), ref.b_out, what + " relu"))
    print(f"\nGRAPH_GAT_F64_RATIO H={H} C={C} rows={_name(dtype)} {regime}: " +
          "; ".join(f"{k} {v[0]:.3f} ({v[1]})" for k, v in top.items()))


@pytest.mark.parametrize("H,C", [(1, 4), (1, 260)])
def test_short_rows_carry_the_training_kernels_bits(H, C):
    """rows of at most C_g raw entries, one head, fp32 rows and output, relu = 0: spp_gat_forward over the whole graph as
    one square hop (T = S = N) on the same projected rows and logits (see the module docstring)"""
    from salient_plusplus_amd.models import _GatAggregate
    hop, rowptr, col = _graph()
    short = (hop.raw <= _cg()).cuda()
    assert int(short.sum()) > 600 and int((~short).sum()) >= 7
    for slope in gat_f64.SLOPES:
        for regime in FEW + ["mixed", "selfmin"]:
            h, a_src, a_dst = _device(regime, H, C, torch.float32)
            want = _GatAggregate.apply(h, a_src[:, 0], a_dst[:, 0], rowptr, col, slope)
            got = _run(regime, H, C, torch.float32, slope)
            assert torch.equal(got[short].view(torch.int32), want[short].view(torch.int32)), (regime, slope)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("regime", ["last_chunk_max", "wide"])
@pytest.mark.parametrize("H,C,dtype", [(4, 16, torch.bfloat16), (2, 47, torch.float32)], ids=["4x16-bf16", "2x47-fp32"])
def test_parts_lists_and_slabs_give_the_same_bits(H, C, dtype, regime):
    """the whole table in one call, the same rows as three slabs, as a shuffled list with duplicates, and from three
    parts (one of them empty) whose logits sit in rows wider than 2 H: one row, one bit pattern"""
    from salient_plusplus_amd.inference import graph_gat_aggregate_parts
    hop, rowptr, col = _graph()
    slope = gat_f64.SLOPES[0]
    h, a_src, a_dst = _device(regime, H, C, dtype)
    whole = _bits(_run(regime, H, C, dtype, slope))
    cuts = [0, 13, 300, N]                                    # (the deep row opens the second slab)
    slabs = torch.cat([_bits(_run(regime, H, C, dtype, slope, row0=b, num_targets=e - b)) for b, e in zip(cuts, cuts[1:])])
    g = torch.Generator().manual_seed(3)
    ids = torch.cat([torch.randperm(N, generator=g), torch.tensor(hop.planted + [gg.DEEP_ROW, 8, 8, gg.ISOLATED])])
    ids = ids[torch.randperm(ids.numel(), generator=g)].cuda()
    listed = _bits(_run(regime, H, C, dtype, slope, target_ids=ids))
    off = [0, 300, 300, N]
    a = torch.cat([a_src, a_dst], 1)
    hp, ap = [], []
    for b, e in zip(off, off[1:]):
        if e == b:
            hp.append(None), ap.append(None)
            continue
        wide = torch.full((e - b, 2 * H + 3), float("nan"), device="cuda")
        wide[:, :2 * H] = a[b:e]
        hp.append(h[b:e].clone()), ap.append(wide[:, :2 * H])
    parts = _bits(graph_gat_aggregate_parts(hp, ap, off, rowptr, col, heads=H, negative_slope=slope, row0=0, num_targets=N))
    for what, got, want in (("slabs", slabs, whole), ("parts", parts, whole), ("list", listed, whole[ids])):
        rows = torch.nonzero((got != want).any(1)).flatten().tolist()       # row by row: the rows that differ
        assert got.shape == want.shape and not rows, (what, rows if what != "list" else ids[rows].tolist())


def test_zz_largest_ratios_seen():
    """prints the largest err / bound per shape and output over the tests of this module that ran before it.

    Seen on an MI355X (a record, not an input to the bounds), largest err / bound per shape (H, C) in the order (1, 4),
    (4, 16), (3, 20), (8, 128), (1, 260), (2, 47), (4, 65): fp32 output 0.171, 0.263, 0.320, 0.487, 0.487, 0.487, 0.395
    -- every one of them in a SHORT row ("wide" at slope 0.2, an element near 2^-126, or a row of two entries whose bound
    is the __expf term alone); over the long rows alone 0.010, 0.031, 0.043, 0.091, 0.039, 0.020, 0.019.  bf16 output
    0.987-0.995 (bf16's own rounding: the widened bound is 2^-8 relative and a value just above a power of two uses
    all of it), over the long rows 0.83-0.98.  relu 0.136, 0.261, 0.320, 0.395, 0.262, 0.487, 0.395.  None is near 1 but
    the bf16 rounding; with State::merge changed to ignore f1 (a temporary build) "last_chunk_max" failed at all seven
    shapes, by err / bound between 1.2e5 and 1e22."""
    print("\nGRAPH_GAT_F64_LARGEST " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(SEEN.items())))
