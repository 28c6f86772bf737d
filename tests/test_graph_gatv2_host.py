"""CPU-only: the host side of exact layer-wise GATv2 inference (spp.h f3w) -- the exported entries and the ctypes layout
of spp_graph_gatv2_desc against the header, every refusal of spp_graph_gatv2_forward that needs no device, the argument
validation of inference.graph_gatv2_aggregate / gatv2_inference / evaluate before any device call, the entries that keep
refusing a GATv2 model (the field and partitioned ones) and the three spellings of the resident one, the float64
helper's own check (tests/graph_gatv2_f64.py: a correct chunked fp32 computation stays inside every bound, three
planted faults leave them), and the channel-padding identity of the driver."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_FAKE = 0x10000
SPP_OK, SPP_ERR_INVALID = 0, -1                               # spp_status (include/spp.h)


@pytest.fixture
def no_device(monkeypatch):
    """any step towards the device fails the test: the refusals must come first"""
    from salient_plusplus_amd import _native as nat

    def touched(*_a, **_k):
        raise AssertionError("a device call was made before the arguments were refused")
    monkeypatch.setattr(nat, "require_device", touched)


def _lib():
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import build
    build.build()
    return nat, nat.load()


def test_library_exports_the_graph_gatv2_entries():
    from salient_plusplus_amd.inference import graph_gatv2_chunk, graph_gatv2_workspace_bytes
    nat, L = _lib()
    for name in ("spp_graph_gatv2_forward", "spp_graph_gatv2_chunk", "spp_graph_gatv2_workspace_bytes"):
        assert hasattr(L, name) and name in nat.SIGNATURES
    assert L.spp_abi_version() == 6
    assert graph_gatv2_chunk() >= 32
    counts = (0, 1, 2, 7, 1000, 1 << 20, 1 << 33)
    sizes = [graph_gatv2_workspace_bytes(T) for T in counts]
    assert sizes == sorted(sizes) and sizes[0] >= 16 and all(b >= 8 * T for b, T in zip(sizes, counts))


def test_graph_gatv2_desc_layout_matches_header():
    """sizeof and every field offset of spp_graph_gatv2_desc, cross-checked by compiling the header with gcc"""
    from salient_plusplus_amd import _native as nat
    names = [n for n, _t in nat.GraphGatv2Desc._fields_]
    offs = ", ".join(f"offsetof(spp_graph_gatv2_desc, {n})" for n in names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spp.h"\n'
            "int main(void) { size_t v[] = { sizeof(spp_graph_gatv2_desc), " + offs + " };\n"
            "  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\n  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(nat.GraphGatv2Desc)] + [getattr(nat.GraphGatv2Desc, n).offset for n in names]


def _desc(nat, **over):
    """a descriptor that passes every check; the pointers are never dereferenced by a refusal (nothing is enqueued)"""
    kw = dict(x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, heads=2, relu=0, rowptr_dev=_FAKE, col_dev=_FAKE,
              x_l_dev=_FAKE, x_l_stride_elems=16, x_r_dev=_FAKE, x_r_stride_elems=16, x_rows=10, C=8, att_dev=_FAKE,
              target_row0=0, target_ids_dev=None, num_targets=4, out_dev=_FAKE, out_stride_elems=0, negative_slope=0.2)
    kw.update(over)
    return nat.GraphGatv2Desc(**kw)


REFUSALS = [
    ("heads = 3", dict(heads=3, C=4), {}, b"heads"),
    ("heads = 16", dict(heads=16, C=4), {}, b"heads"),
    ("C = 0", dict(C=0), {}, b"C"),
    ("C = 6", dict(C=6), {}, b"C %"),
    ("C = 12: C / 4 no power of two", dict(C=12, x_l_stride_elems=24, x_r_stride_elems=24), {}, b"power of two"),
    ("D = 2048", dict(heads=8, C=256, x_l_stride_elems=2048, x_r_stride_elems=2048), {}, b"1024"),
    ("unknown x_elem", dict(x_elem=77), {}, b"x_elem"),
    ("fp16 output", dict(out_elem="F16"), {}, b"out_elem"),
    ("fp8 rows", dict(x_elem="FP8_E4M3"), {}, b"fp8"),
    ("fp8 output", dict(out_elem="FP8_E4M3"), {}, b"fp8"),
    ("both target forms", dict(target_ids_dev=_FAKE), {}, b"not both"),
    ("neither target form", dict(target_row0=-1), {}, b"target_row0"),
    ("slab outside the graph", dict(target_row0=8, num_targets=4), {}, b"target_row0"),
    ("missing workspace", {}, dict(ws=None), b"spp_graph_gatv2_workspace_bytes"),
    ("misaligned workspace", {}, dict(ws=_FAKE + 8), b"workspace"),
    ("small workspace", {}, dict(bytes=8), b"workspace"),
    ("x_l stride smaller than the row", dict(x_l_stride_elems=12), {}, b"x_l_stride_elems"),
    ("x_r stride smaller than the row", dict(x_r_stride_elems=12), {}, b"x_r_stride_elems"),
    ("output stride smaller than the row", dict(out_stride_elems=8), {}, b"out_stride_elems"),
    ("misaligned output base", dict(out_dev=_FAKE + 4), {}, b"out_dev"),
    ("misaligned output stride", dict(out_stride_elems=18), {}, b"out_dev"),
    ("misaligned x_l base", dict(x_l_dev=_FAKE + 4), {}, b"misaligned"),
    ("misaligned x_r base", dict(x_r_dev=_FAKE + 4), {}, b"misaligned"),
    ("x_l stride no multiple of 4", dict(x_l_stride_elems=18), {}, b"misaligned"),
    ("x_r stride no multiple of 4", dict(x_r_stride_elems=18), {}, b"misaligned"),
    ("misaligned att", dict(att_dev=_FAKE + 4), {}, b"misaligned"),
    ("NULL att", dict(att_dev=None), {}, b"NULL"),
    ("NULL x_r", dict(x_r_dev=None), {}, b"NULL"),
]


@pytest.mark.parametrize("what,over,call,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_refuses_before_anything_is_enqueued(what, over, call, word):
    nat, L = _lib()
    over = {k: getattr(nat, "SPP_ELEM_" + v) if isinstance(v, str) else v for k, v in over.items()}
    d = _desc(nat, **over)
    ws = call.get("ws", _FAKE)
    nbytes = call.get("bytes", int(L.spp_graph_gatv2_workspace_bytes(d.num_targets)))
    assert L.spp_graph_gatv2_forward(ctypes.byref(d), ctypes.c_void_p(ws), nbytes, None) == SPP_ERR_INVALID, what
    assert word in L.spp_last_error(), (what, L.spp_last_error())


def test_entry_refuses_a_null_descriptor_and_accepts_an_empty_call():
    nat, L = _lib()
    assert L.spp_graph_gatv2_forward(None, ctypes.c_void_p(_FAKE), 1 << 20, None) == SPP_ERR_INVALID
    assert b"NULL descriptor" in L.spp_last_error()
    d = _desc(nat, num_targets=0)                             # T == 0: SPP_OK without touching a device or a buffer
    assert L.spp_graph_gatv2_forward(ctypes.byref(d), ctypes.c_void_p(_FAKE), 1 << 10, None) == SPP_OK


def _tiny(H=2, Cc=8):
    x = torch.zeros((3, H * Cc))
    return x, x.clone(), torch.zeros((H, Cc)), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])


def test_graph_gatv2_aggregate_validates_its_arguments(no_device):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.inference import graph_gatv2_aggregate as agg
    x_l, x_r, att, rowptr, col = _tiny()
    slab = dict(row0=0, num_targets=3)
    with pytest.raises(ValueError, match="not both"):
        agg(x_l, x_r, att, rowptr, col, target_ids=torch.tensor([0]), **slab)
    with pytest.raises(ValueError, match="either as a slab"):
        agg(x_l, x_r, att, rowptr, col)
    with pytest.raises(ValueError, match="leaves the graph"):
        agg(x_l, x_r, att, rowptr, col, row0=2, num_targets=2)
    with pytest.raises(ValueError, match="target_ids"):
        agg(x_l, x_r, att, rowptr, col, target_ids=torch.tensor([0], dtype=torch.int32))
    with pytest.raises(ValueError, match="x_r must have x_l's shape"):
        agg(x_l, x_r[:, :8], att, rowptr, col, **slab)
    with pytest.raises(ValueError, match="x_r must have x_l's shape"):
        agg(x_l, x_r.half(), att, rowptr, col, **slab)
    with pytest.raises(ValueError, match="att"):
        agg(x_l, x_r, att.double(), rowptr, col, **slab)
    with pytest.raises(ValueError, match="att"):
        agg(x_l, x_r, att.flatten(), rowptr, col, **slab)
    with pytest.raises(ValueError, match="1, 2, 4 or 8"):
        agg(torch.zeros((3, 12)), torch.zeros((3, 12)), torch.zeros((3, 4)), rowptr, col, **slab)
    with pytest.raises(ValueError, match="power of two"):
        agg(torch.zeros((3, 24)), torch.zeros((3, 24)), torch.zeros((2, 12)), rowptr, col, **slab)
    with pytest.raises(ValueError, match="power of two"):
        agg(torch.zeros((3, 10)), torch.zeros((3, 10)), torch.zeros((2, 5)), rowptr, col, **slab)
    with pytest.raises(ValueError, match="<= 1024"):
        agg(torch.zeros((3, 2048)), torch.zeros((3, 2048)), torch.zeros((8, 256)), rowptr, col, **slab)
    with pytest.raises(ValueError, match="heads \\* C"):
        agg(x_l, x_r, torch.zeros((2, 4)), rowptr, col, **slab)
    with pytest.raises(ValueError, match="aligned to 4 elements"):
        agg(torch.zeros((3, 17))[:, 1:], x_r, att, rowptr, col, **slab)
    with pytest.raises(ValueError, match="aligned to 4 elements"):
        agg(x_l, torch.zeros((3, 18))[:, :16], att, rowptr, col, **slab)
    with pytest.raises(ValueError, match="out_dtype"):
        agg(x_l, x_r, att, rowptr, col, out_dtype=torch.float16, **slab)
    with pytest.raises(ValueError, match="out must be"):
        agg(x_l, x_r, att, rowptr, col, out=torch.zeros((2, 16)), **slab)
    with pytest.raises(ValueError, match="one row per node"):
        agg(x_l, x_r, att, rowptr[:-1], col, **slab)
    with pytest.raises(ValueError, match="2-D"):
        agg(x_l.double(), x_r.double(), att, rowptr, col, **slab)
    with pytest.raises(RuntimeError, match="requires grad"):
        agg(x_l.clone().requires_grad_(), x_r, att, rowptr, col, **slab)
    with pytest.raises(RuntimeError, match="att requires grad"):
        agg(x_l, x_r, att.clone().requires_grad_(), rowptr, col, **slab)
    with pytest.raises(TypeError, match="fp8"):
        agg(fp8.quantize_e4m3(torch.zeros((3, 16))), x_r, att, rowptr, col, **slab)


def test_gatv2_inference_validates_before_the_device(no_device):
    from salient_plusplus_amd import fp8, inference
    from salient_plusplus_amd.models import GAT, GATv2, GATv2Conv
    x, rowptr, col = torch.zeros((3, 4)), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])
    model = GATv2(4, 8, 3, 2, heads=2)
    for entry in (inference.gatv2_inference, inference.evaluate):
        with pytest.raises(TypeError, match="fp8 feature table"):
            entry(model, fp8.quantize_e4m3(torch.zeros((3, 16))), rowptr, col)
        with pytest.raises(TypeError, match="GATv2"):          # an Fp8Table: out of scope, and the message says so
            entry(model, inference.Fp8Table(fp8.quantize_e4m3(torch.zeros((3, 16)))), rowptr, col)
        with pytest.raises(RuntimeError, match="requires grad"):
            entry(model, x.clone().requires_grad_(), rowptr, col)
        with pytest.raises(ValueError, match="one row per node"):
            entry(model, x, rowptr[:-1], col)
        with pytest.raises(ValueError, match="act_dtype"):
            entry(model, x, rowptr, col, act_dtype=torch.float16)
        with pytest.raises(ValueError, match="rows_per_slab"):
            entry(model, x, rowptr, col, rows_per_slab=0)
        with pytest.raises(ValueError, match="nodes"):
            entry(model, x, rowptr, col, nodes=torch.tensor([[0]]))
        assert model.training                                 # a refused call leaves the mode alone
        with pytest.raises(NotImplementedError, match=r"heads = 3.*\{1, 2, 4, 8\}"):
            entry(GATv2(4, 6, 3, 2, heads=3), x, rowptr, col)
        with pytest.raises(NotImplementedError, match=r"8 \* 256 = 2048.*C = 172 padded to Cp = 256"):
            entry(GATv2(4, 8, 172, 2, heads=8), x, rowptr, col)
        biased = GATv2(4, 8, 3, 2, heads=2)
        biased.convs[0] = GATv2Conv(4, 4, heads=2, bias=True)
        with pytest.raises(NotImplementedError, match="bias=False"):
            entry(biased, x, rowptr, col)
        concat = GATv2(4, 8, 3, 2, heads=2)
        concat.convs[1] = GATv2Conv(8, 3, heads=2, bias=False, concat=True)
        with pytest.raises(NotImplementedError, match="concat=False on the last layer only"):
            entry(concat, x, rowptr, col)
    with pytest.raises(NotImplementedError, match="implemented for GATv2, not GAT"):
        inference.gatv2_inference(GAT(4, 4, 2, 2), x, rowptr, col)
    with pytest.raises(ValueError, match="edge_weight is GCN's"):
        inference.evaluate(model, x, rowptr, col, edge_weight=torch.ones(3))


def test_the_other_entries_still_refuse_gatv2_and_name_the_resident_ones(no_device):
    from salient_plusplus_amd import inference
    from salient_plusplus_amd.models import GATv2
    x, rowptr, col = torch.zeros((3, 4)), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])
    model = GATv2(4, 8, 3, 2, heads=2)
    for call in (lambda: inference.layerwise_inference(model, x, rowptr, col), lambda: model.inference(x, rowptr, col)):
        with pytest.raises(AssertionError, match="before the arguments were refused"):       # valid: it reaches the device
            call()
    for fn, kw in ((inference.field_inference, dict(nodes=torch.tensor([0]))),
                   (inference.field_evaluate, dict(nodes=torch.tensor([0]))),
                   (inference.partitioned_inference, dict(part_offsets=[0, 3], rank=0, peers=inference.LocalPeers(1)))):
        with pytest.raises(NotImplementedError, match=rf"^{fn.__name__}: not built for GATv2.*layerwise_inference.*"
                                                      "evaluate"):
            fn(model, x, rowptr, col, **kw)
    with pytest.raises(NotImplementedError, match="GATv2.*gatv2_inference"):
        inference.field_inference(model, x, rowptr, col, torch.tensor([0]))
    with pytest.raises(NotImplementedError, match="GATv2.*gatv2_inference"):
        inference.field_evaluate(model, x, rowptr, col, nodes=torch.tensor([0]))
    with pytest.raises(NotImplementedError, match="GATv2.*gatv2_inference"):
        inference.partitioned_inference(model, x, rowptr, col, part_offsets=[0, 3], rank=0,
                                        peers=inference.LocalPeers(1))


def test_gatv2_method_and_both_entries_raise_the_same(no_device):
    """layerwise_inference takes a GATv2 model with gatv2_inference's checks (each under its own name), and the method
    is layerwise_inference"""
    from salient_plusplus_amd import inference
    from salient_plusplus_amd.models import GATv2
    x, rowptr, col = torch.zeros((3, 4)), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])
    model = GATv2(4, 8, 3, 2, heads=2)
    bad = [dict(act_dtype=torch.float16), dict(rows_per_slab=0), dict(nodes=torch.tensor([0.5]))]
    for model_, kw in [(model, k) for k in bad] + [(GATv2(4, 6, 3, 2, heads=3), {}), (GATv2(4, 8, 172, 2, heads=8), {})]:
        seen = []
        for call in (lambda: inference.layerwise_inference(model_, x, rowptr, col, **kw),
                     lambda: model_.inference(x, rowptr, col, **kw),
                     lambda: inference.gatv2_inference(model_, x, rowptr, col, **kw)):
            with pytest.raises((ValueError, NotImplementedError)) as info:
                call()
            seen.append((type(info.value), str(info.value)))
        assert seen[0] == seen[1] and seen[0][1].startswith("layerwise_inference: ")
        assert seen[2] == (seen[0][0], "gatv2_inference: " + seen[0][1][len("layerwise_inference: "):])
    with pytest.raises(TypeError, match="^layerwise_inference: x is an Fp8Table.*GATv2"):
        from salient_plusplus_amd import fp8
        model.inference(inference.Fp8Table(fp8.quantize_e4m3(torch.zeros((3, 16)))), rowptr, col)


# ---------------------------------------------------------------------------------------------------- the helper's own check
def _cg():
    """the helper is checked at the kernel's own chunk, so that the self-check follows C_g if it ever changes"""
    from salient_plusplus_amd.inference import graph_gatv2_chunk
    _lib()
    return graph_gatv2_chunk()


def _case(H, Cc, regime="model", slope=None):
    import gatv2_f64
    import graph_gatv2_f64 as gg
    hop = gg.planted_graph(_cg())
    x_l, x_r, att, _g = gatv2_f64.inputs(regime, hop, H, Cc, torch.float32)
    return gg, hop, x_l, x_r, att, gatv2_f64.SLOPES[0] if slope is None else slope


def test_the_planted_graph_has_the_rows_it_promises():
    import graph_gatv2_f64 as gg
    CG = _cg()
    hop = gg.planted_graph(CG)
    raw = hop.raw.tolist()
    assert raw[:9] == [0, 1, 63, 64, 65, CG, CG + 1, 3 * CG + 7, 9 * CG] and raw[gg.ISOLATED] == 0
    assert not bool((hop.col == gg.ISOLATED).any()) and hop.T == gg.N
    b = int(hop.rowptr[gg.EMPTY_CHUNK_ROW])
    assert hop.col[b + CG:b + 2 * CG].tolist() == [gg.EMPTY_CHUNK_ROW] * CG and raw[gg.EMPTY_CHUNK_ROW] > 2 * CG
    assert int(hop.kept[gg.ONLY_SELF]) == 0 and raw[gg.ONLY_SELF] == 3
    assert int(hop.col[hop.rowptr[12] + CG]) == 12
    assert int((hop.kept < hop.raw).sum()) >= 6                # rows with diagonal entries
    row8 = hop.col[hop.rowptr[8]:hop.rowptr[9]]
    assert row8.unique().numel() < row8.numel()                # duplicates


def test_the_two_float64_statements_agree():
    gg, hop, x_l, x_r, att, slope = _case(4, 16)
    CG = _cg()
    ref = gg.reference(hop, x_l, x_r, att, slope, CG)
    rows = gg.plain_rows(hop.rowptr, hop.col, x_l, x_r, att, slope)
    assert float((ref.out - rows).abs().max()) < 1e-13
    assert bool((ref.b_out > 0).all()) and float(ref.b_out.max()) < 1e-4       # (|x_l| is O(1): the bounds bind)
    assert ref.M[:13].tolist() == [0, 0, 0, 0, 1, 0, 1, 3, 8, 2, 0, 0, 1] and float(ref.M[13:].max()) == 0


@pytest.mark.parametrize("regime", ["model", "wide", "equal"])
def test_a_correct_chunked_fp32_computation_stays_inside_every_bound(regime):
    import gatv2_f64
    gg, hop, x_l, x_r, att, slope = _case(4, 16, regime)
    CG = _cg()
    ref = gg.reference(hop, x_l, x_r, att, slope, CG)
    got = gg.chunked_fp32(hop.rowptr, hop.col, x_l, x_r, att, slope, CG)
    ratio, where = gatv2_f64.worst(got, ref.out, ref.b_out, hop)
    print(f"chunked fp32, {regime}: largest err / bound {ratio:.3f} at {where}")
    assert ratio <= 1.0, where


@pytest.mark.parametrize("fault", ["no_rescale", "self_everywhere", "keep_diag"])
def test_planted_faults_leave_the_bounds(fault):
    import gatv2_f64
    gg, hop, x_l, x_r, att, slope = _case(4, 16)
    CG = _cg()
    ref = gg.reference(hop, x_l, x_r, att, slope, CG)
    got = gg.chunked_fp32(hop.rowptr, hop.col, x_l, x_r, att, slope, CG, fault=fault)
    ratio, where = gatv2_f64.worst(got, ref.out, ref.b_out, hop)
    print(f"{fault}: largest err / bound {ratio:.3e} at {where}")
    assert ratio > 100.0, (fault, where)
    bad = ((got.double() - ref.out).abs() > ref.b_out).flatten(1).any(1)
    long_rows, diag_rows = hop.raw > CG, hop.kept < hop.raw
    assert not bool((bad & ~(diag_rows if fault == "keep_diag" else long_rows)).any())     # and only where it can show


# ------------------------------------------------------------------------------------------------------ the padding identity
@pytest.mark.parametrize("H,Cc", [(1, 5), (4, 5), (2, 47), (1, 172)])
def test_zero_padded_channels_change_nothing(H, Cc):
    """what ``_gatv2_layer`` relies on: zero rows of W_l / W_r (here: zero columns of the projected rows) and zero
    columns of att, sliced away afterwards, give the unpadded result -- ``_gatv2_reference`` on both, float64, so that
    the comparison is of the formula and not of a summation order"""
    from salient_plusplus_amd.inference import _gatv2_pad
    from salient_plusplus_amd.models import _gatv2_reference
    Cp = _gatv2_pad(Cc)
    assert Cp >= Cc and Cp % 4 == 0 and (Cp // 4) & (Cp // 4 - 1) == 0 and (Cp == 4 or Cp // 2 < Cc)
    g = torch.Generator().manual_seed(Cc)
    n = 40
    deg = torch.randint(0, 9, (n,), generator=g)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, n, (int(rowptr[-1]),), generator=g)
    x_l, x_r = (torch.randn((n, H, Cc), generator=g, dtype=torch.float64) for _ in range(2))
    att = torch.randn((H, Cc), generator=g, dtype=torch.float64)
    want = _gatv2_reference(x_l, x_r, att, rowptr, col, 0.2)
    pl, pr, pa = torch.zeros((n, H, Cp), dtype=torch.float64), torch.zeros((n, H, Cp), dtype=torch.float64), \
        torch.zeros((H, Cp), dtype=torch.float64)
    pl[:, :, :Cc], pr[:, :, :Cc], pa[:, :Cc] = x_l, x_r, att
    got = _gatv2_reference(pl, pr, pa, rowptr, col, 0.2)
    assert torch.equal(got[:, :, Cc:], torch.zeros_like(got[:, :, Cc:]))
    # torch may add the Cp terms of a logit in another order than the C terms: float64 rounding, nothing more.  A logit
    # moves by at most (Cp + 2) 2^-53 sum_c |att lr| <= 258 * 1.2e-16 * 172 * 5 = 2.7e-11, a weight relatively by as
    # much, an output by that times twice max|x_l| (< 10): below 1e-9 absolute.
    torch.testing.assert_close(got[:, :, :Cc], want, rtol=0, atol=1e-9)


def test_pad_widths():
    from salient_plusplus_amd.inference import _gatv2_pad
    assert [_gatv2_pad(c) for c in (1, 4, 5, 8, 9, 16, 32, 47, 48, 64, 65, 172, 256)] == \
        [4, 4, 8, 8, 16, 16, 32, 64, 64, 64, 128, 256, 256]
