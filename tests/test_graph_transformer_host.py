"""CPU-only: the host side of exact layer-wise GraphTransformer inference (spp.h f3z) -- the exported entries and the
ctypes layout of spp_graph_transformer_desc against the header, the refusals of spp_graph_transformer_forward that need
no device in the header's order, the argument validation of inference.graph_transformer_aggregate /
layerwise_inference / transformer_inference / evaluate before any device call, the entries that refuse a
GraphTransformer (Fp8Table, field, partitioned) with the one message that names the two that work, and the float64
helper's own check (tests/graph_transformer_f64.py: the two float64 statements agree, a correct chunked fp32 computation
stays inside every bound, three planted faults leave them)."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_FAKE = 0x10000
SPP_OK, SPP_ERR_INVALID = 0, -1                               # spp_status (include/spp.h)
ENTRIES = ("spp_graph_transformer_forward", "spp_graph_transformer_chunk", "spp_graph_transformer_workspace_bytes")


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


def test_library_exports_the_graph_transformer_entries():
    from salient_plusplus_amd import build
    from salient_plusplus_amd.inference import graph_transformer_chunk, graph_transformer_workspace_bytes
    nat, L = _lib()
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name) and name in nat.SIGNATURES
        assert re.search(rf"\b{name}\(", header), name
    assert "graph_transformer.hip" in build.SOURCES and "transformer_conv.hip" in build.SOURCES
    assert L.spp_abi_version() == 6
    assert graph_transformer_chunk() >= 32
    counts = (0, 1, 2, 7, 1000, 1 << 20, 1 << 33)
    sizes = [graph_transformer_workspace_bytes(T) for T in counts]
    assert sizes == sorted(sizes) and sizes[0] >= 16 and all(b >= 8 * T for b, T in zip(sizes, counts))


def test_graph_transformer_desc_has_the_fields_and_order_of_the_header():
    """the field names in the header's order, then sizeof and every offset cross-checked by compiling the header"""
    from salient_plusplus_amd import _native as nat
    names = [n for n, _t in nat.GraphTransformerDesc._fields_]
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    body = re.search(r"typedef struct spp_graph_transformer_desc \{(.*?)\} spp_graph_transformer_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == names
    offs = ", ".join(f"offsetof(spp_graph_transformer_desc, {n})" for n in names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "spp.h"\n'
            "int main(void) { size_t v[] = { sizeof(spp_graph_transformer_desc), " + offs + " };\n"
            "  for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf(\"%zu \", v[i]);\n  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(nat.GraphTransformerDesc)] + [getattr(nat.GraphTransformerDesc, n).offset for n in names]


def _desc(nat, **over):
    """a descriptor that passes every check; the pointers are never dereferenced by a refusal (nothing is enqueued)"""
    kw = dict(x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, heads=2, relu=0, rowptr_dev=_FAKE, col_dev=_FAKE,
              q_dev=_FAKE, q_stride_elems=16, k_dev=_FAKE, k_stride_elems=32, v_dev=_FAKE + 64, v_stride_elems=32, x_rows=10,
              C=8, target_row0=0, target_ids_dev=None, num_targets=4, out_dev=_FAKE, out_stride_elems=0, skip_dev=_FAKE,
              skip_stride_elems=16, scale=0.25)
    kw.update(over)
    return nat.GraphTransformerDesc(**kw)


# in the header's order: f3w's through check_common, then the strides / alignment of q, v, skip, last the scale.  Each
# case breaks ONE thing and also everything that is checked behind it stays valid, so the word pins the check that fired;
# the order itself is pinned below by breaking two at once.
REFUSALS = [
    ("heads = 3", dict(heads=3, C=4), {}, b"heads"),
    ("C = 6", dict(C=6), {}, b"C %"),
    ("C = 12: C / 4 no power of two", dict(C=12), {}, b"power of two"),
    ("D = 2048", dict(heads=8, C=256), {}, b"1024"),
    ("unknown x_elem", dict(x_elem=77), {}, b"x_elem"),
    ("fp16 output", dict(out_elem="F16"), {}, b"out_elem"),
    ("fp8 rows", dict(x_elem="FP8_E4M3"), {}, b"fp8"),
    ("both target forms", dict(target_ids_dev=_FAKE), {}, b"not both"),
    ("neither target form", dict(target_row0=-1), {}, b"target_row0"),
    ("slab outside the graph", dict(target_row0=8, num_targets=4), {}, b"target_row0"),
    ("output stride smaller than the row", dict(out_stride_elems=8), {}, b"out_stride_elems"),
    ("missing workspace", {}, dict(ws=None), b"spp_graph_transformer_workspace_bytes"),
    ("small workspace", {}, dict(bytes=8), b"workspace"),
    ("NULL q", dict(q_dev=None), {}, b"NULL"),
    ("NULL v", dict(v_dev=None), {}, b"NULL"),
    ("k stride smaller than the row", dict(k_stride_elems=12), {}, b"k_stride_elems"),
    ("misaligned output base", dict(out_dev=_FAKE + 4), {}, b"out_dev"),
    ("q stride smaller than the row", dict(q_stride_elems=12), {}, b"q_stride_elems"),
    ("v stride smaller than the row", dict(v_stride_elems=12), {}, b"v_stride_elems"),
    ("skip stride smaller than the row", dict(skip_stride_elems=12), {}, b"skip_stride_elems"),
    ("misaligned k base", dict(k_dev=_FAKE + 4), {}, b"misaligned"),
    ("misaligned q base", dict(q_dev=_FAKE + 4), {}, b"misaligned"),
    ("q stride no multiple of 4", dict(q_stride_elems=18), {}, b"misaligned"),
    ("misaligned skip base", dict(skip_dev=_FAKE + 4), {}, b"misaligned"),
    ("scale = 0", dict(scale=0.0), {}, b"scale"),
    ("scale < 0", dict(scale=-1.0), {}, b"scale"),
    ("scale = inf", dict(scale=float("inf")), {}, b"scale"),
    ("scale = nan", dict(scale=float("nan")), {}, b"scale"),
]


def _call(nat, L, over, call):
    over = {k: getattr(nat, "SPP_ELEM_" + v) if isinstance(v, str) else v for k, v in over.items()}
    d = _desc(nat, **over)
    ws = call.get("ws", _FAKE)
    nbytes = call.get("bytes", int(L.spp_graph_transformer_workspace_bytes(d.num_targets)))
    return L.spp_graph_transformer_forward(ctypes.byref(d), ctypes.c_void_p(ws), nbytes, None)


@pytest.mark.parametrize("what,over,call,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_refuses_before_anything_is_enqueued(what, over, call, word):
    nat, L = _lib()
    assert _call(nat, L, over, call) == SPP_ERR_INVALID, what
    assert word in L.spp_last_error(), (what, L.spp_last_error())


def test_entry_refuses_in_the_headers_order():
    """two broken things at once: the earlier check of the header's list is the one that speaks"""
    nat, L = _lib()
    pairs = [(dict(heads=3, scale=0.0), b"heads"), (dict(x_elem=77, q_stride_elems=12), b"x_elem"),
             (dict(target_row0=-1, scale=-1.0), b"target_row0"), (dict(k_stride_elems=12, q_stride_elems=12), b"k_stride"),
             (dict(q_stride_elems=12, q_dev=_FAKE + 4), b"q_stride_elems"), (dict(skip_dev=_FAKE + 4, scale=0.0), b"misaligned")]
    for over, word in pairs:
        assert _call(nat, L, over, {}) == SPP_ERR_INVALID and word in L.spp_last_error(), (over, L.spp_last_error())
    assert L.spp_graph_transformer_forward(None, ctypes.c_void_p(_FAKE), 1 << 20, None) == SPP_ERR_INVALID
    assert b"NULL descriptor" in L.spp_last_error()
    # T == 0: SPP_OK without touching a device or a buffer, even with a scale that a non-empty call refuses
    d = _desc(nat, num_targets=0, scale=0.0, q_dev=None)
    assert L.spp_graph_transformer_forward(ctypes.byref(d), ctypes.c_void_p(_FAKE), 1 << 10, None) == SPP_OK


def _tiny(H=2, Cc=8):
    x = torch.zeros((3, H * Cc))
    return x, x.clone(), x.clone(), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])


def test_graph_transformer_aggregate_validates_its_arguments(no_device):
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd.inference import graph_transformer_aggregate as agg
    q, k, v, rowptr, col = _tiny()
    kw = dict(heads=2, scale=0.35, row0=0, num_targets=3)
    with pytest.raises(AssertionError, match="before the arguments were refused"):       # CPU tensors: valid up to the device
        agg(q, k, v, rowptr, col, **kw)
    with pytest.raises(ValueError, match="not both"):
        agg(q, k, v, rowptr, col, target_ids=torch.tensor([0]), **kw)
    with pytest.raises(ValueError, match="either as a slab"):
        agg(q, k, v, rowptr, col, heads=2, scale=0.35)
    with pytest.raises(ValueError, match="leaves the graph"):
        agg(q, k, v, rowptr, col, heads=2, scale=0.35, row0=2, num_targets=2)
    with pytest.raises(ValueError, match="target_ids"):
        agg(q, k, v, rowptr, col, heads=2, scale=0.35, target_ids=torch.tensor([0], dtype=torch.int32))
    with pytest.raises(ValueError, match="k must have q's shape"):
        agg(q, k[:, :8], v, rowptr, col, **kw)
    with pytest.raises(ValueError, match="v must have q's shape and dtype"):
        agg(q, k, v.half(), rowptr, col, **kw)
    with pytest.raises(ValueError, match="skip must have q's shape and dtype"):
        agg(q, k, v, rowptr, col, skip=q.bfloat16(), **kw)
    with pytest.raises(ValueError, match="2-D"):
        agg(q.double(), k.double(), v.double(), rowptr, col, **kw)
    for bad in (3, 16, True, 2.0):
        with pytest.raises(ValueError, match="1, 2, 4 or 8"):
            agg(q, k, v, rowptr, col, **dict(kw, heads=bad))
    with pytest.raises(ValueError, match="power of two"):
        agg(*(torch.zeros((3, 24)) for _ in range(3)), rowptr, col, **kw)
    with pytest.raises(ValueError, match="power of two"):
        agg(*(torch.zeros((3, 10)) for _ in range(3)), rowptr, col, **kw)
    with pytest.raises(ValueError, match=r"8 \* 256 = 2048 <= 1024"):
        agg(*(torch.zeros((3, 2048)) for _ in range(3)), rowptr, col, **dict(kw, heads=8))
    for bad in (0.0, -0.5, float("inf"), float("nan"), None, True):
        with pytest.raises(ValueError, match="scale must be a finite positive number"):
            agg(q, k, v, rowptr, col, **dict(kw, scale=bad))
    with pytest.raises(ValueError, match="rows of q must be aligned to 4 elements"):
        agg(torch.zeros((3, 17))[:, 1:], k, v, rowptr, col, **kw)
    with pytest.raises(ValueError, match="rows of v must be aligned to 4 elements"):
        agg(q, k, torch.zeros((3, 18))[:, :16], rowptr, col, **kw)
    with pytest.raises(ValueError, match="rows of skip must be aligned to 4 elements"):
        agg(q, k, v, rowptr, col, skip=torch.zeros((3, 18))[:, :16], **kw)
    with pytest.raises(ValueError, match="out_dtype"):
        agg(q, k, v, rowptr, col, out_dtype=torch.float16, **kw)
    with pytest.raises(ValueError, match="out must be"):
        agg(q, k, v, rowptr, col, out=torch.zeros((2, 16)), **kw)
    with pytest.raises(ValueError, match="one row per node"):
        agg(q, k, v, rowptr[:-1], col, **kw)
    with pytest.raises(RuntimeError, match="k requires grad"):
        agg(q, k.clone().requires_grad_(), v, rowptr, col, **kw)
    with pytest.raises(TypeError, match="fp8"):
        agg(fp8.quantize_e4m3(torch.zeros((3, 16))), k, v, rowptr, col, **kw)
    kv = torch.zeros((3, 32))                                  # the halves of one matrix are valid rows
    with pytest.raises(AssertionError, match="before the arguments were refused"):
        agg(q, kv[:, :16], kv[:, 16:], rowptr, col, skip=q, **kw)


def test_the_resident_entries_validate_before_the_device(no_device):
    from salient_plusplus_amd import fp8, inference
    from salient_plusplus_amd.models import GAT, GraphTransformer, TransformerConv
    x, rowptr, col = torch.zeros((3, 4)), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])
    model = GraphTransformer(4, 8, 3, 2, heads=2)
    assert not hasattr(model, "inference") and not hasattr(GraphTransformer, "inference")
    assert "batch-wise" in GraphTransformer.__doc__ and "inference.layerwise_inference(model, ...)" in GraphTransformer.__doc__
    for entry in (inference.layerwise_inference, inference.transformer_inference, inference.evaluate):
        name = entry.__name__
        with pytest.raises(AssertionError, match="before the arguments were refused"):   # valid: it reaches the device
            entry(model, x, rowptr, col)
        with pytest.raises(TypeError, match="fp8 feature table"):
            entry(model, fp8.quantize_e4m3(torch.zeros((3, 16))), rowptr, col)
        with pytest.raises(TypeError, match=rf"^{name}: x is an Fp8Table.*GraphTransformer.*layerwise_inference.*evaluate"):
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
        with pytest.raises(NotImplementedError, match=rf"^{name}: layer 0 has heads = 3.*\{{1, 2, 4, 8\}}"):
            entry(GraphTransformer(4, 6, 3, 2, heads=3), x, rowptr, col)
        with pytest.raises(NotImplementedError, match=r"layer 1 .*8 \* 256 = 2048.*C = 172 padded to Cp = 256"):
            entry(GraphTransformer(4, 8, 172, 2, heads=8), x, rowptr, col)
        with pytest.raises(NotImplementedError, match=r"layer 0 .*2 \* 1024 = 2048.*C = 600 padded to Cp = 1024"):
            entry(GraphTransformer(4, 1200, 3, 2, heads=2), x, rowptr, col)
        concat = GraphTransformer(4, 8, 3, 2, heads=2)
        concat.convs[1] = TransformerConv(8, 3, heads=2, concat=True)
        with pytest.raises(NotImplementedError, match="concat=False on the last layer only"):
            entry(concat, x, rowptr, col)
    for entry in (inference.layerwise_inference, inference.evaluate):
        with pytest.raises(ValueError, match="edge_weight is GCN's.*GraphTransformer has no weighted aggregation"):
            entry(model, x, rowptr, col, edge_weight=torch.ones(3))
    with pytest.raises(NotImplementedError, match="^transformer_inference: implemented for GraphTransformer, not GAT"):
        inference.transformer_inference(GAT(4, 4, 2, 2), x, rowptr, col)
    with pytest.raises(NotImplementedError, match="^layerwise_inference: implemented for SAGE, GIN, GAT, "
                                                  "SAGEResInception, GCN and GATv2, not Linear$"):
        inference.layerwise_inference(torch.nn.Linear(2, 2), x, rowptr, col)


def test_the_other_entries_refuse_a_graph_transformer_with_one_message(no_device):
    from salient_plusplus_amd import inference
    from salient_plusplus_amd.models import GraphTransformer
    x, rowptr, col = torch.zeros((3, 4)), torch.tensor([0, 1, 2, 3]), torch.tensor([0, 1, 2])
    model = GraphTransformer(4, 8, 3, 2, heads=2, beta=True)
    said = set()
    for fn, kw in ((inference.field_inference, dict(nodes=torch.tensor([0]))),
                   (inference.field_evaluate, dict(nodes=torch.tensor([0]))),
                   (inference.partitioned_inference, dict(part_offsets=[0, 3], rank=0, peers=inference.LocalPeers(1))),
                   (inference.partitioned_evaluate, dict(part_offsets=[0, 3], rank=0, peers=inference.LocalPeers(1))),
                   (inference.partitioned_layerwise_inference,
                    dict(part_offsets=[0, 3], rank=0, peers=inference.LocalPeers(1)))):
        with pytest.raises(NotImplementedError, match=r"not built for GraphTransformer.*inference\.layerwise_inference.*"
                                                      r"inference\.evaluate") as info:
            fn(model, x, rowptr, col, **kw)
        said.add(str(info.value).split(": ", 1)[1])
    assert len(said) == 1                                     # one message, whoever refuses
    assert said.pop().split(": ", 1)[1] == inference._TRANSFORMER_RESIDENT


# ---------------------------------------------------------------------------------------------------- the helper's own check
def _cg():
    """the helper is checked at the kernel's own chunk, so that the self-check follows C_g if it ever changes"""
    from salient_plusplus_amd.inference import graph_transformer_chunk
    _lib()
    return graph_transformer_chunk()


def _case(H, Cc, regime="model"):
    import graph_transformer_f64 as gt
    import transformer_f64 as tf
    CG = _cg()
    ent = gt.planted_graph(CG, gt.hub_length(H * Cc, CG))
    q, k, v, skip = gt.inputs(regime, ent, H, Cc, torch.float32)
    return gt, ent, q, k, v, skip, tf.scale32(Cc), CG


def test_the_planted_graph_has_the_rows_it_promises():
    import graph_transformer_f64 as gt
    CG = _cg()
    for D in (4, 64, 1024):
        ent = gt.planted_graph(CG, gt.hub_length(D, CG))
        raw, row = ent.raw.tolist(), lambda t: ent.col_raw[ent.rowptr[t]:ent.rowptr[t + 1]].tolist()
        assert [raw[t] for t in (gt.EMPTY, gt.ISOLATED, gt.ONE, gt.EXACT, gt.PLUS_ONE, gt.CHUNK, gt.DOUBLED, gt.MID)] == \
            [0, 0, 1, CG, CG + 1, CG, 2 * CG, 3 * CG + 7]
        assert not bool((ent.col_raw == gt.ISOLATED).any()) and ent.T == gt.N
        assert row(gt.ONLY_SELF) == [gt.ONLY_SELF] and row(gt.DOUBLED) == row(gt.CHUNK) * 2
        rep = row(gt.REPEATS)
        assert rep[0] == rep[1] and gt.REPEATS in rep
        lpr = min(64, D // 4)
        assert raw[gt.HUB] > 2 * (256 // lpr) * CG and row(gt.HUB) == sorted(row(gt.HUB))
        assert row(gt.BAD_COL)[1] == gt.OUTSIDE >= gt.N and int((ent.col_raw != ent.col).sum()) == 1
        assert int(ent.col[ent.rowptr[gt.BAD_COL] + 1]) == 0
    assert gt.hub_length(4, CG) > 32768


def test_the_two_float64_statements_agree_on_the_small_rows():
    gt, ent, q, k, v, skip, scale, CG = _case(4, 16)
    ref = gt.reference(ent, q, k, v, scale, CG)
    small = [t for t in range(gt.N) if int(ent.raw[t]) <= 4 * CG]
    assert len(small) >= gt.N - 2 and gt.MID in small and gt.BAD_COL in small
    rows = gt.plain_rows(ent.rowptr, ent.col_raw, q, k, v, scale, rows=small)
    assert float((ref.out[small] - rows).abs().max()) < 1e-13
    assert torch.equal(ref.out[gt.EMPTY], torch.zeros(4, 16, dtype=torch.float64)) and float(ref.b_out[gt.EMPTY].max()) == 0
    # |v| is O(1), so the bounds bind: a short row's is a few EXP0, the hub's grows with its merges (M EXP0 a weight)
    assert float(ref.b_out[small].max()) < 1e-4 and float(ref.b_out.max()) < (int(ref.M[gt.HUB]) + 70) * 2e-6
    planted = {gt.PLUS_ONE: 1, gt.DOUBLED: 1, gt.MID: 3, gt.EXACT: 0, gt.CHUNK: 0, gt.EMPTY: 0}
    assert all(int(ref.M[t]) == m for t, m in planted.items()) and int(ref.M[gt.HUB]) == -(-int(ent.raw[gt.HUB]) // CG) - 1
    with_tail = gt.reference(ent, q, k, v, scale, CG, skip=skip, relu=True)
    assert torch.equal(with_tail.out, torch.clamp(ref.out + skip.double(), min=0))
    assert bool((with_tail.b_out >= ref.b_out).all()) and bool((with_tail.b_out[gt.EMPTY] > 0).any())


@pytest.mark.parametrize("tail", [False, True], ids=["bare", "skip_relu"])
@pytest.mark.parametrize("regime", ["model", "wide", "equal", "rising", "falling"])
def test_a_correct_chunked_fp32_computation_stays_inside_every_bound(regime, tail):
    import transformer_f64 as tf
    gt, ent, q, k, v, skip, scale, CG = _case(4, 16, regime)
    kw = dict(skip=skip, relu=True) if tail else {}
    ref = gt.reference(ent, q, k, v, scale, CG, **kw)
    got = gt.chunked_fp32(ent.rowptr, ent.col_raw, q, k, v, scale, CG, **kw)
    ratio, where = tf.worst(got, ref.out, ref.b_out)
    print(f"chunked fp32, {regime}{' + skip + relu' if tail else ''}: largest err / bound {ratio:.3f} at {where}")
    assert ratio <= 1.0, where


@pytest.mark.parametrize("fault,regime", [("merge_order", "rising"), ("merge_order", "falling"), ("dropped_chunk", "model"),
                                          ("dropped_chunk", "rising"), ("no_rescale", "rising")])
def test_planted_faults_leave_the_bounds(fault, regime):
    import transformer_f64 as tf
    gt, ent, q, k, v, skip, scale, CG = _case(4, 16, regime)
    ref = gt.reference(ent, q, k, v, scale, CG, skip=skip)
    got = gt.chunked_fp32(ent.rowptr, ent.col_raw, q, k, v, scale, CG, skip=skip, fault=fault)
    ratio, where = tf.worst(got, ref.out, ref.b_out)
    print(f"{fault} ({regime}): largest err / bound {ratio:.3e} at {where}")
    assert ratio > 100.0, (fault, where)
    bad = ((got.double() - ref.out).abs() > ref.b_out).flatten(1).any(1)
    assert not bool((bad & (ent.raw <= CG)).any())            # and only where it can show: in rows of several chunks


# ------------------------------------------------------------------------------------------------------ the padding identity
@pytest.mark.parametrize("H,Cc", [(1, 5), (4, 5), (2, 47)])
def test_zero_padded_channels_change_nothing(H, Cc):
    """what ``_transformer_layer`` relies on: zero weight rows and zero bias entries per head (here: zero columns of the
    projected rows), sliced away afterwards, give the unpadded result when the scale stays 1 / sqrt(Cc) of the UNPADDED
    width -- ``_transformer_reference`` on both, in float64"""
    from salient_plusplus_amd.inference import _gatv2_pad
    from salient_plusplus_amd.models import _transformer_reference
    Cp = _gatv2_pad(Cc)
    g = torch.Generator().manual_seed(Cc)
    n = 40
    deg = torch.randint(0, 9, (n,), generator=g)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, n, (int(rowptr[-1]),), generator=g)
    q, k, v = (torch.randn((n, H, Cc), generator=g, dtype=torch.float64) for _ in range(3))
    scale = 1.0 / float(Cc) ** 0.5
    want = _transformer_reference(q, k, v, rowptr, col, scale)
    pq, pk, pv = (torch.zeros((n, H, Cp), dtype=torch.float64) for _ in range(3))
    pq[:, :, :Cc], pk[:, :, :Cc], pv[:, :, :Cc] = q, k, v
    got = _transformer_reference(pq, pk, pv, rowptr, col, scale)
    assert torch.equal(got[:, :, Cc:], torch.zeros_like(got[:, :, Cc:]))
    # torch may add the Cp terms of a logit in another order than the Cc terms: float64 rounding of a dot product of
    # O(10) magnitude, 1e-14, times |v| < 10 twice: far below 1e-9
    torch.testing.assert_close(got[:, :, :Cc], want, rtol=0, atol=1e-9)
