"""CPU-only: edge-weighted aggregation and GCN (spp.h f3r) without a device -- the four descriptors against the header,
every refusal the entries make before a launch, the Python argument checks, GCN's state dict against the reference
tree, get_model_type("gcn"), and the plain-torch restatements _weighted_reference / _gcn_norm_reference and the CPU
GCNConv / GCN against dense float64 formulas."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SPP_OK, SPP_ERR_INVALID = 0, -1
_FAKE = 0x7F0000001000                                   # never dereferenced: every refusal comes before a launch
ENTRIES = ("spp_agg_weighted_forward", "spp_agg_weighted_backward", "spp_agg_weighted_wgrad", "spp_gcn_norm",
           "spp_agg_weighted_backward_workspace_bytes")


def _lib():
    from salient_plusplus_amd import _native as nat
    return nat, nat.load()


@pytest.mark.parametrize("struct,cname", [("AggWeightedFwdDesc", "spp_agg_weighted_fwd_desc"),
                                          ("AggWeightedBwdDesc", "spp_agg_weighted_bwd_desc"),
                                          ("AggWeightedWgradDesc", "spp_agg_weighted_wgrad_desc"),
                                          ("GcnNormDesc", "spp_gcn_norm_desc")])
def test_descriptor_layout_matches_header(tmp_path, struct, cname):
    """sizeof and every field offset, in the header's order, cross-checked by compiling the header with gcc"""
    nat, _ = _lib()
    cls = getattr(nat, struct)
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    body = header[header.index("typedef struct %s {" % cname):header.index("} %s;" % cname)]
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body))
    assert names == [f[0] for f in cls._fields_]
    offs = ", ".join(f"offsetof({cname}, {n})" for n in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spp.h"\n'
                   "int main(void) { size_t v[] = { sizeof(%s), %s };\n"
                   "  for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf(\"%%zu\\n\", v[i]);\n  return 0; }\n"
                   % (cname, offs))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n in names]


def test_library_exports_the_entries_and_the_abi_version_stays():
    nat, L = _lib()
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name) and name in nat.SIGNATURES and f" {name}(" in header, name
    assert "#define SPP_ABI_VERSION 6" in header
    assert "aggregate_weighted.hip" in __import__("salient_plusplus_amd.build", fromlist=["SOURCES"]).SOURCES


def _fwd(nat, **over):
    kw = dict(source=nat.SPP_AGG_DENSE, x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, rowptr_dev=_FAKE,
              col_dev=_FAKE, num_targets=5, num_edges=12, x_dev=_FAKE, x_stride_elems=8, x_rows=0, n_id_dev=None, F=8,
              w_dev=_FAKE, self_w_dev=_FAKE, out_dev=_FAKE, out_stride_elems=0)
    kw.update(over)
    return nat.AggWeightedFwdDesc(**kw)


def _bwd(nat, **over):
    kw = dict(grad_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, rowptr_dev=_FAKE, col_dev=_FAKE, num_targets=5,
              num_sources=9, num_edges=12, grad_out_dev=_FAKE, grad_out_stride_elems=0, F=8, w_dev=_FAKE,
              self_w_dev=_FAKE, grad_x_dev=_FAKE)
    kw.update(over)
    return nat.AggWeightedBwdDesc(**kw)


def _wgrad(nat, **over):
    kw = dict(source=nat.SPP_AGG_DENSE, x_elem=nat.SPP_ELEM_F32, grad_elem=nat.SPP_ELEM_F32, rowptr_dev=_FAKE,
              col_dev=_FAKE, num_targets=5, num_edges=12, x_dev=_FAKE, x_stride_elems=8, x_rows=0, n_id_dev=None, F=8,
              grad_out_dev=_FAKE, grad_out_stride_elems=0, grad_w_dev=_FAKE, grad_self_w_dev=_FAKE)
    kw.update(over)
    return nat.AggWeightedWgradDesc(**kw)


def _norm(nat, **over):
    kw = dict(fill=1, rowptr_dev=_FAKE, col_dev=_FAKE, num_targets=5, num_sources=9, num_edges=12, w_dev=_FAKE,
              dinv_dev=_FAKE, coef_dev=_FAKE, self_coef_dev=_FAKE)
    kw.update(over)
    return nat.GcnNormDesc(**kw)


def _rows_cases(nat):
    """the refusals the forward and the weight gradient share: codes, sizes and the row source"""
    return {
        "unknown source": (dict(source=3), b"source"),
        "negative source": (dict(source=-1), b"source"),
        "unknown x code": (dict(x_elem=7), b"element code"),
        "fp8 rows": (dict(x_elem=nat.SPP_ELEM_FP8_E4M3), b"fp8"),
        "negative T": (dict(num_targets=-1), b"negative"),
        "negative F": (dict(F=-8), b"negative"),
        "negative E": (dict(num_edges=-1), b"negative"),
        "T * F out of range": (dict(num_targets=1 << 60), b"out of range"),
        "row stride": (dict(x_stride_elems=7), b"row stride"),
        "NULL rowptr": (dict(rowptr_dev=None), b"NULL"),
        "NULL col": (dict(col_dev=None), b"NULL"),
        "NULL x": (dict(x_dev=None), b"NULL"),
        "table without ids": (dict(source=nat.SPP_AGG_TABLE, x_rows=10), b"NULL"),
        "empty table": (dict(source=nat.SPP_AGG_TABLE, n_id_dev=_FAKE, x_rows=0), b"empty table"),
        "row references without addresses": (dict(source=nat.SPP_AGG_ROWS, n_id_dev=None), b"NULL"),
        "misaligned x": (dict(x_dev=_FAKE + 1, x_elem=nat.SPP_ELEM_BF16), b"misaligned"),
    }


def _refused(L, name, call, cases):
    for what, (over, text) in cases.items():
        assert call(over) == SPP_ERR_INVALID, (name, what)
        msg = L.spp_last_error()
        assert name.encode() in msg and text in msg, (name, what, msg)


def test_forward_refusals_come_before_any_launch():
    nat, L = _lib()
    cases = dict(_rows_cases(nat))
    cases.update({
        "fp16 output": (dict(out_elem=nat.SPP_ELEM_F16), b"element code"),
        "fp8 output": (dict(out_elem=nat.SPP_ELEM_FP8_E4M3), b"element code"),
        "output stride": (dict(out_stride_elems=7), b"output stride"),
        "negative output stride": (dict(out_stride_elems=-1), b"output stride"),
        "NULL out": (dict(out_dev=None), b"NULL"),
        "NULL w": (dict(w_dev=None), b"NULL"),
        "misaligned out": (dict(out_dev=_FAKE + 2), b"misaligned"),
        "misaligned w": (dict(w_dev=_FAKE + 2), b"misaligned"),
        "misaligned self_w": (dict(self_w_dev=_FAKE + 1), b"misaligned"),
    })
    _refused(L, "spp_agg_weighted_forward", lambda o: L.spp_agg_weighted_forward(ctypes.byref(_fwd(nat, **o)), None), cases)
    assert L.spp_agg_weighted_forward(None, None) == SPP_ERR_INVALID and b"NULL descriptor" in L.spp_last_error()
    # nothing to do: SPP_OK without a launch (and without a look at the pointers)
    for over in (dict(num_targets=0), dict(F=0, x_stride_elems=0), dict(num_targets=0, rowptr_dev=None, out_dev=None)):
        assert L.spp_agg_weighted_forward(ctypes.byref(_fwd(nat, **over)), None) == SPP_OK, over


def test_backward_refusals_come_before_any_launch():
    nat, L = _lib()
    need = L.spp_agg_weighted_backward_workspace_bytes(5, 9, 12)
    assert need > 4 * (2 * 10 + 2 * 12 + 5)                  # cnt, start, tcol, tedge, inv
    assert need > L.spp_sage_operand_backward_workspace_bytes(5, 9, 12)          # (the edge ids)
    for bad in ((-1, 9, 12), (5, 4, 12), (5, 9, -1), (5, 1 << 31, 12), (5, 9, 1 << 31)):
        assert L.spp_agg_weighted_backward_workspace_bytes(*bad) == -1, bad

    def call(over):
        over = dict(over)
        ws, nbytes = over.pop("ws", _FAKE), over.pop("nbytes", need)
        return L.spp_agg_weighted_backward(ctypes.byref(_bwd(nat, **over)), ws, nbytes, None)

    cases = {
        "fp16 gradient": (dict(grad_elem=nat.SPP_ELEM_F16), b"element code"),
        "fp8 output": (dict(out_elem=nat.SPP_ELEM_FP8_E4M3), b"element code"),
        "unknown code": (dict(out_elem=9), b"element code"),
        "negative T": (dict(num_targets=-1), b"bad sizes"),
        "S < T": (dict(num_sources=4), b"bad sizes"),
        "negative F": (dict(F=-1), b"bad sizes"),
        "negative E": (dict(num_edges=-1), b"bad sizes"),
        "S beyond int32": (dict(num_sources=1 << 31), b"2^31"),
        "E beyond int32": (dict(num_edges=1 << 31), b"2^31"),
        "S * F out of range": (dict(num_sources=(1 << 31) - 1, F=1 << 40), b"out of range"),
        "gradient stride": (dict(grad_out_stride_elems=7), b"gradient stride"),
        "NULL grad_x": (dict(grad_x_dev=None), b"NULL"),
        "NULL grad_out": (dict(grad_out_dev=None), b"NULL"),
        "NULL rowptr": (dict(rowptr_dev=None), b"NULL"),
        "NULL col": (dict(col_dev=None), b"NULL"),
        "NULL w": (dict(w_dev=None), b"NULL"),
        "misaligned grad_x": (dict(grad_x_dev=_FAKE + 2), b"misaligned"),
        "misaligned w": (dict(w_dev=_FAKE + 2), b"misaligned"),
        "no workspace": (dict(ws=None), b"workspace"),
        "small workspace": (dict(nbytes=need - 1), b"workspace"),
        "misaligned workspace": (dict(ws=_FAKE + 8, nbytes=1 << 20), b"workspace"),
    }
    _refused(L, "spp_agg_weighted_backward", call, cases)
    assert L.spp_agg_weighted_backward(None, _FAKE, need, None) == SPP_ERR_INVALID and b"NULL descriptor" in L.spp_last_error()
    for over in (dict(num_targets=0, num_sources=0, num_edges=0), dict(F=0)):
        assert L.spp_agg_weighted_backward(ctypes.byref(_bwd(nat, **over)), None, 0, None) == SPP_OK, over


def test_wgrad_refusals_come_before_any_launch():
    nat, L = _lib()
    cases = dict(_rows_cases(nat))
    cases.update({
        "fp16 gradient": (dict(grad_elem=nat.SPP_ELEM_F16), b"element code"),
        "gradient stride": (dict(grad_out_stride_elems=7), b"gradient stride"),
        "NULL grad_out": (dict(grad_out_dev=None), b"NULL"),
        "NULL grad_w": (dict(grad_w_dev=None), b"NULL"),
        "misaligned grad_w": (dict(grad_w_dev=_FAKE + 2), b"misaligned"),
        "misaligned grad_self_w": (dict(grad_self_w_dev=_FAKE + 2), b"misaligned"),
        "misaligned grad_out": (dict(grad_out_dev=_FAKE + 1, grad_elem=nat.SPP_ELEM_BF16), b"misaligned"),
    })
    _refused(L, "spp_agg_weighted_wgrad", lambda o: L.spp_agg_weighted_wgrad(ctypes.byref(_wgrad(nat, **o)), None), cases)
    assert L.spp_agg_weighted_wgrad(None, None) == SPP_ERR_INVALID and b"NULL descriptor" in L.spp_last_error()
    assert L.spp_agg_weighted_wgrad(ctypes.byref(_wgrad(nat, num_targets=0, num_edges=0)), None) == SPP_OK


def test_gcn_norm_refusals_come_before_any_launch():
    nat, L = _lib()
    cases = {
        "unknown fill": (dict(fill=3), b"fill"),
        "negative fill": (dict(fill=-1), b"fill"),
        "negative T": (dict(num_targets=-1), b"bad sizes"),
        "S < T": (dict(num_sources=4), b"bad sizes"),
        "negative E": (dict(num_edges=-1), b"bad sizes"),
        "E out of range": (dict(num_edges=1 << 60), b"out of range"),
        "NULL rowptr": (dict(rowptr_dev=None), b"NULL"),
        "NULL col": (dict(col_dev=None), b"NULL"),
        "NULL coef": (dict(coef_dev=None), b"NULL"),
        "no dinv workspace": (dict(dinv_dev=None), b"workspace"),
        "misaligned w": (dict(w_dev=_FAKE + 2), b"misaligned"),
        "misaligned dinv": (dict(dinv_dev=_FAKE + 1), b"misaligned"),
        "misaligned coef": (dict(coef_dev=_FAKE + 2), b"misaligned"),
        "misaligned self_coef": (dict(self_coef_dev=_FAKE + 3), b"misaligned"),
    }
    _refused(L, "spp_gcn_norm", lambda o: L.spp_gcn_norm(ctypes.byref(_norm(nat, **o)), None), cases)
    assert L.spp_gcn_norm(None, None) == SPP_ERR_INVALID and b"NULL descriptor" in L.spp_last_error()
    assert L.spp_gcn_norm(ctypes.byref(_norm(nat, num_targets=0, num_sources=0, num_edges=0)), None) == SPP_OK


def test_the_older_entries_accept_what_they_accepted():
    """no new epilogue code: spp_agg_forward / spp_agg_backward still stop at SPP_AGG_SUM (and the graph codes 4, 5)"""
    nat, L = _lib()
    assert L.spp_agg_forward(ctypes.byref(nat.AggFwdDesc(epilogue=6)), None) == SPP_ERR_INVALID
    assert b"epilogue" in L.spp_last_error()
    assert L.spp_agg_backward(ctypes.byref(nat.AggBwdDesc(epilogue=4)), None, 0, None) == SPP_ERR_INVALID


# ---------------------------------------------------------------------------------------------- Python
def _hop():
    """T = 5 targets over S = 8 sources: an empty row, a duplicate entry, a self reference, sources nobody names"""
    rows = [[1, 2, 5], [], [2, 2, 0, 7], [3], [0, 1, 2, 3, 4]]
    rowptr, col = [0], []
    for r in rows:
        col += r
        rowptr.append(len(col))
    return torch.tensor(rowptr), torch.tensor(col), 5, 8


def _dense(rowptr, col, w, T, S):
    A = torch.zeros((T, S), dtype=torch.float64)
    for t in range(T):
        for k in range(int(rowptr[t]), int(rowptr[t + 1])):
            A[t, int(col[k])] += float(w[k])
    return A


def test_python_argument_checks_raise_before_any_device_call(monkeypatch):
    from salient_plusplus_amd import _native as nat
    from salient_plusplus_amd import fp8
    from salient_plusplus_amd import models
    from salient_plusplus_amd.fast_sampler import TableRows

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(nat, "load", no_device)
    monkeypatch.setattr(nat, "require_device", no_device)
    rowptr, col, T, S = _hop()
    x, w, sw = torch.zeros((S, 4)), torch.ones(col.numel()), torch.ones(T)
    wa = models.weighted_aggregate
    with pytest.raises(ValueError, match="weighted_aggregate: x must be a 2-D fp32 / fp16 / bf16"):
        wa(x.double(), rowptr, col, w, T)
    with pytest.raises(ValueError, match="weighted_aggregate: x must be a 2-D"):
        wa(x[0], rowptr, col, w, T)
    with pytest.raises(TypeError, match="weighted_aggregate: x must be a tensor, a TableRows or a RowRefs"):
        wa([[0.0]], rowptr, col, w, T)
    q = fp8.Fp8Features(torch.zeros((S, 16)).to(torch.float8_e4m3fn), torch.zeros(16, dtype=torch.int8))
    for bad in (q, TableRows(q, torch.arange(S))):
        with pytest.raises(ValueError, match="weighted_aggregate: fp8 rows are not supported"):
            wa(bad, rowptr, col, w, T)
    with pytest.raises(ValueError, match="rowptr must be a 1-D int64"):
        wa(x, rowptr.int(), col, w, T)
    with pytest.raises(ValueError, match="col must be a 1-D int64"):
        wa(x, rowptr, col.float(), w, T)
    with pytest.raises(ValueError, match="num_targets must be an int in"):
        wa(x, rowptr, col, w, T + 1)
    with pytest.raises(ValueError, match="num_targets must be an int in"):
        wa(x, rowptr, col, w, -1)
    with pytest.raises(ValueError, match=f"weight must be a 1-D fp32 tensor of {col.numel()} values"):
        wa(x, rowptr, col, w[:-1], T)
    with pytest.raises(ValueError, match="weight must be a 1-D fp32 tensor"):
        wa(x, rowptr, col, w.double(), T)
    with pytest.raises(ValueError, match="weight must be a 1-D fp32 tensor"):
        wa(x, rowptr, col, None, T)
    with pytest.raises(ValueError, match=f"self_weight must be a 1-D fp32 tensor of {T} values"):
        wa(x, rowptr, col, w, T, torch.ones(T + 1))
    with pytest.raises(ValueError, match="the targets are the first rows of x"):
        wa(x[:3], rowptr, col, w, T, sw)
    with pytest.raises(ValueError, match="gcn_norm: edge_weight requires grad, and gcn_norm is not differentiable"):
        models.gcn_norm(rowptr, col, T, w.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="gcn_norm: edge_weight must be a 1-D fp32 tensor"):
        models.gcn_norm(rowptr, col, T, w[:3])
    with pytest.raises(ValueError, match="gcn_norm: rowptr must be a 1-D int64"):
        models.gcn_norm(rowptr.view(1, -1), col, T)
    with pytest.raises(TypeError):
        models.gcn_norm(rowptr, col, T, None, False)             # keyword only
    with pytest.raises(TypeError):
        models.GCN(8, 8, 3, 2, True)                             # keyword only
    with pytest.raises(TypeError):
        models.GCNConv(8, 8, True, True)                         # keyword only


def test_gcn_state_dict_is_the_reference_tree():
    from salient_plusplus_amd.models import GCN
    want = {"convs.0.lin.weight": (256, 128), "convs.1.lin.weight": (256, 256), "convs.2.lin.weight": (47, 256)}
    for i in range(3):
        want.update({f"bns.{i}.weight": (256,), f"bns.{i}.bias": (256,), f"bns.{i}.running_mean": (256,),
                     f"bns.{i}.running_var": (256,), f"bns.{i}.num_batches_tracked": ()})
    for kw in ({}, dict(normalize=True), dict(fused_norm=True)):
        state = GCN(128, 256, 47, 3, **kw).state_dict()
        assert {k: tuple(v.shape) for k, v in state.items()} == want
        assert list(state) == [f"convs.{i}.lin.weight" for i in range(3)] + \
            [f"bns.{i}.{n}" for i in range(3) for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    m = GCN(128, 256, 47, 3)
    assert all(c.bias is None and not c.normalize and not c.improved for c in m.convs)
    assert all(c.normalize for c in GCN(8, 8, 3, 2, normalize=True).convs)
    from salient_plusplus_amd.models import GCNConv
    assert sorted(GCNConv(4, 6).state_dict()) == ["bias", "lin.weight"]          # PyG's names


def test_get_model_type_resolves_gcn():
    from salient_plusplus_amd.models import GCN, _UNSUPPORTED_MODELS, get_model_type
    assert get_model_type("gcn") is GCN and get_model_type("GCN") is GCN and get_model_type("Gcn") is GCN
    assert "gcn" not in _UNSUPPORTED_MODELS
    m = get_model_type("gcn")(128, 256, 47, 3)               # built as the reference's: no bias, no normalisation
    assert all(c.bias is None and not c.normalize for c in m.convs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_weighted_reference_is_the_dense_product(dtype):
    from salient_plusplus_amd.models import _weighted_reference, weighted_aggregate
    rowptr, col, T, S = _hop()
    g = torch.Generator().manual_seed(1)
    x = torch.randn((S, 6), generator=g).to(dtype)
    w = torch.randn(col.numel(), generator=g)
    w[2] = 0.0
    sw = torch.randn(T, generator=g)
    A = _dense(rowptr, col, w, T, S)
    for self_w in (None, sw):
        want = A @ x.double()
        if self_w is not None:
            want = want + self_w.double().unsqueeze(1) * x[:T].double()
        got = _weighted_reference(x, rowptr, col, w, T, self_w)
        assert got.dtype == (torch.float64 if dtype == torch.float64 else torch.float32) and got.shape == (T, 6)
        # fp32 sums of at most 6 products of exactly read inputs
        torch.testing.assert_close(got.double(), want, rtol=0, atol=8 * 2.0 ** -24 * float((A.abs() @ x.double().abs()).max() + 10))
        if dtype != torch.float64:
            assert torch.equal(weighted_aggregate(x, rowptr, col, w, T, self_w), got)        # the CPU path
    assert bool((_weighted_reference(x, rowptr, col, w, T)[1] == 0).all())                 # the empty row
    # differentiable in all three
    xg, wg, sg = x.float().requires_grad_(True), w.clone().requires_grad_(True), sw.clone().requires_grad_(True)
    _weighted_reference(xg, rowptr, col, wg, T, sg).sum().backward()
    want_gx = A.sum(0, keepdim=True).t().expand(S, 6).clone()
    want_gx[:T] += sw.double().unsqueeze(1)
    torch.testing.assert_close(xg.grad.double(), want_gx, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(wg.grad, x.float()[col].sum(1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(sg.grad, x.float()[:T].sum(1), rtol=1e-5, atol=1e-5)


def _pyg_gcn_norm_f64(rowptr, col, w, T, S, fill):
    """PyG's gcn_norm, restated in float64 on the hop padded to [S, S]: remaining self loops are added with `fill`,
    deg = the row sum, deg^-1/2 with inf -> 0, and every value scaled from both sides"""
    A = _dense(rowptr, col, w, T, S)
    P = torch.zeros((S, S), dtype=torch.float64)
    P[:T] = A
    deg = P.sum(1) + fill
    dinv = deg.pow(-0.5)
    dinv[dinv == float("inf")] = 0
    coef = torch.tensor([float(dinv[t] * float(w[k]) * dinv[int(col[k])])
                         for t in range(T) for k in range(int(rowptr[t]), int(rowptr[t + 1]))], dtype=torch.float64)
    return coef, fill * dinv[:T] * dinv[:T], P, dinv


@pytest.mark.parametrize("kw,fill", [(dict(), 1.0), (dict(improved=True), 2.0), (dict(add_self_loops=False), 0.0)])
@pytest.mark.parametrize("weighted", [False, True])
def test_gcn_norm_reference_is_pygs_formula_on_the_padded_square(kw, fill, weighted):
    from salient_plusplus_amd.models import _gcn_norm_reference, gcn_norm
    rowptr, col, T, S = _hop()
    w = torch.rand(col.numel(), generator=torch.Generator().manual_seed(2)) + 0.1 if weighted else None
    ones = torch.ones(col.numel())
    want_coef, want_self, _P, _dinv = _pyg_gcn_norm_f64(rowptr, col, w if weighted else ones, T, S, fill)
    for fn in (_gcn_norm_reference, gcn_norm):               # (gcn_norm on CPU tensors is the restatement)
        coef, self_coef = fn(rowptr, col, T, w, **kw)
        assert coef.dtype == self_coef.dtype == torch.float32 and coef.shape == (col.numel(),) and self_coef.shape == (T,)
        torch.testing.assert_close(coef.double(), want_coef, rtol=16 * 2.0 ** -24, atol=0)
        torch.testing.assert_close(self_coef.double(), want_self, rtol=16 * 2.0 ** -24, atol=0)
    c64, s64 = _gcn_norm_reference(rowptr, col, T, w.double() if weighted else None, dtype=torch.float64, **kw)
    torch.testing.assert_close(c64, want_coef, rtol=1e-14, atol=0)
    torch.testing.assert_close(s64, want_self, rtol=1e-14, atol=0)
    if fill == 0.0:                                          # no self loops: a source that is no target has degree 0
        assert bool((coef[col >= T] == 0).all()) and bool((self_coef == 0).all())
        assert float(coef[int(rowptr[1]):int(rowptr[2])].sum()) == 0 and bool((coef[col < T][col[col < T] != 1] > 0).all())


def test_gcn_norm_on_a_whole_graph_is_the_textbook_normalisation():
    """T == S: D^-1/2 (A + I) D^-1/2 with D the degree of A + I"""
    from salient_plusplus_amd.models import _gcn_norm_reference, _weighted_reference
    g = torch.Generator().manual_seed(5)
    N = 7
    A = (torch.rand((N, N), generator=g) < 0.4).double()
    A.fill_diagonal_(0)
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = A.sum(1).long().cumsum(0)
    col = A.nonzero()[:, 1].contiguous()
    At = A + torch.eye(N, dtype=torch.float64)
    d = At.sum(1).pow(-0.5)
    want = d.unsqueeze(1) * At * d.unsqueeze(0)
    coef, self_coef = _gcn_norm_reference(rowptr, col, N, None, dtype=torch.float64)
    got = _dense(rowptr, col, coef, N, N) + torch.diag(self_coef)
    torch.testing.assert_close(got, want, rtol=1e-14, atol=0)
    x = torch.randn((N, 3), generator=g, dtype=torch.float64)
    torch.testing.assert_close(_weighted_reference(x, rowptr, col, coef, N, self_coef), want @ x, rtol=1e-13, atol=1e-14)


def _adj(rowptr, col, T, S, value=None):
    from salient_plusplus_amd.fast_trainer.monkeypatch import Adj, SparseTensor
    m = SparseTensor(rowptr=rowptr, row=None, col=col, value=value, sparse_sizes=(T, S), is_sorted=True, trust_data=True)
    return Adj(m, None, (S, T))


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("valued", [False, True])
def test_cpu_gcnconv_is_the_dense_formula(normalize, valued):
    from salient_plusplus_amd.models import GCNConv
    rowptr, col, T, S = _hop()
    g = torch.Generator().manual_seed(3)
    value = torch.rand(col.numel(), generator=g) + 0.5 if valued else None
    w = value if valued else torch.ones(col.numel())
    x = torch.randn((S, 6), generator=g)
    torch.manual_seed(0)
    conv = GCNConv(6, 4, normalize=normalize)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(4, generator=g))
    adj = _adj(rowptr, col, T, S, value)
    if normalize:
        coef, self_coef, _P, _d = _pyg_gcn_norm_f64(rowptr, col, w, T, S, 1.0)
        M = _dense(rowptr, col, coef, T, S)
        M[:, :T] += torch.diag(self_coef)
    else:
        M = _dense(rowptr, col, w, T, S)
    want = (M @ x.double()) @ conv.lin.weight.double().t() + conv.bias.double()
    for got in (conv(x, adj.adj_t, adj.size), conv((x, x[:T]), adj.adj_t), conv((x, x[:T].clone()), adj.adj_t),
                conv(x, adj.adj_t)):
        assert got.shape == (T, 4) and got.dtype == torch.float32
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-5)
    got.sum().backward()
    assert conv.lin.weight.grad is not None and conv.bias.grad is not None


@pytest.mark.parametrize("normalize", [False, True])
def test_cpu_gcn_forward_is_the_dense_formula(normalize):
    from salient_plusplus_amd.models import GCN
    g = torch.Generator().manual_seed(4)
    sizes = [(9, 14), (6, 9), (3, 6)]                        # (targets, sources), outermost first
    adjs, mats = [], []
    for T, S in sizes:
        deg = torch.randint(0, 4, (T,), generator=g)
        rowptr = torch.zeros(T + 1, dtype=torch.int64)
        rowptr[1:] = deg.cumsum(0)
        col = torch.randint(0, S, (int(rowptr[-1]),), generator=g)
        adjs.append(_adj(rowptr, col, T, S))
        ones = torch.ones(col.numel())
        if normalize:
            coef, self_coef, _P, _d = _pyg_gcn_norm_f64(rowptr, col, ones, T, S, 1.0)
            M = _dense(rowptr, col, coef, T, S)
            M[:, :T] += torch.diag(self_coef)
        else:
            M = _dense(rowptr, col, ones, T, S)
        mats.append(M)
    torch.manual_seed(0)
    model = GCN(5, 8, 3, 3, normalize=normalize).eval()
    with torch.no_grad():
        for bn in model.bns:
            bn.running_mean.copy_(torch.randn(8, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(8, generator=g) + 0.5)
    x = torch.randn((14, 5), generator=g).half()
    h = x.double()
    for i, M in enumerate(mats):
        h = (M @ h) @ model.convs[i].lin.weight.double().t()
        if i != 2:
            bn = model.bns[i]
            h = (h - bn.running_mean.double()) / (bn.running_var.double() + bn.eps).sqrt() * bn.weight.double() + bn.bias.double()
            h = h.relu()
    want = torch.log_softmax(h, dim=-1)
    for fused in (False, True):
        model.fused_norm = fused                             # (CPU tensors take batch_norm_act's torch composition)
        got = model(x, adjs)
        assert got.shape == (3, 3) and got.dtype == torch.float32
        torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-5)
    from inference_method import assert_method_is_the_function
    rowptr = torch.arange(15, dtype=torch.int64)             # 14 nodes of one entry each
    assert_method_is_the_function(model, x, rowptr, torch.arange(14), edge_weight=torch.ones(14))
    assert not model.training
