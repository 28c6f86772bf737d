"""CPU-only: the one-pass mean / min / max / std aggregation (spp.h f4b) without a device -- spp_agg_stats_desc against
the header, the refusals the two entries make before a launch and their order, _stats_reference in float64 against a
row-by-row numpy formula and its autograd against the closed-form gradient, and the PNAConv / PNA surface."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_FAKE = 0x7F0000001000                                   # never dereferenced: every refusal comes before a launch


def test_descriptor_round_trips_through_ctypes(tmp_path):
    """field names in the header's order, sizeof and every offset cross-checked by compiling the header with gcc"""
    from salient_plusplus_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    body = header[header.index("typedef struct spp_agg_stats_desc {"):header.index("} spp_agg_stats_desc;")]
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body))
    assert names == [f[0] for f in nat.AggStatsDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spp.h"\nint main(void) { size_t v[] = { '
                   "sizeof(spp_agg_stats_desc), %s };\n for (size_t i = 0; i < sizeof v / sizeof *v; ++i) "
                   'printf("%%zu\\n", v[i]);\n return 0; }\n' % ", ".join(f"offsetof(spp_agg_stats_desc, {n})" for n in names))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "layout")]).split()]
    assert got == [ctypes.sizeof(nat.AggStatsDesc)] + [getattr(nat.AggStatsDesc, n).offset for n in names]
    assert "aggregate_stats.hip" in __import__("salient_plusplus_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("entry", ["spp_agg_stats_forward", "spp_agg_stats_backward"])
def test_refusals_come_before_any_launch_in_the_stated_order(entry):
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    ok = dict(x_elem=nat.SPP_ELEM_F32, out_elem=nat.SPP_ELEM_F32, grad_elem=nat.SPP_ELEM_F32, scalers=7, delta=1.5,
              eps=1e-5, rowptr_dev=_FAKE, col_dev=_FAKE, num_targets=5, num_sources=9, num_edges=20, x_dev=_FAKE,
              x_stride_elems=8, F=8, add_dev=_FAKE, out_dev=_FAKE, stats_dev=_FAKE, pos_dev=_FAKE, grad_out_dev=_FAKE,
              grad_x_dev=_FAKE, grad_add_dev=_FAKE)
    stride = "out_stride_elems" if entry.endswith("forward") else "grad_out_stride_elems"
    # each case keeps every LATER fault of the list as well: the message names the earliest one
    order = [(dict(x_elem=7), b"element code"), (dict(scalers=8), b"scalers"), (dict(delta=0.0), b"delta"),
             (dict(num_targets=-1), b"negative"), (dict(num_edges=1 << 31), b"2^31"), (dict(F=6), b"F % 4"),
             (dict(num_sources=1 << 60), b"out of range"), ({stride: 7}, b"stride smaller"), (dict(rowptr_dev=None), b"NULL"),
             (dict(x_stride_elems=4), b"row stride"), (dict(x_dev=_FAKE + 4), b"misaligned")]
    for i, (_, text) in enumerate(order):
        over = {k: v for o, _t in order[i:] for k, v in o.items()}
        assert getattr(L, entry)(ctypes.byref(nat.AggStatsDesc(**dict(ok, **over))), None) == -1, text
        msg = L.spp_last_error()
        assert entry.encode() in msg and text in msg, (text, msg)
    assert getattr(L, entry)(None, None) == -1 and b"NULL descriptor" in L.spp_last_error()
    for over in (dict(eps=-1.0), dict(delta=float("nan")), dict(scalers=0), dict(stats_dev=None)):
        assert getattr(L, entry)(ctypes.byref(nat.AggStatsDesc(**dict(ok, **over))), None) == -1, over
    # nothing to do: SPP_OK without a launch and without a look at the pointers
    assert getattr(L, entry)(ctypes.byref(nat.AggStatsDesc(**dict(ok, num_targets=0, rowptr_dev=None, x_dev=None))), None) == 0


def test_reference_against_numpy_and_the_closed_form_gradient():
    """rows: empty, one entry, a source listed twice that holds the minimum (column 0) and a tie for the maximum
    (column 1), and a longer one; out, positions and autograd against the formulas, literally, row by row"""
    from salient_plusplus_amd.models import _stats_reference
    rng = np.random.default_rng(0)
    x = rng.standard_normal((7, 3))
    x[2, 0], x[2, 1], x[4, 1] = -5.0, 9.0, 9.0
    rows = [[], [6], [4, 2, 5, 2], [0, 1, 3, 5, 6, 1]]
    add, g = rng.standard_normal((4, 3)), rng.standard_normal((4, 36))
    delta, eps, scalers = 1.7, 1e-5, ("identity", "amplification", "attenuation")
    want, gx, ga, kmins = np.zeros((4, 36)), np.zeros((7, 3)), np.zeros((4, 3)), np.full((4, 3), -1)
    k0 = 0
    for t, row in enumerate(rows):
        d = len(row)
        if d:
            v = x[row]
            mean, std, kmn, kmx = v.mean(0), np.sqrt(v.var(0) + eps), v.argmin(0), v.argmax(0)      # arg*: first occurrence
            blocks = np.concatenate([mean + add[t], v.min(0) + add[t], v.max(0) + add[t], std])
            sc = [1.0, np.log(d + 1) / delta, delta / np.log(d + 1)]
            want[t] = np.concatenate([s * blocks for s in sc])
            G = sum(s * g[t, 12 * i:12 * i + 12] for i, s in enumerate(sc)).reshape(4, 3)       # mean, min, max, std
            ga[t] = G[0] + G[1] + G[2]
            for k, j in enumerate(row):
                gx[j] += G[0] / d + G[3] * (v[k] - mean) / (d * std) + (k == kmn) * G[1] + (k == kmx) * G[2]
            kmins[t] = k0 + kmn
        k0 += d
    rowptr = torch.tensor(np.cumsum([0] + [len(r) for r in rows]))
    col = torch.tensor([j for r in rows for j in r])
    xt, at = torch.tensor(x, requires_grad=True), torch.tensor(add, requires_grad=True)
    out, kmin, _ = _stats_reference(xt, rowptr, col, 4, add=at, scalers=scalers, delta=delta, eps=eps, with_pos=True)
    out.backward(torch.tensor(g))
    assert out.dtype == torch.float64 and kmin.tolist() == kmins.tolist() and kmins[2, 0] == 2       # the FIRST of the two
    for got, ref in ((out, want), (xt.grad, gx), (at.grad, ga)):
        np.testing.assert_allclose(got.detach().numpy(), ref, rtol=1e-12, atol=1e-13)
    assert _stats_reference(xt.detach().float(), rowptr, col, 4).dtype == torch.float32


def test_pna_surface():
    from salient_plusplus_amd import models
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    assert models.get_model_type("pna") is models.PNA and models.get_model_type("PNA") is models.PNA
    conv = models.PNAConv(8, 16, delta=1.2)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {
        "pre_nns.0.0.weight": (8, 16), "pre_nns.0.0.bias": (8,), "post_nns.0.0.weight": (16, 104),
        "post_nns.0.0.bias": (16,), "lin.weight": (16, 16), "lin.bias": (16,)}
    for bad in (dict(aggregators=("mean", "max")), dict(scalers=("attenuation", "identity")), dict(scalers=()), dict(delta=0)):
        with pytest.raises(ValueError):
            models.PNAConv(8, 16, **dict(dict(delta=1.2), **bad))
    with pytest.raises(ValueError, match="scalers"):
        models.stats_aggregate(torch.zeros((3, 4)), torch.tensor([0, 1]), torch.tensor([2]), 1, scalers=("linear",))
    rowptr, col = torch.tensor([0, 2, 2, 5]), torch.tensor([4, 1, 0, 3, 3])
    assert abs(models.pna_delta(rowptr) - float(np.log([3, 1, 4]).mean())) < 1e-12
    adj = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(3, 5))
    out = conv(torch.randn((5, 8)), adj, (5, 3))
    assert out.shape == (3, 16) and bool(torch.isfinite(out).all())
    model = models.PNA(8, 16, 4, 2, delta=1.2)
    assert not hasattr(model, "inference") and len(model.convs) == 2 and len(model.bns) == 1
