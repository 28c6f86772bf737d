"""CPU: ResGatedGraphConv (spp.h f4g): PyG's module tree, the refusals in the header's order, the reference against float64"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resgated_f64 as G  # noqa: E402
from salient_plusplus_amd import _native as nat  # noqa: E402
from salient_plusplus_amd import models  # noqa: E402
from salient_plusplus_amd.models import ResGated, ResGatedGraphConv, get_model_type  # noqa: E402


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("root_weight", [False, True])
def test_state_dict_is_pygs(root_weight, bias):
    want = {f"lin_{n}.{p}": s for n in ("key", "query", "value") for p, s in (("weight", (6, 10)), ("bias", (6,)))}
    want.update({"lin_skip.weight": (6, 10)} if root_weight else {}, **({"bias": (6,)} if bias else {}))
    assert {k: tuple(v.shape) for k, v in ResGatedGraphConv(10, 6, root_weight=root_weight, bias=bias).state_dict().items()} == want


def test_constructor_refusals_and_model_names():
    with pytest.raises(NotImplementedError, match="edge_dim"):
        ResGatedGraphConv(8, 8, edge_dim=4)
    with pytest.raises(NotImplementedError, match="act"):
        ResGatedGraphConv(8, 8, act=torch.nn.Tanh())
    assert get_model_type("resgated") is ResGated and get_model_type("ResGated") is ResGated
    assert not hasattr(ResGated(10, 8, 3, 3, fused_norm=True), "inference")
    for name in ("sageclassic", "jknet", "arma", "mlp", "gatv3", "transformerconv"):
        with pytest.raises(NotImplementedError if name in ("sageclassic", "jknet", "arma") else ValueError):
            get_model_type(name)


_MEM = (C.c_char * 128)()
_PTRS = {f[0] for f in nat.ResGatedDesc._fields_ if f[0].endswith("_dev")}    # host addresses: no check dereferences one
# spp.h f4g's refusals in its order: (fields of an otherwise valid descriptor, a word of the message); the earlier fault wins
REFUSALS = [
    (dict(x_elem=3), "element code"), (dict(x_elem=-1, D=6), "element code"), (dict(D=0), "multiple of 4"),
    (dict(D=6, num_targets=-1), "multiple of 4"), (dict(D=1028), "multiple of 4"), (dict(num_targets=6), "bad sizes"),
    (dict(num_targets=-1, k_stride_elems=1), "bad sizes"), (dict(num_edges=-1), "bad sizes"), (dict(num_sources=1 << 31), "2^31"),
    (dict(k_stride_elems=12, k_dev=None), "stride"), (dict(q_stride_elems=18), "stride"), (dict(v_stride_elems=8), "stride"),
    (dict(rowptr_dev=None, k_dev=4), "NULL"), (dict(col_dev=None), "NULL"), (dict(k_dev=None), "NULL"), (dict(q_dev=None), "NULL"),
    (dict(v_dev=None, q_dev=8), "NULL"), (dict(k_dev=8), "misaligned"), (dict(q_dev=4), "misaligned"), (dict(v_dev=8), "misaligned"),
    (dict(col_dev=4), "misaligned")]
OWN = {"spp_resgated_forward": [(dict(out_dev=None, k_dev=8), "NULL"), (dict(out_dev=8), "misaligned")],
       "spp_resgated_backward": [(dict(grad_out_dev=None), "NULL"), (dict(grad_k_dev=None, q_dev=8), "NULL"),
                                 (dict(grad_q_dev=None), "together"), (dict(workspace_dev=None, grad_k_dev=8), "workspace"),
                                 (dict(grad_v_dev=8), "misaligned"), (dict(workspace_dev=8), "workspace"), (dict(workspace_bytes=16), "workspace")]}


def _desc(**kw):
    ok = C.addressof(_MEM) + (-C.addressof(_MEM)) % 16
    d = dict(x_elem=0, num_targets=3, num_sources=5, num_edges=4, D=16, k_stride_elems=16, q_stride_elems=32,
             v_stride_elems=32, workspace_bytes=1 << 20, **{n: ok for n in _PTRS})
    d.update({n: (ok + v if v is not None else None) if n in _PTRS else v for n, v in kw.items()})
    return nat.ResGatedDesc(**d)


@pytest.mark.parametrize("entry", list(OWN))
def test_refusals_in_the_documented_order(entry):
    L = nat.load()
    assert getattr(L, entry)(None, None) == -1 and "NULL descriptor" in L.spp_last_error().decode()
    for fields, word in REFUSALS + OWN[entry]:
        assert getattr(L, entry)(C.byref(_desc(**fields)), None) == -1, (entry, fields)
        assert entry in (msg := L.spp_last_error().decode()) and word in msg, (fields, msg)
    # no targets: OK before a pointer is looked at; the shape is still checked.  Without grad_q / grad_v: no workspace
    assert getattr(L, entry)(C.byref(_desc(num_targets=0, k_dev=None, out_dev=None, grad_k_dev=None, q_stride_elems=1)), None) == 0
    assert getattr(L, entry)(C.byref(_desc(num_targets=0, D=6)), None) == -1 and L.spp_resgated_workspace_bytes(6, 5, 4) == -1


@pytest.mark.parametrize("regime", G.REGIMES)
def test_reference_is_the_float64_restatement_on_the_planted_hop(regime):
    rowptr, col, S = G.hop("planted")
    k, q, v, g = (t.double() for t in G.inputs(regime, 5, S, 12, torch.float32))
    want = G.restate(k, q, v, g, rowptr, col)
    k, q, v = (t.clone().requires_grad_() for t in (k, q, v))
    (out := models._resgated_reference(k, q, v, rowptr, col)).backward(g)
    assert out.dtype == torch.float64 and not out[1].any() and not q.grad[8].any() and not v.grad[8].any()
    for got, ref in zip((out, k.grad, q.grad, v.grad), want):
        torch.testing.assert_close(got.detach(), ref, rtol=0, atol=1e-13 * max(1.0, float(ref.abs().max())))
