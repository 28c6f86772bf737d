"""CPU-only: the f4f entries (spp.h) refuse what needs no device to refuse (ctypes descriptors on fake pointers);
layer_norm_act on CPU tensors is the torch composition's bits; norm="layer" adds the norms.* keys; inference refuses it."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

_FAKE = 0x10000                                               # 16-byte aligned, never dereferenced
ENTRIES = ["spp_ln_act_forward", "spp_ln_act_backward"]
REFUSALS = [("C = 6", dict(C=6), b"C = 6", ENTRIES), ("C = 1028", dict(C=1028), b"C = 1028", ENTRIES),
            ("p = 1", dict(p=1.0), b"[0, 1)", ENTRIES), ("NaN p", dict(p=float("nan")), b"[0, 1)", ENTRIES),
            ("short workspace", dict(workspace_bytes=16), b"workspace", ENTRIES[1:])]     # (forward takes none)


def _desc(nat, L, **over):
    kw = dict(act=nat.SPP_LN_ACT_RELU, training=1, negative_slope=0.01, p=0.1, eps=1e-5, seed=7, n=100, C=8,
              workspace_bytes=1 << 20, **{k: _FAKE for k in ("z_dev", "gamma_dev", "beta_dev", "y_dev", "mean_dev", "rstd_dev",
                                                          "g_dev", "dz_dev", "dgamma_dev", "dbeta_dev", "workspace_dev")})
    return nat.LnActDesc(**{**kw, **over})


@pytest.mark.parametrize("what,over,word,entries", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_entry_and_an_empty_call_succeeds(what, over, word, entries):
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    assert L.spp_ln_act_workspace_bytes(2 * L.spp_ln_act_slab_rows() + 3, 260) == 3 * 2 * 260 * 4   # [2, C] fp32 a slab
    for entry in entries:
        assert getattr(L, entry)(ctypes.byref(_desc(nat, L, **over)), None) == -1, (entry, what)
        msg = L.spp_last_error()
        assert msg.startswith(entry.encode() + b":") and word in msg, (entry, what, msg)
    for entry in ENTRIES:                                      # n == 0: success before any pointer is looked at
        assert getattr(L, entry)(ctypes.byref(nat.LnActDesc(n=0, C=8)), None) == 0, L.spp_last_error()


@pytest.mark.parametrize("act,training,with_r", itertools.product(["none", "relu", "leaky_relu"], [True, False], [False, True]))
def test_cpu_tensors_take_the_torch_composition_bit_for_bit(act, training, with_r):
    from salient_plusplus_amd.models import layer_norm_act
    g = torch.Generator().manual_seed(11)
    z0, r0, w = (torch.randn((37, 12), generator=g) for _ in range(3))
    res = []
    for ours in (True, False):
        torch.manual_seed(0)
        ln = torch.nn.LayerNorm(12)
        ln.weight.data.uniform_(0.5, 1.5), ln.bias.data.uniform_(-1, 1)
        z, r = z0.clone().requires_grad_(True), (r0.clone().requires_grad_(True) if with_r else None)
        if ours:
            y = layer_norm_act(z, ln, act=act, negative_slope=0.02, p=0.0, training=training, residual=r)
        else:
            h = F.relu(ln(z)) if act == "relu" else F.leaky_relu(ln(z), 0.02) if act == "leaky_relu" else ln(z)
            y = F.dropout(h, 0.0, training) + r if with_r else F.dropout(h, 0.0, training)
        (y * w).sum().backward()
        res.append((y.detach(), z.grad, ln.weight.grad, ln.bias.grad, r.grad if with_r else None))
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(*res))


def test_norm_keyword_state_dict_bad_arguments_and_the_inference_refusal():
    from salient_plusplus_amd.inference import layerwise_inference
    from salient_plusplus_amd.models import GAT, GATv2, GraphTransformer, layer_norm_act
    m = GATv2(100, 32, 7, 3, heads=4, norm="layer")
    plain = GATv2(100, 32, 7, 3, heads=4)
    assert [k for k in m.state_dict() if k not in plain.state_dict()] == [f"norms.{i}.{n}" for i in (0, 1) for n in ("weight", "bias")]
    assert list(GATv2(100, 32, 7, 3, heads=4, norm=None).state_dict()) == list(plain.state_dict())
    assert not hasattr(plain, "norms") and [type(n) for n in m.norms] == [torch.nn.LayerNorm] * 2
    for cls in (GAT, GATv2, GraphTransformer):
        with pytest.raises(ValueError, match="norm must be None or 'layer'"):
            cls(100, 32, 7, 3, norm="batch")
    with pytest.raises(ValueError, match="act must be one of"):
        layer_norm_act(torch.randn(3, 4), torch.nn.LayerNorm(4), act="gelu")
    for call in (m.inference, lambda *a: layerwise_inference(m, *a), lambda *a: layerwise_inference(GraphTransformer(100, 32, 7, 3, norm="layer"), *a)):
        with pytest.raises(ValueError, match="norm='layer'.*no LayerNorm yet"):
            call(None, None, None)                             # refused before any tensor is looked at
