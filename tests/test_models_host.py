"""CPU-only: the model menu of driver/main.py:74-95 and the module trees of GIN and SAGEResInception
(driver/models.py:95-283), whose state dicts must load the reference's checkpoints and back."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _gin_keys(in_c, hid, out_c, L):
    keys = {}
    for i in range(L):
        d_in = in_c if i == 0 else hid
        keys[f"convs.{i}.eps"] = (1,)
        keys[f"convs.{i}.nn.0.weight"] = (hid, d_in)
        keys[f"convs.{i}.nn.0.bias"] = (hid,)
        for b in ("weight", "bias", "running_mean", "running_var"):
            keys[f"convs.{i}.nn.1.{b}"] = (hid,)
        keys[f"convs.{i}.nn.1.num_batches_tracked"] = ()
        keys[f"convs.{i}.nn.3.weight"] = (hid, hid)
        keys[f"convs.{i}.nn.3.bias"] = (hid,)
    keys.update({"lin1.weight": (hid, hid), "lin1.bias": (hid,), "lin2.weight": (out_c, hid), "lin2.bias": (out_c,)})
    return keys


def _sage_ri_keys(in_c, hid, out_c, L):
    keys = {}
    for i in range(L):
        d_in = in_c if i == 0 else hid
        keys[f"convs.{i}.lin_l.weight"] = (hid, d_in)
        keys[f"convs.{i}.lin_r.weight"] = (hid, d_in)
        for b in ("weight", "bias", "running_mean", "running_var"):
            keys[f"bns.{i}.{b}"] = (hid,)
        keys[f"bns.{i}.num_batches_tracked"] = ()
    keys.update({"res_linears.0.weight": (hid, in_c), "res_linears.0.bias": (hid,),
                 "mlp.module_list.0.weight": (2 * out_c, in_c + hid * L), "mlp.module_list.0.bias": (2 * out_c,),
                 "mlp.module_list.1.weight": (out_c, 2 * out_c), "mlp.module_list.1.bias": (out_c,)})
    return keys


def test_get_model_type_maps_the_four_working_models():
    from salient_plusplus_amd import models as M
    for name, cls in (("sage", M.SAGE), ("GAT", M.GAT), ("Gin", M.GIN), ("SAGEResInception", M.SAGEResInception),
                      ("sageresinception", M.SAGEResInception), ("gcn", M.GCN), ("GCN", M.GCN)):
        assert M.get_model_type(name) is cls
    for name in ("sageclassic", "JKNet", "ARMA"):
        with pytest.raises(NotImplementedError, match="not implemented"):
            M.get_model_type(name)
    with pytest.raises(ValueError):
        M.get_model_type("mlp")


def test_gin_state_dict_matches_the_reference_tree():
    from salient_plusplus_amd.models import GIN
    m = GIN(128, 256, 47, 3)
    sd = m.state_dict()
    want = _gin_keys(128, 256, 47, 3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    names = {n for n, _ in m.named_parameters()}
    for i in range(3):
        assert f"convs.{i}.eps" not in names                        # a buffer, as PyG's GINConv(train_eps=False)
        assert torch.equal(sd[f"convs.{i}.eps"], torch.zeros(1))
    # a checkpoint round trip through a second instance (what driver/main.py saves and loads)
    m2 = GIN(128, 256, 47, 3)
    m2.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), sd.values()))


def test_sage_res_inception_state_dict_and_mlp():
    from salient_plusplus_amd.models import SAGEResInception
    m = SAGEResInception(128, 256, 47, 3)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == _sage_ri_keys(128, 256, 47, 3)
    mods = list(m.mlp.module_list)
    assert len(mods) == 2 and all(isinstance(x, torch.nn.Linear) for x in mods)    # the reference's `continue`
    assert isinstance(m.res_linears[0], torch.nn.Linear)
    assert all(isinstance(x, torch.nn.Identity) for x in list(m.res_linears)[1:])
    assert m.convs[-1].lin_l.weight.shape == (256, 256)                              # the last conv outputs hidden


def test_mlp_without_end_up_with_fc_has_bn_and_activation():
    from salient_plusplus_amd.models import MLP
    m = MLP(10, 20, 5, 3, act="LeakyReLU", bn=True)
    kinds = [type(x).__name__ for x in m.module_list]
    assert kinds == ["Linear", "BatchNorm1d", "LeakyReLU"] * 3
    assert m.module_list[0].in_features == 10 and m.module_list[-3].out_features == 5


def test_dropout_overrides_are_keyword_only_with_reference_defaults():
    from salient_plusplus_amd.models import GIN, SAGEResInception
    assert GIN(8, 16, 3, 2).dropout == 0.5 and SAGEResInception(8, 16, 3, 2).dropout == 0.1
    assert GIN(8, 16, 3, 2, dropout=0.0).dropout == 0.0
    with pytest.raises(TypeError):
        GIN(8, 16, 3, 2, 0.0)


def test_sum_aggregation_symbols_are_declared_and_bound():
    from salient_plusplus_amd import _native as nat
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spp.h")).read(), flags=re.S)
    new = ["spp_csr_sum_forward", "spp_csr_sum_forward_table", "spp_csr_sum_forward_rows", "spp_csr_sum_backward",
           "spp_csr_sum_backward_gather"]
    for name in new:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in nat.SIGNATURES
    if os.path.exists(nat.LIB_PATH):
        L = nat.load()
        for name in new:
            assert hasattr(L, name), f"{name} not exported"
