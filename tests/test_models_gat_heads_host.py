"""CPU-only: multi-head GAT (PyG's ``heads`` / ``concat``).  The module trees and state dicts of GATConv and GAT with
heads > 1, the unchanged heads=1 layout, the width rule of GAT(heads=H), the C ABI of the spp_gat_mh_* entries, and
the plain-torch path of GATConv(heads=H) against a per-edge restatement of PyG's GATConv."""
import io
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MH_ENTRIES = ["spp_gat_mh_logits", "spp_gat_mh_logits_backward", "spp_gat_mh_aggregate_forward",
              "spp_gat_mh_aggregate_backward", "spp_gat_mh_aggregate_backward_gather_workspace_bytes",
              "spp_gat_mh_aggregate_backward_gather"]


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_gatconv_heads_state_dict_follows_pyg(concat, bias):
    from salient_plusplus_amd.models import GATConv
    conv = GATConv(128, 64, heads=4, concat=concat, bias=bias)
    want = {"lin_src.weight": (256, 128), "lin_dst.weight": (256, 128), "att_src": (1, 4, 64), "att_dst": (1, 4, 64)}
    if bias:
        want["bias"] = (256,) if concat else (64,)
    assert _shapes(conv) == want
    assert conv.lin_dst is conv.lin_src
    assert conv.heads == 4 and conv.concat == concat


def test_gatconv_heads1_state_dict_is_unchanged():
    from salient_plusplus_amd.models import GATConv
    want = {"lin_src.weight": (64, 128), "lin_dst.weight": (64, 128), "att_src": (1, 1, 64), "att_dst": (1, 1, 64)}
    assert _shapes(GATConv(128, 64, bias=False)) == want
    assert _shapes(GATConv(128, 64)) == dict(want, bias=(64,))


def test_gat_heads4_module_tree_and_widths():
    from salient_plusplus_amd.models import GAT, GATConv
    m = GAT(128, 256, 47, 3, heads=4)
    assert len(m.convs) == 3 and all(isinstance(c, GATConv) for c in m.convs)
    assert [(c.heads, c.out_channels, c.concat, c.bias is None) for c in m.convs] == [
        (4, 64, True, True), (4, 64, True, True), (4, 47, False, True)]
    want = {}
    for i, (w, c) in enumerate([((256, 128), 64), ((256, 256), 64), ((188, 256), 47)]):   # 188 = 4 heads x 47
        want.update({f"convs.{i}.lin_src.weight": w, f"convs.{i}.lin_dst.weight": w, f"convs.{i}.att_src": (1, 4, c),
                     f"convs.{i}.att_dst": (1, 4, c)})
    assert _shapes(m) == want


def test_gat_without_heads_keeps_todays_keys_and_shapes():
    from salient_plusplus_amd.models import GAT
    want = {}
    for i, (d_in, d_out) in enumerate([(128, 256), (256, 256), (256, 47)]):
        want[f"convs.{i}.lin_src.weight"] = (d_out, d_in)
        want[f"convs.{i}.lin_dst.weight"] = (d_out, d_in)
        want[f"convs.{i}.att_src"] = (1, 1, d_out)
        want[f"convs.{i}.att_dst"] = (1, 1, d_out)
    assert _shapes(GAT(128, 256, 47, 3)) == want
    assert _shapes(GAT(128, 256, 47, 3, heads=1)) == want


def test_gat_heads_checkpoint_round_trip():
    from salient_plusplus_amd.models import GAT
    torch.manual_seed(0)
    a = GAT(32, 64, 5, 3, heads=4)
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    torch.manual_seed(1)
    b = GAT(32, 64, 5, 3, heads=4)
    assert not torch.equal(a.convs[0].lin_src.weight, b.convs[0].lin_src.weight)
    b.load_state_dict(torch.load(buf))
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    with pytest.raises(RuntimeError):                          # a heads=1 checkpoint does not fit heads=4
        b.load_state_dict(GAT(32, 64, 5, 3).state_dict())


def test_gat_hidden_not_a_multiple_of_heads_raises():
    from salient_plusplus_amd.models import GAT
    with pytest.raises(ValueError):
        GAT(128, 250, 47, 3, heads=4)
    with pytest.raises(ValueError):
        GAT(128, 256, 47, 3, heads=0)


def test_gat_heads_is_keyword_only():
    from salient_plusplus_amd.models import GAT
    with pytest.raises(TypeError):
        GAT(128, 256, 47, 3, 4)


def test_gat_mh_symbols_are_declared_and_bound():
    from salient_plusplus_amd import _native as nat
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spp.h")).read(), flags=re.S)
    for name in MH_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in nat.SIGNATURES
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(decl.split(",")) == len(nat.SIGNATURES[name][1]), name
        assert "int32_t heads" in decl, name
    if os.path.exists(nat.LIB_PATH):
        L = nat.load()
        for name in MH_ENTRIES:
            assert hasattr(L, name), f"{name} not exported"
        # a head count the kernels are not built for is refused by the workspace query without a device
        assert L.spp_gat_mh_aggregate_backward_gather_workspace_bytes(10, 20, 30, 3) == -1      # SPP_ERR_INVALID
        assert L.spp_gat_mh_aggregate_backward_gather_workspace_bytes(10, 20, 30, 4) > 0


@pytest.mark.parametrize("T,S,E", [(0, 0, 0), (0, 5, 0), (1, 1, 1), (37, 90, 231), (1500, 5000, 9001),
                                   (164_000, 947_000, 1_640_003)])
def test_single_head_gather_workspace_is_the_heads1_spelling(T, S, E):
    """alpha_e [E, H] | alpha_self [T, H] | the transposed hop with edge ids, each part rounded up to 16 bytes; the
    transposed hop with edge ids is spp_sage_operand_backward_workspace_bytes' (without them) plus tedge [E]"""
    from salient_plusplus_amd import _native as nat
    L = nat.load()

    def a16(v):
        return (v + 15) & ~15

    def want(H):
        return a16(4 * H * E) + a16(4 * H * T) + int(L.spp_sage_operand_backward_workspace_bytes(T, S, E)) + a16(4 * E)

    one = int(L.spp_gat_aggregate_backward_gather_workspace_bytes(T, S, E))
    assert one == int(L.spp_gat_mh_aggregate_backward_gather_workspace_bytes(T, S, E, 1)) == want(1)
    assert int(L.spp_gat_mh_aggregate_backward_gather_workspace_bytes(T, S, E, 4)) == want(4)


def _per_edge_gat(x, x_t, W, att_src, att_dst, rowptr, col, slope, concat):
    """PyG's GATConv written edge by edge in float64 (set_diag: diagonal entries dropped, one self loop per target)"""
    H, C = att_src.shape
    h = (x.double() @ W.double().t()).view(-1, H, C)
    h_t = (x_t.double() @ W.double().t()).view(-1, H, C)
    out = torch.zeros(x_t.size(0), H, C, dtype=torch.float64)
    for i in range(x_t.size(0)):
        srcs = [int(j) for j in col[rowptr[i]:rowptr[i + 1]] if int(j) != i] + [i]
        for hd in range(H):
            e = torch.stack([torch.nn.functional.leaky_relu(h[j, hd] @ att_src[hd].double() +
                                                            h_t[i, hd] @ att_dst[hd].double(), slope) for j in srcs])
            a = torch.softmax(e, 0)
            out[i, hd] = sum(a[k] * h[j, hd] for k, j in enumerate(srcs))
    return out.reshape(x_t.size(0), H * C) if concat else out.mean(1)


@pytest.mark.parametrize("heads,concat", [(4, True), (4, False), (3, True)])
def test_gatconv_heads_plain_torch_path_matches_pyg(heads, concat):
    """On CPU tensors GATConv(heads > 1) takes the plain-torch composition: forward against the per-edge restatement"""
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    from salient_plusplus_amd.models import GATConv
    torch.manual_seed(heads)
    T, S, K, C = 12, 30, 10, 5
    deg = torch.randint(0, 5, (T,))
    deg[3] = 0                                                 # an empty row
    deg[1] = 2
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, S, (int(rowptr[-1]),))
    col[rowptr[1]] = 1                                         # a diagonal entry (dropped by set_diag)
    conv = GATConv(K, C, heads=heads, concat=concat, bias=True)
    torch.nn.init.normal_(conv.bias)
    x = torch.randn(S, K)
    adj = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(T, S))
    out = conv((x, x[:T]), adj)
    want = _per_edge_gat(x, x[:T], conv.lin_src.weight.detach(), conv.att_src.detach().view(heads, C),
                         conv.att_dst.detach().view(heads, C), rowptr, col, 0.2, concat) + conv.bias.detach().double()
    assert out.shape == ((T, heads * C) if concat else (T, C))
    torch.testing.assert_close(out.double(), want, rtol=1e-5, atol=1e-6)
    # a target block that is not x's prefix: the logits of the targets come from x_target
    xt = torch.randn(T, K)
    out2 = conv((x, xt), adj)
    want2 = _per_edge_gat(x, xt, conv.lin_src.weight.detach(), conv.att_src.detach().view(heads, C),
                          conv.att_dst.detach().view(heads, C), rowptr, col, 0.2, concat) + conv.bias.detach().double()
    torch.testing.assert_close(out2.double(), want2, rtol=1e-5, atol=1e-6)
