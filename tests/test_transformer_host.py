"""CPU: TransformerConv (csrc/transformer_conv.hip, spp.h f3y, models.TransformerConv / GraphTransformer) without a
device.  The two entries are exported, bound and declared, the ctypes descriptor is the header's struct, and the entries
refuse what the header says in the order it says; the module tree is PyG's; _transformer_reference is the float64
restatement of tests/transformer_f64.py, an independent dense formulation, and differentiable (gradcheck); the p > 0
training path draws torch's mask on the reference path."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transformer_f64 as G  # noqa: E402

ENTRIES = ["spp_transformer_forward", "spp_transformer_backward"]
F32, F64 = torch.float32, torch.float64


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spp.h")).read(), flags=re.S)


def test_symbols_are_exported_bound_and_declared():
    from salient_plusplus_amd import _native as nat
    src = _header()
    L = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bspp_status\s+" + name + r"\s*\(\s*const\s+spp_transformer_desc\s*\*", src), name
        assert name in nat.SIGNATURES and hasattr(L, name)
    assert L.spp_abi_version() == 6 and "#define SPP_ABI_VERSION 6" in src
    assert set(re.findall(r"\b(spp_\w+)\s*\(", src)) == set(nat.SIGNATURES)


def test_descriptor_is_the_headers_struct():
    """field names in order, and the size the header's types give (4-byte int32_t / float, 8-byte int64_t / pointers,
    no padding: the four 4-byte fields come first)"""
    from salient_plusplus_amd import _native as nat
    body = re.search(r"typedef struct spp_transformer_desc \{(.*?)\} spp_transformer_desc;", _header(), flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)$", d).group(1) for d in decls]
    assert names == [f[0] for f in nat.TransformerDesc._fields_]
    size = sum(8 if "*" in d or d.startswith("int64_t") else 4 for d in decls)
    assert size == 160 and C.sizeof(nat.TransformerDesc) == size
    for (name, ctype), d in zip(nat.TransformerDesc._fields_, decls):
        assert C.sizeof(ctype) == (8 if "*" in d or d.startswith("int64_t") else 4), name
    assert nat.TransformerDesc.scale.offset == 8 and nat.TransformerDesc.rowptr_dev.offset == 16


_MEM = (C.c_char * 128)()
_PTRS = {"rowptr_dev", "col_dev", "q_dev", "k_dev", "v_dev", "out_dev", "row_max_dev", "row_sum_dev", "grad_out_dev",
         "grad_q_dev", "grad_k_dev", "grad_v_dev"}


def _desc(**kw):
    """a descriptor that passes every check (the pointers are host addresses: no check dereferences one)"""
    from salient_plusplus_amd import _native as nat
    ok = C.addressof(_MEM) + (-C.addressof(_MEM)) % 16
    d = dict(heads=4, x_elem=0, scale=0.25, rowptr_dev=ok, col_dev=ok, num_targets=3, num_sources=5, C=16, q_dev=ok,
             q_stride_elems=64, k_dev=ok, k_stride_elems=128, v_dev=ok, v_stride_elems=128, out_dev=ok,
             row_max_dev=ok, row_sum_dev=ok, grad_out_dev=ok, grad_q_dev=ok, grad_k_dev=ok, grad_v_dev=ok)
    for k, v in kw.items():
        d[k] = (ok + v if v is not None else None) if k in _PTRS else v
    return nat.TransformerDesc(**d)


# the refusals of spp.h f3y in the documented order: (fields, a word of the message); ORDER: two faults, the earlier one
# is reported
REFUSALS = [
    (dict(heads=3), "heads"), (dict(heads=0), "heads"), (dict(heads=16), "heads"),
    (dict(x_elem=3), "element code"), (dict(x_elem=-1), "element code"),
    (dict(C=0), "C % 4"), (dict(C=-4), "C % 4"), (dict(C=10), "C % 4"),
    (dict(C=12), "power of two"), (dict(C=24), "power of two"),
    (dict(heads=8, C=256), "<= 1024"), (dict(heads=1, C=2048), "<= 1024"),
    (dict(num_targets=-1), "T <= S"), (dict(num_targets=6), "T <= S"), (dict(num_sources=-1), "T <= S"),
    (dict(q_stride_elems=60), "stride"), (dict(k_stride_elems=66), "stride"), (dict(v_stride_elems=32), "stride"),
    (dict(rowptr_dev=None), "NULL"), (dict(q_dev=None), "NULL"), (dict(k_dev=None), "NULL"), (dict(v_dev=None), "NULL"),
    (dict(out_dev=None), "NULL"), (dict(row_max_dev=None), "NULL"), (dict(row_sum_dev=None), "NULL"),
    (dict(q_dev=8), "misaligned"), (dict(k_dev=4), "misaligned"), (dict(v_dev=8), "misaligned"),
    (dict(out_dev=4), "misaligned"), (dict(row_max_dev=2), "misaligned"), (dict(col_dev=4), "misaligned"),
    (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("inf")), "scale"),
    (dict(scale=float("nan")), "scale"),
]
ORDER = [(dict(heads=3, x_elem=9), "heads"), (dict(x_elem=9, C=10), "element code"), (dict(C=10, num_targets=-1), "C % 4"),
         (dict(C=12, heads=8), "power of two"), (dict(heads=8, C=256, num_targets=-1), "<= 1024"),
         (dict(heads=8, C=256, scale=0.0), "<= 1024"),
         (dict(num_targets=-1, q_stride_elems=1), "T <= S"), (dict(k_stride_elems=1, k_dev=None), "stride"),
         (dict(out_dev=None, q_dev=8), "NULL"), (dict(v_dev=8, scale=0.0), "misaligned")]


def _refused(entry, fields, word):
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    d = _desc(**fields)
    assert getattr(L, entry)(C.byref(d), None) == -1, (entry, fields)
    msg = L.spp_last_error().decode()
    assert entry in msg and word in msg, (fields, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_in_the_documented_order(entry):
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    assert getattr(L, entry)(None, None) == -1 and "NULL descriptor" in L.spp_last_error().decode()
    for fields, word in REFUSALS + ORDER:
        _refused(entry, fields, word)


def test_the_backwards_own_refusals():
    entry = "spp_transformer_backward"
    _refused(entry, dict(grad_out_dev=None), "NULL")
    _refused(entry, dict(grad_q_dev=None), "NULL")
    _refused(entry, dict(grad_q_dev=None, out_dev=4), "NULL")                   # NULL pointers before alignment
    for k in ("grad_out_dev", "grad_q_dev", "grad_k_dev", "grad_v_dev"):
        _refused(entry, {k: 8}, "misaligned")
    _refused(entry, dict(grad_k_dev=8, scale=0.0), "misaligned")                # alignment before the scale


def test_no_targets_returns_ok_before_the_rows_are_looked_at():
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    d = _desc(num_targets=0, q_dev=None, out_dev=None, scale=0.0, q_stride_elems=1)
    assert L.spp_transformer_forward(C.byref(d), None) == 0 and L.spp_transformer_backward(C.byref(d), None) == 0
    _refused("spp_transformer_forward", dict(num_targets=0, heads=3), "heads")  # the shape is still checked


# ------------------------------------------------------------------------------------------------ the module tree
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("root_weight", [False, True])
@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("concat", [False, True])
def test_state_dict_is_pygs(concat, beta, root_weight, bias):
    from salient_plusplus_amd.models import TransformerConv
    conv = TransformerConv(10, 6, heads=4, concat=concat, beta=beta, bias=bias, root_weight=root_weight)
    width = 24 if concat else 6
    want = {}
    for n in ("lin_key", "lin_query", "lin_value"):
        want.update({n + ".weight": (24, 10), n + ".bias": (24,)})
    if root_weight:
        want["lin_skip.weight"] = (width, 10)
        if bias:
            want["lin_skip.bias"] = (width,)
        if beta:
            want["lin_beta.weight"] = (1, 3 * width)
    sd = conv.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    other = TransformerConv(10, 6, heads=4, concat=concat, beta=beta, bias=bias, root_weight=root_weight)
    other.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), sd.values()))
    assert (conv.heads, conv.out_channels, conv.dropout) == (4, 6, 0.0)


def test_constructor_refusals():
    from salient_plusplus_amd.models import GraphTransformer, TransformerConv
    for heads in (0, -1, 2.0, "2", True):
        with pytest.raises(ValueError):
            TransformerConv(8, 4, heads=heads)
    for p in (1.0, -0.1, True, "0.5", float("nan")):
        with pytest.raises(ValueError):
            TransformerConv(8, 4, dropout=p)
    with pytest.raises(NotImplementedError, match="edge_dim"):
        TransformerConv(8, 4, edge_dim=3)
    conv = TransformerConv(8, 4, 2, False, True, 0.25, None, False, True)      # PyG's argument order
    assert (conv.heads, conv.concat, conv.beta, conv.dropout, conv.lin_skip.bias) == (2, False, True, 0.25, None)
    with pytest.raises(ValueError):
        GraphTransformer(16, 30, 5, 3, heads=4)
    with pytest.raises(ValueError):
        GraphTransformer(16, 32, 5, 3, heads=0)
    with pytest.raises(TypeError):
        GraphTransformer(16, 32, 5, 3, 4)


def test_get_model_type_and_the_models_shape():
    from salient_plusplus_amd import models
    assert models.get_model_type("transformer") is models.GraphTransformer
    assert models.get_model_type("Transformer") is models.GraphTransformer
    for name in ("sageclassic", "jknet", "arma"):
        with pytest.raises(NotImplementedError):
            models.get_model_type(name)
    with pytest.raises(ValueError):
        models.get_model_type("transformerconv")
    model = models.GraphTransformer(16, 32, 5, 3, heads=4, beta=True, attn_dropout=0.1)
    assert [(c.heads, c.out_channels, c.concat, c.beta, c.dropout) for c in model.convs] == \
        [(4, 8, True, True, 0.1), (4, 8, True, True, 0.1), (4, 5, False, True, 0.1)]
    assert not hasattr(model, "inference") and "batch-wise" in models.GraphTransformer.__doc__


# ------------------------------------------------------------------------------------------------ the reference
def _small_hop():
    """5 targets over 9 sources: a repeated entry (row 0 names 6 twice), diagonal entries (rows 1 and 3), an empty row
    (2), a row of one"""
    rows = [[6, 3, 6], [1, 8], [], [3], [0, 7, 5, 2]]
    rowptr = torch.tensor([0] + [sum(len(r) for r in rows[:i + 1]) for i in range(len(rows))])
    return G.Entries(rowptr, torch.tensor([j for r in rows for j in r]), 5, 9)


def _dense(ent, q, k, v, scale):
    """independent of the entry list: a [T, S] multiplicity matrix times exp(logits)"""
    mult = torch.zeros((ent.T, ent.S), dtype=q.dtype)
    for t in range(ent.T):
        for j in ent.col[int(ent.rowptr[t]):int(ent.rowptr[t + 1])].tolist():
            mult[t, j] += 1
    e = torch.einsum("thc,shc->hts", q, k) * scale
    e = e - torch.where(mult > 0, e, torch.full_like(e, -float("inf"))).amax(2, keepdim=True).nan_to_num(neginf=0.0)
    w = mult * torch.exp(e)
    den = w.sum(2, keepdim=True)
    alpha = torch.where(den > 0, w / den.clamp(min=1e-300), torch.zeros_like(w))
    return torch.einsum("hts,shc->thc", alpha, v)


def test_reference_against_a_dense_formulation():
    from salient_plusplus_amd.models import _transformer_reference
    ent = _small_hop()
    q, k, v, _g = (t.double() for t in G.inputs("model", ent, 2, 4, F32))
    out = _transformer_reference(q, k, v, ent.rowptr, ent.col, 0.5)
    assert out.dtype == F64 and out.shape == (5, 2, 4)
    torch.testing.assert_close(out, _dense(ent, q, k, v, 0.5), rtol=1e-12, atol=1e-14)
    assert bool((out[2] == 0).all()) and bool(torch.isfinite(out).all())
    torch.testing.assert_close(out[3], v[3])                               # a row of one diagonal entry: alpha = 1
    assert _transformer_reference(q.float(), k.float(), v.float(), ent.rowptr, ent.col, 0.5).dtype == F32
    assert _transformer_reference(q.bfloat16(), k.bfloat16(), v.bfloat16(), ent.rowptr, ent.col, 0.5).dtype == F32


@pytest.mark.parametrize("S", [200, 70])
@pytest.mark.parametrize("H,Cc", [(1, 4), (4, 8)])
@pytest.mark.parametrize("name", G.REGIMES)
def test_reference_in_float64_is_the_restatement(name, H, Cc, S):
    """forward, and autograd's gradients against the helper's closed forms"""
    from salient_plusplus_amd.models import _transformer_reference
    ent = G.entries_of(G.planted_hop(70, S))
    scale = G.scale32(Cc)
    q, k, v, g = (t.double() for t in G.inputs(name, ent, H, Cc, F32))
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = _transformer_reference(*leaves, ent.rowptr, ent.col, scale)
    out.backward(g)
    bw = G.backward(ent, q, k, v, g, scale)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-12)   # noqa: E731
    close(out.detach(), bw.fw.out)
    close(leaves[0].grad, bw.gq)
    close(leaves[1].grad, bw.gk)
    close(leaves[2].grad, bw.gv)
    empty = ent.n == 0
    assert bool(empty.any()) and bool((bw.fw.out[empty] == 0).all()) and bool((bw.fw.row_max[empty] == 0).all())
    assert bool((bw.fw.b_out[empty] == 0).all()) and bool((bw.gq[empty] == 0).all())
    if name == "zero":
        close(bw.fw.out, G.mean_of_v(ent, v))


def test_a_correct_fp32_computation_stays_inside_the_bounds_and_a_fault_leaves_them():
    """_transformer_reference in fp32 (two-pass, index_add) is inside every bound; a self loop added to every row, and
    dropped diagonal entries, are outside"""
    from salient_plusplus_amd.models import _transformer_reference
    hop = G.planted_hop(70, 200)
    ent = G.entries_of(hop)
    H, Cc = 2, 8
    scale = G.scale32(Cc)
    left = {"self_loop": False, "no_diag": False}
    for name in G.REGIMES:
        q, k, v, g = G.inputs(name, ent, H, Cc, F32)
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out = _transformer_reference(*leaves, ent.rowptr, ent.col, scale)
        out.backward(g)
        bw = G.backward(ent, q, k, v, g, scale)
        for what, got, ref, b in (("out", out.detach(), bw.fw.out, bw.fw.b_out), ("grad_q", leaves[0].grad, bw.gq, bw.b_gq),
                                  ("grad_k", leaves[1].grad, bw.gk, bw.b_gk), ("grad_v", leaves[2].grad, bw.gv, bw.b_gv)):
            ratio, where = G.worst(got, ref, b)
            assert ratio <= 1.0, (name, what, ratio, where)
        # the GAT convention on the same rows: hop.r / hop.s drop diagonals and append self loops
        order = torch.argsort(hop.r, stable=True)
        counts = torch.bincount(hop.r, minlength=hop.T)
        rp = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
        wrong = _transformer_reference(q, k, v, rp, hop.s[order], scale)
        left["self_loop"] |= G.worst(wrong, bw.fw.out, bw.fw.b_out)[0] > 1.0
        keep = hop.col != hop.row
        rp2 = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(hop.row[keep], minlength=hop.T), 0)])
        wrong = _transformer_reference(q, k, v, rp2, hop.col[keep], scale)
        left["no_diag"] |= G.worst(wrong, bw.fw.out, bw.fw.b_out)[0] > 1.0
    assert all(left.values()), left


def test_gradcheck_of_the_reference():
    from salient_plusplus_amd.models import _transformer_reference
    ent = _small_hop()
    q, k, v, _g = (t.double().requires_grad_(True) for t in G.inputs("model", ent, 2, 4, F32))
    assert torch.autograd.gradcheck(lambda a, b, c: _transformer_reference(a, b, c, ent.rowptr, ent.col, 0.5), (q, k, v))


# ------------------------------------------------------------------------------------------------ the layer and the model
def _adj(ent):
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    return SparseTensor(rowptr=ent.rowptr, col=ent.col, sparse_sizes=(ent.T, ent.S))


@pytest.mark.parametrize("heads,Cc,concat,beta,root_weight", [(4, 8, True, False, True), (3, 5, False, True, True),
                                                              (2, 12, True, True, True), (4, 8, False, False, False)])
def test_cpu_layer_is_the_float64_formula(heads, Cc, concat, beta, root_weight):
    from salient_plusplus_amd.models import TransformerConv
    torch.manual_seed(heads + Cc)
    ent = G.entries_of(G.planted_hop(70, 200))
    conv = TransformerConv(10, Cc, heads=heads, concat=concat, beta=beta, root_weight=root_weight)
    x = torch.randn(ent.S, 10)
    for xt in (x[:ent.T], torch.randn(ent.T, 10)):                 # the prefix, and a target block of its own
        out = conv((x, xt), _adj(ent))
        lin = lambda m, t: t.double() @ m.weight.double().t() + (m.bias.double() if m.bias is not None else 0)   # noqa: E731
        q = lin(conv.lin_query, xt).view(ent.T, heads, Cc).detach()
        k, v = (lin(m, x).view(ent.S, heads, Cc).detach() for m in (conv.lin_key, conv.lin_value))
        ref = _dense(ent, q, k, v, 1.0 / Cc ** 0.5)
        ref = ref.reshape(ent.T, -1) if concat else ref.mean(1)
        if root_weight:
            x_r = lin(conv.lin_skip, xt).detach()
            if beta:
                b = torch.sigmoid(torch.cat([ref, x_r, ref - x_r], -1) @ conv.lin_beta.weight.double().t()).detach()
                ref = b * x_r + (1 - b) * ref
            else:
                ref = ref + x_r
        assert out.dtype == F32 and out.shape == ref.shape
        torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-5)


def test_training_with_attention_dropout_takes_the_reference_and_torchs_mask(monkeypatch):
    from salient_plusplus_amd import models
    ent = G.entries_of(G.planted_hop(70, 200))
    seen, layer = [], []
    orig = models._transformer_reference
    monkeypatch.setattr(models, "_transformer_reference", lambda *a: (seen.append(a[-1]), orig(*a))[1])

    def fake_apply(q, k, v, rowptr, col, H, scale):
        layer.append(1)
        return orig(q.view(q.size(0), H, -1), k.view(k.size(0), H, -1), v.view(v.size(0), H, -1), rowptr, col, scale)

    monkeypatch.setattr(models._TransformerLayer, "apply", fake_apply)
    monkeypatch.setattr(models, "_transformer_kernels_read", lambda *a: True)   # even for rows the kernels would read
    conv = models.TransformerConv(10, 8, heads=2, dropout=0.5).train()
    x = torch.randn(ent.S, 10)
    torch.manual_seed(7)
    a = conv((x, x[:ent.T]), _adj(ent))
    torch.manual_seed(7)
    b = conv((x, x[:ent.T]), _adj(ent))
    c = conv((x, x[:ent.T]), _adj(ent))
    assert seen == [0.5, 0.5, 0.5] and not layer
    assert torch.equal(a, b) and not torch.equal(a, c)             # torch's generator decides the mask
    a.sum().backward()
    assert conv.lin_key.weight.grad is not None and bool(torch.isfinite(conv.lin_key.weight.grad).all())
    # F.dropout's mask on alpha, restated: the same seed gives the same output
    q, k, v = conv.lin_query(x[:ent.T]), conv.lin_key(x), conv.lin_value(x)
    torch.manual_seed(7)
    again = orig(q.view(ent.T, 2, 8), k.view(ent.S, 2, 8), v.view(ent.S, 2, 8), ent.rowptr, ent.col, 1.0 / 8 ** 0.5, 0.5)
    torch.testing.assert_close(a, again.reshape(ent.T, 16) + conv.lin_skip(x[:ent.T]))
    conv.eval()                                                     # eval mode: p = 0, the kernel path's condition
    conv((x, x[:ent.T]), _adj(ent))
    assert layer == [1]


def test_graph_transformer_trains_on_cpu_through_the_trainers_loop():
    from gatv2_f64 import sampled_batch
    from salient_plusplus_amd.fast_trainer.monkeypatch import Adj, SparseTensor
    from salient_plusplus_amd.fast_trainer.samplers import PreparedBatch
    from salient_plusplus_amd.fast_trainer.train import barebones_train_core, serial_train
    from salient_plusplus_amd.models import get_model_type
    torch.manual_seed(0)
    x, y, hops = sampled_batch(seeds=16)
    adjs = [Adj(SparseTensor(rowptr=rp, col=cl, sparse_sizes=(T, S)), None, (S, T)) for rp, cl, T, S in hops]
    batch = PreparedBatch(x, y.unsqueeze(-1), adjs, slice(0, 16))
    model = get_model_type("transformer")(16, 16, 5, 3, heads=4, beta=True, attn_dropout=0.1)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = []

    def eval_loss():
        model.eval()
        with torch.no_grad():
            return float(torch.nn.functional.nll_loss(model(x, adjs), y))

    before = eval_loss()
    for _ in range(3):
        serial_train(model, barebones_train_core, [(batch,)] * 4, opt, None, cb=lambda b, r: losses.append(float(r[0])))
    assert len(losses) == 12 and all(torch.isfinite(torch.tensor(losses)))
    assert eval_loss() < before
