"""CPU: GATv2 (csrc/gatv2.hip, spp.h f3v, models.GATv2Conv / GATv2) without a device.  The two entries are exported, bound
and declared, and refuse what the header says in the order it says; the module tree is PyG's; the float64 restatement
of tests/gatv2_f64.py is checked on its own: its closed-form gradients are autograd's, a correct fp32 computation
(_gatv2_reference through GATv2Conv, forward and autograd gradients) stays inside every bound, and three planted faults
leave them; GATv2 trains on CPU through fast_trainer's loop."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gatv2_f64 as G  # noqa: E402

ENTRIES = ["spp_gatv2_forward", "spp_gatv2_backward"]
F32 = torch.float32


def test_symbols_are_exported_bound_and_declared():
    from salient_plusplus_amd import _native as nat
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spp.h")).read(), flags=re.S)
    L = nat.load()
    for name in ENTRIES:
        assert re.search(r"\bspp_status\s+" + name + r"\s*\(\s*const\s+spp_gatv2_desc\s*\*", src), name
        assert name in nat.SIGNATURES and hasattr(L, name)
    assert L.spp_abi_version() == 6
    declared = set(re.findall(r"\b(spp_\w+)\s*\(", src))
    assert declared == set(nat.SIGNATURES), declared ^ set(nat.SIGNATURES)
    fields = re.search(r"typedef struct spp_gatv2_desc \{(.*?)\} spp_gatv2_desc;", src, flags=re.S).group(1)
    names = re.findall(r"(\w+);", fields)
    assert names == [f[0] for f in nat.Gatv2Desc._fields_]


def _desc(**kw):
    """a descriptor that passes every check (the pointers are host addresses: no check dereferences one)"""
    from salient_plusplus_amd import _native as nat
    buf = (C.c_char * 64).from_address(C.addressof(_desc.mem) + (-C.addressof(_desc.mem)) % 16)
    ok = C.addressof(buf)
    d = dict(heads=4, x_elem=0, negative_slope=0.2, rowptr_dev=ok, col_dev=ok, num_targets=3, num_sources=5, C=16,
             x_l_dev=ok, x_l_stride_elems=64, x_r_dev=ok, x_r_stride_elems=64, att_dev=ok, out_dev=ok, row_max_dev=ok,
             row_sum_dev=ok, grad_out_dev=ok, grad_x_l_dev=ok, grad_x_r_dev=ok, grad_att_dev=ok)
    d.update(kw)
    return nat.Gatv2Desc(**d), ok


_desc.mem = (C.c_char * 128)()

# every refusal of spp.h f3v, in the documented order: (fields, a word of the message); each later case keeps the earlier
# fields valid, and ORDER pairs check that with two faults the earlier one is reported
REFUSALS = [
    (dict(heads=3), "heads"), (dict(heads=0), "heads"), (dict(heads=16), "heads"),
    (dict(x_elem=3), "element code"), (dict(x_elem=-1), "element code"),
    (dict(C=0), "C % 4"), (dict(C=-4), "C % 4"), (dict(C=10), "C % 4"),
    (dict(C=12), "power of two"), (dict(C=24), "power of two"),
    (dict(heads=8, C=256), "<= 1024"), (dict(heads=1, C=2048), "<= 1024"),
    (dict(num_targets=-1), "T <= S"), (dict(num_targets=6), "T <= S"), (dict(num_sources=-1), "T <= S"),
    (dict(x_l_stride_elems=60), "stride"), (dict(x_r_stride_elems=66), "stride"),
    (dict(rowptr_dev=None), "NULL"), (dict(x_l_dev=None), "NULL"), (dict(x_r_dev=None), "NULL"), (dict(att_dev=None), "NULL"),
    (dict(out_dev=None), "NULL"), (dict(row_max_dev=None), "NULL"), (dict(row_sum_dev=None), "NULL"),
    (dict(x_l_dev=8), "misaligned"), (dict(x_r_dev=4), "misaligned"), (dict(att_dev=8), "misaligned"),
    (dict(out_dev=4), "misaligned"), (dict(row_max_dev=2), "misaligned"), (dict(col_dev=4), "misaligned"),
]
ORDER = [(dict(heads=3, x_elem=9), "heads"), (dict(x_elem=9, C=10), "element code"), (dict(C=10, num_targets=-1), "C % 4"),
         (dict(C=12, heads=8), "power of two"), (dict(heads=8, C=256, num_targets=-1), "<= 1024"),
         (dict(num_targets=-1, x_l_stride_elems=1), "T <= S"), (dict(x_l_stride_elems=1, x_l_dev=None), "stride"),
         (dict(out_dev=None, att_dev=8), "NULL")]


def _refused(entry, fields, word):
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    d, ok = _desc()
    for k, v in fields.items():
        setattr(d, k, (ok + v if v is not None else None) if k in _PTRS else v)
    assert getattr(L, entry)(C.byref(d), None) == -1, (entry, fields)
    msg = L.spp_last_error().decode()
    assert entry in msg and word in msg, (fields, msg)


_PTRS = {"rowptr_dev", "col_dev", "x_l_dev", "x_r_dev", "att_dev", "out_dev", "row_max_dev", "row_sum_dev", "grad_out_dev",
         "grad_x_l_dev", "grad_x_r_dev", "grad_att_dev"}


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_in_the_documented_order(entry):
    from salient_plusplus_amd import _native as nat
    L = nat.load()
    assert getattr(L, entry)(None, None) == -1 and "NULL descriptor" in L.spp_last_error().decode()
    for fields, word in REFUSALS + ORDER:
        _refused(entry, fields, word)


def test_the_backwards_own_refusals():
    entry = "spp_gatv2_backward"
    _refused(entry, dict(grad_att_dev=None), "grad_att")
    _refused(entry, dict(grad_att_dev=4), "grad_att")
    _refused(entry, dict(num_targets=-1, grad_att_dev=None), "T <= S")          # the shape comes first
    _refused(entry, dict(grad_att_dev=None, x_l_dev=None), "grad_att")          # grad_att before the rows
    _refused(entry, dict(grad_out_dev=None), "NULL")
    _refused(entry, dict(grad_x_r_dev=None), "NULL")
    _refused(entry, dict(x_l_dev=None, grad_out_dev=None), "NULL buffer")
    for k in ("grad_out_dev", "grad_x_l_dev", "grad_x_r_dev"):
        _refused(entry, {k: 8}, "misaligned")


def test_forward_with_no_targets_enqueues_nothing():
    from salient_plusplus_amd import _native as nat
    d, _ = _desc(num_targets=0, x_l_dev=None, out_dev=None)
    assert nat.load().spp_gatv2_forward(C.byref(d), None) == 0


# ------------------------------------------------------------------------------------------------ the module tree
@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("concat", [False, True])
def test_state_dict_is_pygs(concat, bias, share):
    from salient_plusplus_amd.models import GATv2Conv
    conv = GATv2Conv(10, 6, heads=4, concat=concat, bias=bias, share_weights=share)
    sd = conv.state_dict()
    want = {"att": (1, 4, 6), "lin_l.weight": (24, 10), "lin_r.weight": (24, 10)}
    if bias:
        want.update({"lin_l.bias": (24,), "lin_r.bias": (24,), "bias": (24,) if concat else (6,)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert (conv.lin_r is conv.lin_l) == share
    assert (sd["lin_l.weight"].data_ptr() == sd["lin_r.weight"].data_ptr()) == share
    other = GATv2Conv(10, 6, heads=4, concat=concat, bias=bias, share_weights=share)
    other.load_state_dict(sd)
    assert (conv.heads, conv.out_channels, conv.negative_slope, conv.dropout) == (4, 6, 0.2, 0.0)


def test_constructor_refuses_what_gatconv_refuses():
    from salient_plusplus_amd.models import GATv2, GATv2Conv
    for heads in (0, -1, 2.0, "2"):
        with pytest.raises(ValueError):
            GATv2Conv(8, 4, heads=heads)
    for p in (1.0, -0.1, True, "0.5", float("nan")):
        with pytest.raises(ValueError):
            GATv2Conv(8, 4, dropout=p)
    assert GATv2Conv(8, 4, 2, True, 0.1, 0.25, False, True).share_weights      # PyG's argument order
    with pytest.raises(ValueError):
        GATv2(16, 30, 5, 3, heads=4)
    with pytest.raises(TypeError):
        GATv2(16, 32, 5, 3, 4)


def test_get_model_type_and_the_inference_refusals():
    from salient_plusplus_amd import inference, models
    assert models.get_model_type("gatv2") is models.GATv2 and models.get_model_type("GATv2") is models.GATv2
    for name, cls in (("sage", models.SAGE), ("gat", models.GAT), ("gin", models.GIN),
                      ("sageresinception", models.SAGEResInception), ("gcn", models.GCN)):
        assert models.get_model_type(name) is cls
    for name in ("sageclassic", "jknet", "arma"):
        with pytest.raises(NotImplementedError):
            models.get_model_type(name)
    with pytest.raises(ValueError):
        models.get_model_type("gatv3")
    model = models.GATv2(16, 32, 5, 3, heads=4)
    assert [(c.heads, c.out_channels, c.concat, c.bias is None) for c in model.convs] == \
        [(4, 8, True, True), (4, 8, True, True), (4, 5, False, True)]
    x, rowptr, col = torch.zeros(4, 16), torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    from inference_method import assert_method_is_the_function
    assert_method_is_the_function(model, x, rowptr, col)     # the method is layerwise_inference, which takes the model
    with pytest.raises(NotImplementedError, match=r"^layerwise_inference: layer 0 has heads = 3"):
        models.GATv2(16, 36, 5, 2, heads=3).inference(x, rowptr, col)


# ------------------------------------------------------------------------------------------------ the restatement
def _plain_formula(hop, x_l, x_r, att, slope):
    """row by row, nothing shared with gatv2_f64.forward"""
    rows = []
    for t in range(hop.T):
        c = hop.col[int(hop.rowptr[t]):int(hop.rowptr[t + 1])]
        idx = torch.cat([c[c != t], torch.tensor([t])])
        e = (torch.nn.functional.leaky_relu(x_l[idx] + x_r[t], slope) * att).sum(-1)      # [n, H]
        rows.append(torch.einsum("nh,nhc->hc", torch.softmax(e, 0), x_l[idx]))
    return torch.stack(rows)


@pytest.mark.parametrize("S", [200, 70])
@pytest.mark.parametrize("H", [1, 4])
def test_closed_form_gradients_are_autograds(H, S):
    hop = G.planted_hop(70, S)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-12)   # noqa: E731
    for slope in G.SLOPES:
        x_l, x_r, att, g = (t.double() for t in G.inputs("model", hop, H, 8, F32))
        att = 3 * att
        leaves = [t.clone().requires_grad_(True) for t in (x_l, x_r, att)]
        out = _plain_formula(hop, *leaves, slope)
        out.backward(g)
        bw = G.backward(hop, x_l, x_r, att, g, slope)
        close(bw.fw.out, out.detach())
        close(bw.gxl, leaves[0].grad)
        close(bw.gxr, leaves[1].grad)
        close(bw.gatt, leaves[2].grad)


def _adj(hop):
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    return SparseTensor(rowptr=hop.rowptr, col=hop.col, sparse_sizes=(hop.T, hop.S))


def _fp32_layer(hop, name, H, Cc, slope):
    """GATv2Conv on CPU fp32 (the _gatv2_reference path) with lin_l = lin_r = identity-free random maps, set up so that
    the projected rows ARE the regime's rows: x = [x_l | x_r-padded], W_l = [I 0], W_r = [0 I].  Returns what it computed
    and the float64 values and bounds for the same fp32 rows."""
    from salient_plusplus_amd.models import GATv2Conv
    D = H * Cc
    x_l, x_r, att, g = G.inputs(name, hop, H, Cc, F32)
    x = torch.zeros((hop.S, 2 * D))
    x[:, :D] = x_l.view(hop.S, D)
    x[:hop.T, D:] = x_r.view(hop.T, D)
    conv = GATv2Conv(2 * D, Cc, heads=H, negative_slope=slope, bias=False)
    with torch.no_grad():
        conv.lin_l.weight.copy_(torch.eye(D, 2 * D))
        conv.lin_r.weight.copy_(torch.cat([torch.zeros(D, D), torch.eye(D)], 1))
        conv.att.copy_(att.view(1, H, Cc))
    x = x.requires_grad_(True)
    kept = {}
    hl = conv.lin_l.register_forward_hook(lambda m, i, o: (o.retain_grad(), kept.__setitem__("x_l", o))[0])
    hr = conv.lin_r.register_forward_hook(lambda m, i, o: (o.retain_grad(), kept.__setitem__("x_r", o))[0])
    out = conv((x, x[:hop.T]), _adj(hop))
    hl.remove(), hr.remove()
    out.backward(g.view(hop.T, D))
    assert torch.equal(kept["x_l"].detach().view_as(x_l), x_l) and torch.equal(kept["x_r"].detach().view_as(x_r), x_r)
    bw = G.backward(hop, x_l, x_r, att, g, slope)
    return conv, x, kept, out, bw, g


@pytest.mark.parametrize("name", G.REGIMES)
@pytest.mark.parametrize("H", [1, 2, 4, 8])
@pytest.mark.parametrize("slope", G.SLOPES)
def test_a_correct_fp32_computation_stays_inside_the_bounds(slope, H, name):
    """_gatv2_reference through GATv2Conv: forward, and autograd's gradients of the rows, att, x, lin_l and lin_r"""
    Cc = 8
    hop = G.planted_hop(70, 200)
    conv, x, kept, out, bw, g = _fp32_layer(hop, name, H, Cc, slope)
    T, S, D = hop.T, hop.S, H * Cc
    got = {"out": (out.detach().view(T, H, Cc), bw.fw.out, bw.fw.b_out),
           "grad_xl": (kept["x_l"].grad.view(S, H, Cc), bw.gxl, bw.b_gxl),
           "grad_xr": (kept["x_r"].grad.view(T, H, Cc), bw.gxr, bw.b_gxr),
           "grad_att": (conv.att.grad.view(H, Cc), bw.gatt, bw.b_gatt)}
    # the projections' gradients: GEMMs of the fp32 row gradients autograd held, (n + 1) u M each
    gl, gr, xd = kept["x_l"].grad.double(), kept["x_r"].grad.double(), x.detach().double()
    Wl, Wr = conv.lin_l.weight.detach().double(), conv.lin_r.weight.detach().double()
    gx, mx = gl @ Wl, gl.abs() @ Wl.abs()
    gx[:T] += gr @ Wr
    mx[:T] += gr.abs() @ Wr.abs()
    got["grad_x"] = (x.grad, gx, G.G2 * (2 * D + 2) * G.U * mx)
    got["grad_lin_l"] = (conv.lin_l.weight.grad, gl.t() @ xd, G.G2 * (S + 1) * G.U * (gl.abs().t() @ xd.abs()))
    got["grad_lin_r"] = (conv.lin_r.weight.grad, gr.t() @ xd[:T], G.G2 * (T + 1) * G.U * (gr.abs().t() @ xd[:T].abs()))
    bad = {}
    for k, (a, ref, b) in got.items():
        ratio, where = G.worst(a, ref, b)
        print(f"GATV2_F64_HOST {name} H={H} slope={slope:.3g} {k}={ratio:.3f}")
        if not ratio <= 1.0:
            bad[k] = (ratio, where)
    assert not bad, bad


def _emu(hop, x_l, x_r, att, slope, fault=None):
    """a two-pass fp32 forward over the entry list of `hop`, with a planted fault"""
    r, s, T = hop.r, hop.s, hop.T
    sl = torch.tensor(slope, dtype=F32)
    pre = x_l[s] + x_r[r]
    if fault == "v1":                                          # LeakyReLU AFTER the dot with att: GAT v1
        raw = (att * pre).sum(2)
        e = torch.where(raw > 0, raw, raw * sl)
    else:
        e = (att * torch.where(pre > 0, pre, pre * sl)).sum(2)
    H = att.size(0)
    m = torch.full((T, H), -float("inf")).scatter_reduce(0, r.unsqueeze(1).expand(-1, H), e, "amax")
    w = torch.exp(e - m[r])
    ssum = torch.zeros((T, H)).index_add_(0, r, w)
    msg = x_l[s].clone()
    if fault == "self_reads_xr":                               # the self loop's message taken from x_r
        msg[hop.nk:] = x_r
    out = torch.zeros((T,) + tuple(x_l.shape[1:])).index_add_(0, r, (w / ssum[r]).unsqueeze(2) * msg)
    return out, m, ssum


@pytest.mark.parametrize("fault", [None, "keep_diag", "v1", "self_reads_xr"])
def test_a_planted_fault_leaves_the_bounds(fault):
    hop = G.planted_hop(70, 200)
    run_on = G.Hop(hop.rowptr, hop.col, hop.T, hop.S, keep_diag=True) if fault == "keep_diag" else hop
    for name in G.REGIMES:
        x_l, x_r, att, _g = G.inputs(name, hop, 2, 8, F32)
        fw = G.forward(hop, x_l, x_r, att, G.SLOPES[0])
        out, m, ssum = _emu(run_on, x_l, x_r, att, G.SLOPES[0], fault)
        over = max(G.worst(out, fw.out, fw.b_out)[0], G.worst(ssum, fw.row_sum, fw.bs)[0], G.worst(m, fw.row_max, fw.bm)[0])
        if fault is None:
            assert over <= 1.0, (name, over)                   # the emulation itself is inside
        elif over > 1.0:
            return
    assert fault is None, f"{fault}: inside every bound in every regime"


# ------------------------------------------------------------------------------------------------ the layer and the model
@pytest.mark.parametrize("heads,Cc,share,concat", [(4, 8, False, True), (3, 5, False, False), (2, 12, True, True),
                                                   (4, 8, True, False)])
def test_cpu_layer_is_the_float64_formula(heads, Cc, share, concat):
    from salient_plusplus_amd.models import GATv2Conv
    torch.manual_seed(heads + Cc)
    hop = G.planted_hop(70, 200)
    conv = GATv2Conv(10, Cc, heads=heads, concat=concat, share_weights=share)
    torch.nn.init.normal_(conv.bias)
    x = torch.randn(hop.S, 10)
    for xt in (x[:hop.T], torch.randn(hop.T, 10)):               # the prefix, and a target block of its own
        out = conv((x, xt), _adj(hop))
        x_l = (x.double() @ conv.lin_l.weight.double().t() + conv.lin_l.bias.double()).view(hop.S, heads, Cc)
        x_r = (xt.double() @ conv.lin_r.weight.double().t() + conv.lin_r.bias.double()).view(hop.T, heads, Cc)
        ref = _plain_formula(hop, x_l.detach(), x_r.detach(), conv.att.detach().double().view(heads, Cc), 0.2)
        ref = (ref.reshape(hop.T, -1) if concat else ref.mean(1)) + conv.bias.detach().double()
        assert out.dtype == F32 and out.shape == ref.shape
        torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-5)


def test_gatv2_trains_on_cpu_through_the_trainers_loop():
    from salient_plusplus_amd.fast_trainer.monkeypatch import Adj
    from salient_plusplus_amd.fast_trainer.samplers import PreparedBatch
    from salient_plusplus_amd.fast_trainer.train import barebones_train_core, serial_train
    from salient_plusplus_amd.models import get_model_type
    torch.manual_seed(0)
    x, y, hops = G.sampled_batch(seeds=16)
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    adjs = [Adj(SparseTensor(rowptr=rp, col=cl, sparse_sizes=(T, S)), None, (S, T)) for rp, cl, T, S in hops]
    batch = PreparedBatch(x, y.unsqueeze(-1), adjs, slice(0, 16))
    model = get_model_type("gatv2")(16, 16, 5, 3, heads=4, share_weights=True, attn_dropout=0.1)
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
