"""CPU: attention dropout of GATv2Conv (spp.h f3x: spp_gatv2_forward_drop / spp_gatv2_backward_drop) without a device.
The two entries are exported, bound and declared with the documented argument list; they refuse what the header says in
the order it says, p included; T == 0 enqueues nothing.  The float64 restatement of tests/gatv2_drop_f64.py is checked on
its own: its closed-form gradients are autograd's, a correct fp32 computation of the dropped formulas stays inside every
bound, and three planted faults leave them."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gatv2_drop_f64 as GD  # noqa: E402
import gatv2_f64 as G  # noqa: E402

DROP = {"spp_gatv2_forward_drop": "spp_gatv2_forward", "spp_gatv2_backward_drop": "spp_gatv2_backward"}
F32 = torch.float32


def _lib():
    from salient_plusplus_amd import _native as nat
    return nat, nat.load()


def test_symbols_are_exported_bound_and_declared():
    nat, L = _lib()
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, base in DROP.items():
        assert hasattr(L, name), name
        res, args = nat.SIGNATURES[name]
        assert res is C.c_int and args == nat.SIGNATURES[base][1] + [C.c_float, C.c_int32, C.c_uint64], name
        decl = re.search(r"\bspp_status\s+%s\s*\((.*?)\);" % name, src, re.S).group(1)
        assert re.sub(r"\s+", " ", decl) == "const spp_gatv2_desc* desc, void* stream, float p, int32_t training, uint64_t seed"
    assert "#define SPP_ABI_VERSION 6" in header and L.spp_abi_version() == 6
    fields = re.search(r"typedef struct spp_gatv2_desc \{(.*?)\} spp_gatv2_desc;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in nat.Gatv2Desc._fields_]      # the descriptor is untouched


_MEM = (C.c_char * 128)()
_PTRS = {"rowptr_dev", "col_dev", "x_l_dev", "x_r_dev", "att_dev", "out_dev", "row_max_dev", "row_sum_dev", "grad_out_dev",
         "grad_x_l_dev", "grad_x_r_dev", "grad_att_dev"}


def _desc(**kw):
    """a descriptor that passes every check (the pointers are host addresses: no check dereferences one)"""
    nat, _ = _lib()
    ok = C.addressof(_MEM) + (-C.addressof(_MEM)) % 16
    d = dict(heads=4, x_elem=0, negative_slope=0.2, rowptr_dev=ok, col_dev=ok, num_targets=3, num_sources=5, C=16,
             x_l_dev=ok, x_l_stride_elems=64, x_r_dev=ok, x_r_stride_elems=64, att_dev=ok, out_dev=ok, row_max_dev=ok,
             row_sum_dev=ok, grad_out_dev=ok, grad_x_l_dev=ok, grad_x_r_dev=ok, grad_att_dev=ok)
    for k, v in kw.items():
        d[k] = (ok + v if v is not None else None) if k in _PTRS else v
    return nat.Gatv2Desc(**d)


NAN = float("nan")
# (descriptor fields, p, a word of the message): the refusals of spp.h f3v in their order with p right after the shape;
# most cases also plant the NEXT stage's fault to show which refusal comes first
REFUSALS = [
    (dict(heads=3), 2.0, "heads"), (dict(heads=0), 0.5, "heads"),
    (dict(x_elem=3), 2.0, "element code"),
    (dict(C=10), 2.0, "C % 4"), (dict(C=0), 0.5, "C % 4"),
    (dict(C=12), 2.0, "power of two"),
    (dict(heads=8, C=256), 2.0, "<= 1024"),
    (dict(num_targets=-1), 2.0, "T <= S"), (dict(num_targets=6), NAN, "T <= S"),
    (dict(), 1.0, "0 <= p < 1"), (dict(), -0.25, "0 <= p < 1"), (dict(), NAN, "0 <= p < 1"), (dict(), 1.5, "0 <= p < 1"),
    (dict(num_targets=0), 1.0, "0 <= p < 1"),                                 # before the T == 0 return
    (dict(x_l_stride_elems=60), -1.0, "0 <= p < 1"), (dict(x_l_dev=None), NAN, "0 <= p < 1"),   # before the rows
    (dict(x_l_stride_elems=60, x_l_dev=None), 0.5, "stride"), (dict(x_r_stride_elems=66), 0.0, "stride"),
    (dict(rowptr_dev=None), 0.5, "NULL"), (dict(out_dev=None, att_dev=8), 0.5, "NULL"), (dict(row_sum_dev=None), 0.5, "NULL"),
    (dict(x_l_dev=8), 0.5, "misaligned"), (dict(att_dev=8), 0.5, "misaligned"), (dict(col_dev=4), 0.6, "misaligned"),
]


def _refused(entry, fields, p, word, training=1):
    _, L = _lib()
    d = _desc(**fields)
    assert getattr(L, entry)(C.byref(d), None, p, training, 7) == -1, (entry, fields, p)
    msg = L.spp_last_error().decode()
    assert entry in msg and word in msg, (fields, p, msg)


@pytest.mark.parametrize("entry", list(DROP))
def test_refusals_in_the_documented_order(entry):
    _, L = _lib()
    assert getattr(L, entry)(None, None, 0.5, 1, 7) == -1 and "NULL descriptor" in L.spp_last_error().decode()
    for fields, p, word in REFUSALS:
        _refused(entry, fields, p, word)
    _refused(entry, dict(), 1.0, "0 <= p < 1", training=0)                    # in eval mode too


def test_the_backwards_own_refusals():
    entry = "spp_gatv2_backward_drop"
    _refused(entry, dict(grad_att_dev=None), 0.5, "grad_att")
    _refused(entry, dict(grad_att_dev=4), 0.5, "grad_att")
    _refused(entry, dict(grad_att_dev=None), 1.0, "0 <= p < 1")               # p before grad_att
    _refused(entry, dict(num_targets=-1, grad_att_dev=None), 1.0, "T <= S")   # the shape before p
    _refused(entry, dict(grad_att_dev=None, x_l_dev=None), 0.5, "grad_att")   # grad_att before the rows
    _refused(entry, dict(grad_out_dev=None), 0.5, "NULL")
    _refused(entry, dict(grad_x_r_dev=None), 0.5, "NULL")
    for k in ("grad_out_dev", "grad_x_l_dev", "grad_x_r_dev"):
        _refused(entry, {k: 8}, 0.5, "misaligned")


def test_forward_with_no_targets_enqueues_nothing():
    _, L = _lib()
    d = _desc(num_targets=0, x_l_dev=None, out_dev=None, rowptr_dev=None)
    for p, training in ((0.6, 1), (0.0, 1), (0.6, 0)):
        assert L.spp_gatv2_forward_drop(C.byref(d), None, p, training, 7) == 0


# ------------------------------------------------------------------------------------------------ the restatement
def _plain_formula(hop, x_l, x_r, att, slope, keep, scale):
    """row by row, nothing shared with the helpers; keep [(E + T), H] as the keep rule lays it out"""
    rows = []
    for t in range(hop.T):
        b, e = int(hop.rowptr[t]), int(hop.rowptr[t + 1])
        pos = torch.arange(b, e)[hop.col[b:e] != t]
        idx = torch.cat([hop.col[pos], torch.tensor([t])])
        kp = torch.cat([keep[pos], keep[hop.E + t:hop.E + t + 1]]).double()
        e_ = (torch.nn.functional.leaky_relu(x_l[idx] + x_r[t], slope) * att).sum(-1)     # [n, H]
        rows.append(torch.einsum("nh,nhc->hc", torch.softmax(e_, 0) * kp * scale, x_l[idx]))
    return torch.stack(rows)


@pytest.mark.parametrize("S", [200, 70])
@pytest.mark.parametrize("H", [1, 4])
def test_closed_form_gradients_are_autograds(H, S):
    hop = G.planted_hop(70, S)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-12)   # noqa: E731
    for slope, p in zip(G.SLOPES, (0.6, 0.5)):
        keep, ke = GD.mask(hop, H, p, 11 + H)
        assert 0 < int(keep.sum()) < keep.size and not keep[hop.E:].all()         # self loops are dropped too
        x_l, x_r, att, g = (t.double() for t in G.inputs("model", hop, H, 8, F32))
        att = 3 * att
        bw = GD.backward_drop(hop, x_l, x_r, att, g, slope, ke, p)
        # autograd of the float64 forward_drop itself
        leaves = [t.clone().requires_grad_(True) for t in (x_l, x_r, att)]
        out = GD.forward_drop(hop, *leaves, slope, ke, p).out
        out.backward(g)
        close(bw.fw.out, out.detach())
        for got, leaf in zip((bw.gxl, bw.gxr, bw.gatt), leaves):
            close(got, leaf.grad)
        # and of a row-by-row formula that shares nothing with it
        leaves = [t.clone().requires_grad_(True) for t in (x_l, x_r, att)]
        out = _plain_formula(hop, *leaves, slope, torch.from_numpy(keep), GD.scale_of(p))
        out.backward(g)
        close(bw.fw.out, out.detach())
        for got, leaf in zip((bw.gxl, bw.gxr, bw.gatt), leaves):
            close(got, leaf.grad)
        # row_max / row_sum and their bounds are the p = 0 restatement's own
        fw = G.forward(hop, x_l, x_r, att, slope)
        assert torch.equal(bw.fw.row_max, fw.row_max) and torch.equal(bw.fw.row_sum, fw.row_sum)
        assert torch.equal(bw.fw.bm, fw.bm) and torch.equal(bw.fw.bs, fw.bs)


def _emu(hop, x_l, x_r, att, g, slope, ke, p, fault=None, ke_bwd=None):
    """the dropped formulas in fp32 torch ops over the entry list (two-pass softmax), with a planted fault.
    ke [N, H] float: the mask per entry; ke_bwd: the backward's (another seed's: a fault)"""
    r, s, T, S = hop.r, hop.s, hop.T, hop.S
    H = att.size(0)
    sl = torch.tensor(slope, dtype=F32)
    scale = torch.tensor(GD.scale_of(p), dtype=F32)
    pre = x_l[s] + x_r[r]
    lr = torch.where(pre > 0, pre, pre * sl)
    e = (att * lr).sum(2)
    m = torch.full((T, H), -float("inf")).scatter_reduce(0, r.unsqueeze(1).expand(-1, H), e, "amax")
    w = torch.exp(e - m[r])
    ssum = torch.zeros((T, H)).index_add_(0, r, w)
    alpha = w / ssum[r]
    kf = ke.float().clone()
    if fault == "self_never_dropped":
        kf[hop.nk:] = 1.0
    kb = kf if ke_bwd is None else ke_bwd.float()
    out = torch.zeros((T,) + tuple(x_l.shape[1:])).index_add_(0, r, (kf * scale * alpha).unsqueeze(2) * x_l[s])
    go = (g * out).sum(2)
    gh = (g[r] * x_l[s]).sum(2)
    q = kb * scale
    ge = alpha * (q * gh - go[r])
    if fault == "dropped_send_nothing":                         # ge without the -alpha go term on dropped entries
        ge = torch.where(kb > 0, ge, torch.zeros_like(ge))
    dl = torch.where(pre > 0, torch.ones_like(pre), sl.expand_as(pre))
    t_r = ge.unsqueeze(2) * att * dl
    gxr = torch.zeros_like(out).index_add_(0, r, t_r)
    gxl = torch.zeros((S,) + tuple(x_l.shape[1:])).index_add_(0, s, (q * alpha).unsqueeze(2) * g[r] + t_r)
    gatt = (ge.unsqueeze(2) * lr).sum(0)
    return dict(out=out, row_max=m, row_sum=ssum, gxl=gxl, gxr=gxr, gatt=gatt)


def _ratios(got, bw):
    fw = bw.fw
    ref = dict(out=(fw.out, fw.b_out), row_max=(fw.row_max, fw.bm), row_sum=(fw.row_sum, fw.bs), gxl=(bw.gxl, bw.b_gxl),
               gxr=(bw.gxr, bw.b_gxr), gatt=(bw.gatt, bw.b_gatt))
    return {k: G.worst(got[k], *ref[k])[0] for k in ref}


@pytest.mark.parametrize("name", ["model", "wide", "zero", "selfmax"])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("slope", G.SLOPES)
def test_a_correct_fp32_computation_stays_inside_the_bounds(slope, H, name):
    hop = G.planted_hop(70, 200)
    for p in (0.5, 0.6):
        _, ke = GD.mask(hop, H, p, 5)
        x_l, x_r, att, g = G.inputs(name, hop, H, 8, F32)
        bw = GD.backward_drop(hop, x_l, x_r, att, g, slope, ke, p)
        ratios = _ratios(_emu(hop, x_l, x_r, att, g, slope, ke, p), bw)
        print(f"GATV2_DROP_HOST {name} H={H} slope={slope:.3g} p={p} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
        assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("fault", [None, "dropped_send_nothing", "self_never_dropped", "other_seed_in_backward"])
def test_a_planted_fault_leaves_the_bounds(fault):
    hop = G.planted_hop(70, 200)
    H, p, seed = 2, 0.6, 5
    _, ke = GD.mask(hop, H, p, seed)
    ke_bwd = GD.mask(hop, H, p, seed + 1)[1] if fault == "other_seed_in_backward" else None
    for name in G.REGIMES:
        x_l, x_r, att, g = G.inputs(name, hop, H, 8, F32)
        bw = GD.backward_drop(hop, x_l, x_r, att, g, G.SLOPES[0], ke, p)
        over = max(_ratios(_emu(hop, x_l, x_r, att, g, G.SLOPES[0], ke, p, fault, ke_bwd), bw).values())
        if fault is None:
            assert over <= 1.0, (name, over)                   # the emulation itself is inside
        elif over > 1.0:
            return
    assert fault is None, f"{fault}: inside every bound in every regime"
