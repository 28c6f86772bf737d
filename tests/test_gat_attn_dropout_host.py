"""CPU-only: attention dropout of GATConv / GAT (spp.h f3t) without a device -- the constructor arguments and the state
dict, the eval and training behaviour of the plain-torch path, the new C entries against the header and every refusal
they make before a launch, and the numpy restatement of the keep rule (models._attn_keep_reference) against the
binomial statistics a dropout mask must have."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SPP_OK, SPP_ERR_INVALID = 0, -1
_FAKE = 0x7F0000001000                                   # never dereferenced: every refusal comes before a launch
DROP = {"spp_gat_mh_aggregate_forward_drop": "spp_gat_mh_aggregate_forward",
        "spp_gat_mh_aggregate_backward_drop": "spp_gat_mh_aggregate_backward",
        "spp_gat_mh_aggregate_backward_gather_drop": "spp_gat_mh_aggregate_backward_gather"}


def _lib():
    from salient_plusplus_amd import _native as nat
    return nat, nat.load()


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def _hop(T=6, S=11, seed=0):
    """a small CSR hop with an empty row, a diagonal entry and a repeated source, as a SparseTensor-like object"""
    g = torch.Generator().manual_seed(seed)
    deg = torch.tensor([0, 1, 3, 4, 2, 5])[:T]
    rowptr = torch.zeros(T + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, S, (int(rowptr[-1]),), generator=g)
    col[1] = 2                                           # row 2's first entry is its diagonal
    col[2] = col[3]

    class Adj:
        def csr(self):
            return rowptr, col, None

        def sparse_sizes(self):
            return (T, S)
    return Adj(), T, S


# ---- constructor, state dict ----
def test_the_modules_construct_and_their_state_dict_is_that_of_p_0():
    from salient_plusplus_amd.models import GAT, GATConv
    conv = GATConv(8, 4, heads=2, dropout=0.6)
    assert conv.dropout == 0.6 and _shapes(conv) == _shapes(GATConv(8, 4, heads=2))
    assert GATConv(8, 4).dropout == 0.0
    model = GAT(8, 8, 3, 2, attn_dropout=0.6)
    assert [c.dropout for c in model.convs] == [0.6, 0.6] and _shapes(model) == _shapes(GAT(8, 8, 3, 2))
    heads = GAT(8, 8, 3, 3, heads=4, attn_dropout=0.5)
    assert [c.dropout for c in heads.convs] == [0.5] * 3 and _shapes(heads) == _shapes(GAT(8, 8, 3, 3, heads=4))
    with pytest.raises(TypeError):
        GAT(8, 8, 3, 2, 1, 0.6)                          # keyword only
    # PyG's position: after negative_slope
    assert GATConv(8, 4, 2, True, 0.2, 0.25).dropout == 0.25


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf"), "0.5", None, True, [0.5]])
def test_dropout_outside_0_1_or_not_a_number_is_refused_at_construction(bad):
    from salient_plusplus_amd.models import GAT, GATConv
    with pytest.raises(ValueError, match="dropout"):
        GATConv(8, 4, heads=2, dropout=bad)
    with pytest.raises(ValueError, match="dropout"):
        GAT(8, 8, 3, 2, attn_dropout=bad)


# ---- the plain-torch path on the CPU ----
@pytest.mark.parametrize("heads,concat", [(2, True), (3, False)])
def test_eval_mode_on_the_cpu_equals_the_p_0_module_bit_for_bit(heads, concat):
    from salient_plusplus_amd.models import GATConv
    adj, T, S = _hop()
    torch.manual_seed(1)
    a, b = GATConv(8, 4, heads=heads, concat=concat), GATConv(8, 4, heads=heads, concat=concat, dropout=0.6)
    b.load_state_dict(a.state_dict())
    x = torch.randn(S, 8)
    a.eval(), b.eval()
    assert torch.equal(a((x, x[:T]), adj), b((x, x[:T]), adj))
    # p = 0 in training is today's path too
    a.train()
    assert torch.equal(a((x, x[:T]), adj), b((x, x[:T]), adj))


def test_training_on_the_cpu_is_repeatable_under_manual_seed_and_differs_from_eval():
    from salient_plusplus_amd.models import GATConv
    adj, T, S = _hop()
    torch.manual_seed(2)
    conv = GATConv(8, 4, heads=2, dropout=0.6).train()
    x = torch.randn(S, 8)
    outs = []
    for _ in range(2):
        torch.manual_seed(77)
        outs.append(conv((x, x[:T]), adj))
    assert torch.equal(outs[0], outs[1])
    torch.manual_seed(78)
    assert not torch.equal(conv((x, x[:T]), adj), outs[0])
    assert not torch.equal(conv.eval()((x, x[:T]), adj), outs[0])
    outs[0].sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in conv.parameters())


# ---- the C entries ----
def test_the_entries_exist_with_the_documented_argument_lists_and_the_abi_version_stays():
    nat, L = _lib()
    header = open(os.path.join(ROOT, "include", "spp.h")).read()
    tail = [ctypes.c_float, ctypes.c_int32, ctypes.c_uint64]
    for name, base in DROP.items():
        assert hasattr(L, name) and f" {name}(" in header, name
        res, args = nat.SIGNATURES[name]
        assert res is ctypes.c_int and args == nat.SIGNATURES[base][1] + tail, name
        decl = re.search(r"spp_status %s\((.*?)\);" % name, header, re.S).group(1)
        assert re.sub(r"\s+", " ", decl).endswith("void* stream, float p, int32_t training, uint64_t seed"), name
        old = re.search(r"spp_status %s\((.*?)\);" % base, header, re.S).group(1)
        assert re.sub(r"\s+", " ", decl).startswith(re.sub(r"\s+", " ", old)), name
    assert hasattr(L, "spp_gat_mh_attn_keep") and " spp_gat_mh_attn_keep(" in header
    assert nat.SIGNATURES["spp_gat_mh_attn_keep"] == (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                                                      ctypes.c_float, ctypes.c_uint64, ctypes.c_void_p,
                                                                      ctypes.c_void_p])
    assert "#define SPP_ABI_VERSION 6" in header


def _refused(L, name, call, cases):
    for what, (over, text) in cases.items():
        assert call(over) == SPP_ERR_INVALID, (name, what)
        msg = L.spp_last_error()
        assert name.encode() in msg and text in msg, (name, what, msg)


_P = dict(rowptr=_FAKE, col=_FAKE, T=5, S=9, E=12, x=_FAKE, elem=0, xs=8, K=8, H=2, a_src=_FAKE, a_dst=_FAKE,
          slope=0.2, z=_FAKE, rmax=_FAKE, rsum=_FAKE, g=_FAKE, v_src=_FAKE, v_dst=_FAKE, gx=_FAKE, gas=_FAKE,
          gad=_FAKE, ws=_FAKE, nbytes=1 << 20, p=0.5, training=1, seed=3)

# shared by the three entries, in the order the entries check: head count, element code, K (gat_check), then p, then
# the sizes, then the buffers; each case also plants the NEXT stage's fault to show which refusal comes first
_COMMON = {
    "heads 3": (dict(H=3, p=2.0), b"heads must be"),
    "heads 0": (dict(H=0), b"heads must be"),
    "unknown element code": (dict(elem=9, p=2.0), b"unknown element code"),
    "K % 4": (dict(K=6, p=2.0), b"K % 4"),
    "row stride below K": (dict(xs=4), b"K % 4"),
    "p = 1": (dict(p=1.0, T=-1), b"0 <= p < 1"),
    "p < 0": (dict(p=-0.25, T=-1), b"0 <= p < 1"),
    "p NaN": (dict(p=float("nan")), b"0 <= p < 1"),
    "p = 1 in eval mode": (dict(p=1.0, training=0), b"0 <= p < 1"),
    "negative T": (dict(T=-1, rowptr=None), b"size"),
    "NULL rowptr": (dict(rowptr=None), b"NULL"),
    "NULL z": (dict(z=None), b"NULL"),
    "misaligned z": (dict(z=_FAKE + 4), b"unaligned"),
    "misaligned a_src at H = 2": (dict(a_src=_FAKE + 4), b"unaligned"),
}


def _fwd(L, **o):
    a = dict(_P, **o)
    return L.spp_gat_mh_aggregate_forward_drop(a["rowptr"], a["col"], a["T"], a["x"], a["elem"], a["xs"], a["K"], a["H"],
                                               a["a_src"], a["a_dst"], a["slope"], a["z"], a["rmax"], a["rsum"], None,
                                               a["p"], a["training"], a["seed"])


def _bwd(L, **o):
    a = dict(_P, **o)
    return L.spp_gat_mh_aggregate_backward_drop(a["rowptr"], a["col"], a["T"], a["x"], a["elem"], a["xs"], a["K"],
                                                a["H"], a["a_src"], a["a_dst"], a["slope"], a["z"], a["rmax"], a["rsum"],
                                                a["g"], a["gx"], a["gas"], a["gad"], None, a["p"], a["training"],
                                                a["seed"])


def _gather(L, **o):
    a = dict(_P, **o)
    return L.spp_gat_mh_aggregate_backward_gather_drop(
        a["rowptr"], a["col"], a["T"], a["S"], a["E"], a["x"], a["elem"], a["xs"], a["K"], a["H"], a["a_src"],
        a["a_dst"], a["slope"], a["z"], a["rmax"], a["rsum"], a["g"], a["v_src"], a["v_dst"], a["gx"], a["gas"], a["gad"],
        a["ws"], a["nbytes"], None, a["p"], a["training"], a["seed"])


def test_forward_refusals_come_before_any_launch():
    _, L = _lib()
    _refused(L, "spp_gat_mh_aggregate_forward_drop", lambda o: _fwd(L, **o), _COMMON)
    assert _fwd(L, T=0, rowptr=None, z=None) == SPP_OK                       # nothing to do: no look at the pointers
    assert _fwd(L, T=0, p=1.0) == SPP_ERR_INVALID                            # p is checked before the sizes


def test_backward_refusals_come_before_any_launch():
    _, L = _lib()
    cases = dict(_COMMON)
    cases.update({"NULL grad_z": (dict(g=None), b"NULL"), "NULL grad_a_dst": (dict(gad=None), b"NULL"),
                  "misaligned grad_z": (dict(g=_FAKE + 8), b"unaligned")})
    _refused(L, "spp_gat_mh_aggregate_backward_drop", lambda o: _bwd(L, **o), cases)
    assert _bwd(L, T=0, rowptr=None) == SPP_OK
    assert _bwd(L, T=0, p=-1.0) == SPP_ERR_INVALID


def test_backward_gather_refusals_come_before_any_launch():
    _, L = _lib()
    cases = dict(_COMMON)
    cases["negative T"] = (dict(T=-1), b"bad sizes")
    cases.update({
        "S < T": (dict(S=4), b"bad sizes"),
        "negative E": (dict(E=-1), b"bad sizes"),
        "p before the sizes": (dict(p=1.0, S=4), b"0 <= p < 1"),
        "S beyond int32": (dict(S=1 << 31), b"32-bit"),
        "E beyond int32": (dict(E=1 << 31), b"32-bit"),
        "NULL v_src": (dict(v_src=None), b"NULL"),
        "NULL grad_x": (dict(gx=None), b"NULL"),
        "misaligned workspace": (dict(ws=_FAKE + 8), b"unaligned"),
        "workspace too small": (dict(nbytes=16), b"workspace too small"),
    })
    _refused(L, "spp_gat_mh_aggregate_backward_gather_drop", lambda o: _gather(L, **o), cases)
    assert _gather(L, T=0, S=0, E=0, rowptr=None) == SPP_OK


def test_attn_keep_refusals_come_before_any_launch():
    _, L = _lib()

    def call(o):
        a = dict(dict(E=12, T=5, H=2, p=0.5, seed=1, keep=_FAKE), **o)
        return L.spp_gat_mh_attn_keep(a["E"], a["T"], a["H"], a["p"], a["seed"], a["keep"], None)

    _refused(L, "spp_gat_mh_attn_keep", call, {
        "negative E": (dict(E=-1, H=3), b"negative size"),
        "negative T": (dict(T=-1, p=1.0), b"negative size"),
        "heads 3": (dict(H=3, p=1.0), b"heads must be"),
        "heads 16": (dict(H=16), b"heads must be"),
        "p = 1": (dict(p=1.0, keep=None), b"0 <= p < 1"),
        "p < 0": (dict(p=-0.5), b"0 <= p < 1"),
        "p NaN": (dict(p=float("nan")), b"0 <= p < 1"),
        "NULL mask": (dict(keep=None), b"NULL"),
    })
    assert call(dict(E=0, T=0, keep=None)) == SPP_OK


# ---- the keep rule in numpy ----
N_DRAWS = 200_000                                        # E + T entries: H * N_DRAWS draws
SEEDS = (0x5EED0001, 0xC0FFEE1234567)                    # fixed; chosen on the CPU so that the restatement passes


def _band(share, want, n):
    sd = math.sqrt(want * (1.0 - want) / n)
    return abs(share - want) <= 4.0 * sd, f"share {share:.6f} want {want:.6f} +- 4 * {sd:.2e}"


@pytest.mark.parametrize("H", [1, 2, 4, 8])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.6])
def test_keep_reference_has_the_statistics_of_a_dropout_mask(p, H):
    from salient_plusplus_amd.models import _attn_keep_reference
    E, T = N_DRAWS - 1000, 1000
    masks = [_attn_keep_reference(E, T, H, p, s) for s in SEEDS]
    for m in masks:
        assert m.shape == (E + T, H) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
        ok, why = _band(float(m.mean()), 1.0 - p, m.size)
        assert ok, ("all draws", why)
        for h in range(H):                               # per head, and the self-loop block on its own scale
            ok, why = _band(float(m[:, h].mean()), 1.0 - p, E + T)
            assert ok, ("head", h, why)
        ok, why = _band(float(m[E:].mean()), 1.0 - p, T * H)
        assert ok, ("self loops", why)
        for h in range(H - 1):                           # two heads of one entry share a hash, not a draw
            ok, why = _band(float((m[:, h] != m[:, h + 1]).mean()), 2 * p * (1 - p), E + T)
            assert ok, ("heads", h, h + 1, why)
        ok, why = _band(float((m[:-1, 0] != m[1:, 0]).mean()), 2 * p * (1 - p), E + T - 1)
        assert ok, ("neighbouring entries", why)         # (at H = 1 they share a hash)
    ok, why = _band(float((masks[0] != masks[1]).mean()), 2 * p * (1 - p), masks[0].size)
    assert ok, ("two seeds", why)
    # the split into E entries and T self loops does not move a draw; the seed is taken modulo 2^64
    assert np.array_equal(masks[0], _attn_keep_reference(E - 7, T + 7, H, p, SEEDS[0]))
    assert np.array_equal(masks[0][:50], _attn_keep_reference(40, 10, H, p, SEEDS[0] + (1 << 64)))


@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_keep_reference_keeps_everything_at_p_0(H):
    from salient_plusplus_amd.models import _attn_keep_reference
    assert bool(_attn_keep_reference(N_DRAWS, 100, H, 0.0, SEEDS[1]).all())


def test_keep_reference_by_hand():
    """draw 0 and 1 of seed 0 are the halves of mix64(0) = 0, so both are kept at any p < 1; a python-int restatement of
    mix64 for a few further indices"""
    from salient_plusplus_amd.models import _attn_keep_reference
    M = (1 << 64) - 1

    def mix64(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    for H, p, seed in ((1, 0.6, 0), (2, 0.5, 12345), (4, 0.6, M), (8, 0.1, 1 << 63)):
        got = _attn_keep_reference(5, 3, H, p, seed)
        thr = int((1.0 - float(np.float32(p))) * 4294967296.0)
        for entry in range(8):
            for h in range(H):
                i = entry * H + h
                r = mix64((seed + (i >> 1) * 0x9E3779B97F4A7C15) & M)
                draw = (r >> 32) if i & 1 else (r & 0xFFFFFFFF)
                assert got[entry, h] == (1 if draw < thr else 0), (H, p, seed, entry, h)
