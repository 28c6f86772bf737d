"""How many values one forward takes from torch's CPU generator: the seeds of the kernels' dropout masks come from it
(models._draw_seed), so their number and order are part of what torch.manual_seed repeats.  Pinned for the flagship SAGE
and the three attention models with attention dropout, in training and in eval mode, on the kernel path of each."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# 3 layers, heads = 2, hidden 8 (C = 4, the narrowest head the kernels accept), 4 classes, 16-wide fp32 features
IN, HIDDEN, CLASSES, LAYERS, HEADS = 16, 8, 4, 3, 2
NODES = (12, 8, 4, 2)                        # a 3-hop MFG, outermost hop first: (S, T) = (12, 8), (8, 4), (4, 2)

# model name -> (constructor keywords, the Function of its kernel path, its calls per forward, draws per training forward)
#   SAGE: _SageStack.forward draws one activation seed per non-final layer                                     -> 2
#   the attention models: one seed per conv -- _gat_kernels_forward (GAT, through _GatLayerMH), _attn_forward
#   (_GATv2Layer, _TransformerLayer) -- and one per relu_dropout between the layers (_ReluDropout.forward)  -> 3 + 2
CASES = {
    "SAGE": ({}, "_SageStack", 1, 2),
    "GAT": (dict(heads=HEADS, attn_dropout=0.5), "_GatLayerMH", 3, 5),
    "GATv2": (dict(heads=HEADS, attn_dropout=0.5), "_GATv2Layer", 3, 5),
    "GraphTransformer": (dict(heads=HEADS, attn_dropout=0.5), "_TransformerLayer", 3, 5),
}


def _adjs():
    """rows of 1, 2, 3, 1, ... entries, every source in range; targets are the first rows of the sources"""
    from salient_plusplus_amd.fast_trainer.monkeypatch import SparseTensor
    adjs = []
    for S, T in zip(NODES[:-1], NODES[1:]):
        rows = [[(t + 5 * j) % S for j in range(1 + t % 3)] for t in range(T)]
        rowptr = torch.tensor([0] + [len(r) for r in rows]).cumsum(0)
        col = torch.tensor([c for r in rows for c in r])
        adjs.append((SparseTensor(rowptr=rowptr.cuda(), col=col.cuda(), sparse_sizes=(T, S)), None, (S, T)))
    return adjs


def _state_after(draws):
    torch.manual_seed(7)
    for _ in range(draws):
        torch.empty((), dtype=torch.int64).random_()
    return torch.get_rng_state()


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(CASES))
def test_cpu_generator_draws_of_one_forward(name, training, monkeypatch):
    from salient_plusplus_amd import models
    kw, node, calls_want, draws = CASES[name]
    model = getattr(models, name)(IN, HIDDEN, CLASSES, LAYERS, **kw).cuda().train(training)
    x = torch.randn(NODES[0], IN).cuda()
    adjs = _adjs()
    calls = []
    fn = getattr(models, node)
    orig = fn.apply
    monkeypatch.setattr(fn, "apply", lambda *a: (calls.append(len(a)), orig(*a))[1])
    torch.manual_seed(7)
    out = model(x, adjs)
    state = torch.get_rng_state()
    assert out.shape == (NODES[-1], CLASSES) and bool(torch.isfinite(out).all())
    assert len(calls) == calls_want, f"{name} left its kernel path: {len(calls)} calls of {node}"
    n = draws if training else 0
    print(f"{name} training={training}: expecting {n} draws")
    assert torch.equal(state, _state_after(n)), f"{name}: not {n} draws from torch's CPU generator"
    if n:
        assert not torch.equal(state, _state_after(n - 1))      # (the comparison tells n from n - 1)
