"""Float64 restatement of the ResGated kernels (csrc/resgated.hip, spp.h f4g) as a loop over the targets, on the CPU, and the
hops and inputs the tests use.  A helper: no tests in here.  fp32 / bf16 inputs convert to float64 exactly."""
import torch

HOPS, REGIMES = ["planted", "T0", "E0", "long", "random"], ["zero", "saturated", "mixed"]
# planted, 5 targets over 9 sources: a repeated entry (3, 3) and a diagonal one in row 0, row 1 empty, source 8 unnamed
_FIXED = {"planted": ([[3, 3, 0], [], [7], [1, 2, 4, 5], [4, 6, 2]], 9), "T0": ([], 4), "E0": ([[], [], []], 5)}


def hop(name):
    """(rowptr, col, S).  long: one row of 130.  random: 70 targets, 200 sources, source 7 in every row, 150.. in none."""
    gen = torch.Generator().manual_seed(7)
    if name in _FIXED:
        rows, S = _FIXED[name]
    elif name == "long":
        rows, S = [torch.randint(0, 140, (130,), generator=gen).tolist()], 140
    else:
        rows, S = [], 200
        for _ in range(70):
            r = torch.randint(0, 150, (int(torch.randint(0, 7, (1,), generator=gen)),), generator=gen).tolist()
            r.insert(int(torch.randint(0, len(r) + 1, (1,), generator=gen)), 7)
            rows.append(r)
    rowptr = torch.tensor([0] + [len(r) for r in rows]).cumsum(0)
    return rowptr, torch.tensor([j for r in rows for j in r], dtype=torch.int64), S


def inputs(regime, T, S, D, dtype, seed=0):
    """k [T, D], q, v [S, D] in dtype, g [T, D] fp32; k + q near 0 ("zero"), near +-20, both signs in every row, or of a few units"""
    gen = torch.Generator().manual_seed(seed + D)
    scale = {"zero": 0.05, "saturated": 0.5, "mixed": 3.0}[regime]
    k, q, v, g = (c * torch.randn(s, generator=gen) for c, s in ((scale, (T, D)), (scale, (S, D)), (1, (S, D)), (1, (T, D))))
    if regime == "saturated":
        k = k + 20.0 * (1 - 2 * ((torch.arange(T).view(T, 1) + torch.arange(D)) % 2))
    return k.to(dtype), q.to(dtype), v.to(dtype), g


def restate(k, q, v, g, rowptr, col):
    """(out, grad_k, grad_q, grad_v) in float64; the gradients are torch.autograd's"""
    k, q, v = (t.detach().double().cpu().requires_grad_() for t in (k, q, v))
    rows = [col[rowptr[i]:rowptr[i + 1]] for i in range(k.size(0))]
    out = torch.stack([(torch.sigmoid(k[i] + q[j]) * v[j]).sum(0) for i, j in enumerate(rows)]) if rows else 0 * k + 0 * (q + v).sum()
    out.backward(g.double().cpu())
    return out.detach(), k.grad, q.grad, v.grad
