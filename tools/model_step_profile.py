"""One resident batch of the bench workload, N optimisation steps of one of the models (models.get_model_type: SAGE, GAT,
GIN, SAGEResInception; and models.GCN) on it (fwd + bwd + Adam), timed; run under `rocprofv3 --kernel-trace --stats` for the per-kernel
table.
usage: model_step_profile.py [sage|gat|gatv2|transformer|gin|sageresinception|gcn] [steps=30] [workload=S-papers] [fused] [max] [norm] [reference] [--amp bf16] [--heads H] [attn=P]
norm: GCN built with normalize=True (gcn_norm's coefficients and the self term; the reference model's setting is False).
max: SAGE built with aggr="max" (csrc/aggregate_max.hip, layer by layer) instead of the mean's fused stack.
fused: GIN / SAGEResInception / GCN built with fused_norm=True (the BatchNorm tail on csrc/bn_act.hip).
--amp bf16: the forward and the loss under torch.autocast("cuda", dtype=torch.bfloat16), as a training loop would wrap them.
attn=P: GAT(..., attn_dropout=P): PyG's dropout on the attention coefficients, inside the GAT kernels (spp.h f3t); default 0.
--heads H: GAT(..., heads=H) (default 1: the reference model): hidden layers of H heads of 256 // H, the last one averaged.
gatv2: models.GATv2 (csrc/gatv2.hip), with --heads and attn= as GAT.
transformer: models.GraphTransformer (csrc/transformer_conv.hip), with --heads and attn= as GAT (attn > 0 trains on the
kernels with the mask drawn inside them: spp.h f4a).  reference: the same model with every layer sent to
models._transformer_reference, the plain-torch path (attn > 0: torch's own mask there), for the comparison of DESIGN
section 7 f3y."""
import contextlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from salient_plusplus_amd import fast_sampler as fs  # noqa: E402
from salient_plusplus_amd.fast_trainer.samplers import FastSampler, FastSamplerConfig  # noqa: E402
from salient_plusplus_amd.fast_trainer.transferers import DevicePrefetcher  # noqa: E402
from salient_plusplus_amd import models  # noqa: E402
from salient_plusplus_amd.models import GCN, get_model_type  # noqa: E402
from salient_plusplus_amd.synthetic import make_workload  # noqa: E402

argv = sys.argv[1:]
amp = None
if "--amp" in argv:
    i = argv.index("--amp")
    amp = argv[i + 1]
    del argv[i:i + 2]
    if amp != "bf16":
        sys.exit(f"--amp {amp}: only bf16 is supported")
heads = 1
if "--heads" in argv:
    i = argv.index("--heads")
    heads = int(argv[i + 1])
    del argv[i:i + 2]
attn = 0.0
for a in [a for a in argv if a.startswith("attn=")]:
    attn = float(a.split("=", 1)[1])
    argv.remove(a)
fused = "fused" in argv
use_max = "max" in argv
norm = "norm" in argv
reference = "reference" in argv
argv = [a for a in argv if a not in ("fused", "max", "norm", "reference")]
arch = argv[0] if len(argv) > 0 else "sage"
steps = int(argv[1]) if len(argv) > 1 else 30
wl = make_workload(argv[2] if len(argv) > 2 else "S-papers", seed=1234, device=torch.device("cuda", 0))
dev = torch.device("cuda", 0)
cfg = FastSamplerConfig(
    x_cpu=wl.x, x_gpu=torch.empty(0), y=wl.y.unsqueeze(-1), rowptr=wl.rowptr, col=wl.col, idx=wl.train_idx[:8 * wl.batch_size],
    batch_size=wl.batch_size, sizes=wl.fanouts, skip_nonfull_batch=False, pin_memory=False, distributed=False,
    partition_book=None, cache=fs.Cache(), force_exact_num_batches=True, exact_num_batches=8,
    count_remote_frequency=False, use_cache=False)
it = DevicePrefetcher([dev], iter(FastSampler(2, 8, cfg)))
batch = next(it)[0]
torch.cuda.synchronize()
ATTN = ("gat", "gatv2", "transformer")
if heads != 1 and arch not in ATTN:
    sys.exit("--heads: GAT, GATv2 and GraphTransformer only")
if attn and arch not in ATTN:
    sys.exit("attn=: GAT, GATv2 and GraphTransformer only")
if reference and arch != "transformer":
    sys.exit("reference: GraphTransformer only")
if reference:
    models._transformer_kernels_read = lambda *a: False
if fused and arch not in ("gin", "sageresinception", "gcn"):
    sys.exit("fused: GIN, SAGEResInception and GCN only")
if norm and arch != "gcn":
    sys.exit("norm: GCN only")
if use_max and arch != "sage":
    sys.exit("max: SAGE only")
kw = {"heads": heads} if heads != 1 else {}
if attn:
    kw["attn_dropout"] = attn
if use_max:
    kw["aggr"] = "max"
if fused:
    kw["fused_norm"] = True
if norm:
    kw["normalize"] = True
model = (GCN if arch == "gcn" else get_model_type(arch))(wl.x.size(1), 256, 47, 3, **kw).to(dev)
if arch in ATTN:
    assert [c.heads for c in model.convs] == [heads] * 3, "the model was not built with --heads"
opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)    # one multi-tensor launch per step


def autocast():
    return torch.autocast("cuda", dtype=torch.bfloat16) if amp == "bf16" else contextlib.nullcontext()


def step():
    opt.zero_grad(set_to_none=True)
    with autocast():
        loss = torch.nn.functional.nll_loss(model(batch.x, batch.adjs), batch.y.reshape(-1))
    loss.backward()
    opt.step()
    return loss


for _ in range(5):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    loss = step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
print(f"MODEL_STEP {arch}{' aggr=max' if use_max else ''}{' normalize' if norm else ''}{f' heads={heads}' if heads != 1 else ''}{f' attn={attn:g}' if attn else ''}{' fused_norm' if fused else ''}{' reference-path' if reference else ''}{' amp=' + amp if amp else ''} {dt * 1e3:.3f} ms/step on a resident batch: {batch.x.size(0)} nodes, "
      f"{[int(a.adj_t.nnz()) for a in batch.adjs]} edges, (S, T) {[tuple(int(v) for v in a.size) for a in batch.adjs]}, loss {float(loss):.4f}", flush=True)
