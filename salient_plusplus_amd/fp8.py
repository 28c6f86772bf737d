"""Opt-in fp8 feature tables: one byte per element (OCP e4m3, ``torch.float8_e4m3fn``) and one power-of-two exponent
per feature COLUMN.

The table is the pair (``q``, ``scale_log2``):
  * ``q``          ``torch.float8_e4m3fn [N, F]``, row-major, rows exactly F bytes apart, F a multiple of 16;
  * ``scale_log2`` ``int8 [F]``, every entry in [-64, 63].
Dequantised value:  ``v[i, c] = float32(q[i, c]) * 2^scale_log2[c]``, computed in fp32.  Every e4m3 code is exact in fp32
and the product with a power of two in that range is exact, so ``v`` is one well-defined fp32 number.  A consumer of fp16
(the delivered ``PreparedBatch.x``) gets ``v`` rounded once, to nearest even: ``v.to(torch.float16)``.

``quantize_e4m3`` is plain torch (CPU or GPU, same result); the data path reads such a table through HIP kernels
(csrc/gather_fp8.hip, csrc/aggregate.hip) when it is handed to ``FastSamplerConfig.x_cpu`` in the place of the feature
tensor (single-GPU, non-distributed session).

Partitioned sessions (``distributed=True``, native exchange): every rank hands its own rows over as
``FastSamplerConfig(x_gpu=Fp8Features(<this rank's rows>), x_cpu=torch.empty(0), ...)``, a VIP cache as
``Cache(rank, P, cached_vertices, Fp8Features(<the cached rows>))``.  The exchange moves the e4m3 bytes (F per row instead
of 2F) and the delivery dequantises while it assembles the batch, so a row quantised by its owner is dequantised by its
requester: EVERY rank (and every cache) must use the SAME per-column exponents -- the Session checks that when it is
created.  A process that sees the whole table gets them from one call, and slices quantise identically::

    e = column_scales(x)                                   # int8[F]: what quantize_e4m3(x) would choose
    mine = quantize_e4m3(x[lo:hi], scale_log2=e)           # == quantize_e4m3(x).rows(slice(lo, hi)), byte for byte

Ranks that never see the whole table agree on the exponents with one element-wise MAX all-reduce: the exponent of a
column is monotone in its largest magnitude, so the maximum of the ranks' exponents is the exponent of the whole column
(an all-zero slice reports 0 where the table may need a negative exponent: the result is then larger than
``quantize_e4m3`` of the whole table would choose -- still valid, never an overflow)::

    e = column_scales(x_local).to(torch.int32).cuda()
    torch.distributed.all_reduce(e, op=torch.distributed.ReduceOp.MAX)
    mine = quantize_e4m3(x_local, scale_log2=e.to(torch.int8).cpu())"""
from typing import Optional

import torch

__all__ = ["Fp8Features", "quantize_e4m3", "column_scales", "save", "load", "E4M3_MAX", "SCALE_LOG2_MIN", "SCALE_LOG2_MAX"]

E4M3_MAX = 448.0                        # largest finite e4m3fn value (0x7E); 0x7F / 0xFF are NaN, there is no infinity
SCALE_LOG2_MIN, SCALE_LOG2_MAX = -64, 63
_FP8 = torch.float8_e4m3fn


def _exp2_f32(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for an integer tensor e in [-126, 127], built from the exponent bits (exact by construction)"""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


class Fp8Features:
    """The pair (q, scale_log2) of an fp8 feature table; reads like a 2-D feature tensor where the sampler façade asks
    for sizes (``shape`` / ``size`` / ``dim`` / ``numel`` / ``device`` / ``is_cuda``)."""
    __slots__ = ("q", "scale_log2")

    def __init__(self, q: torch.Tensor, scale_log2: torch.Tensor):
        if not (isinstance(q, torch.Tensor) and q.dtype == _FP8 and q.dim() == 2):
            raise ValueError("Fp8Features: q must be a 2-D torch.float8_e4m3fn tensor")
        if q.size(1) % 16 != 0:
            raise ValueError(f"Fp8Features: the feature width ({q.size(1)}) must be a multiple of 16 (rows are read in "
                             "16-byte pieces)")
        if not (isinstance(scale_log2, torch.Tensor) and scale_log2.dtype == torch.int8 and scale_log2.dim() == 1 and
                scale_log2.numel() == q.size(1)):
            raise ValueError("Fp8Features: scale_log2 must be an int8 tensor with one entry per feature column")
        if scale_log2.device != q.device:
            raise ValueError("Fp8Features: q and scale_log2 must live on one device")
        if scale_log2.numel() and (int(scale_log2.min()) < SCALE_LOG2_MIN or int(scale_log2.max()) > SCALE_LOG2_MAX):
            raise ValueError(f"Fp8Features: scale_log2 outside [{SCALE_LOG2_MIN}, {SCALE_LOG2_MAX}]")
        self.q = q.contiguous()                          # row stride exactly F bytes
        self.scale_log2 = scale_log2.contiguous()

    @classmethod
    def _wrap(cls, q, scale_log2) -> "Fp8Features":
        """the pair without re-validation (tensors derived from a checked table: moved, sliced)"""
        f = object.__new__(cls)
        f.q, f.scale_log2 = q.contiguous(), scale_log2.contiguous()
        return f

    # -- what reads like the feature tensor --
    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    @property
    def is_cuda(self):
        return self.q.is_cuda

    @property
    def dtype(self):
        return _FP8

    @property
    def requires_grad(self):
        return False

    def size(self, dim=None):
        return self.q.shape if dim is None else self.q.shape[dim]

    def dim(self):
        return 2

    def numel(self):
        return self.q.numel()

    def element_size(self):
        return 1

    def __len__(self):
        return self.q.size(0)

    def __repr__(self):
        return f"Fp8Features(shape={tuple(self.q.shape)}, device={self.q.device})"

    # -- movement --
    def to(self, device, non_blocking=False):
        return Fp8Features._wrap(self.q.to(device, non_blocking=non_blocking),
                                 self.scale_log2.to(device, non_blocking=non_blocking))

    def pin_memory(self):
        return Fp8Features._wrap(self.q.pin_memory(), self.scale_log2.pin_memory())

    def rows(self, index) -> "Fp8Features":
        """The table of the rows ``index`` (a slice or an int64 tensor), same column scales"""
        return Fp8Features._wrap(self.q.view(torch.uint8)[index].view(_FP8), self.scale_log2)

    # -- values --
    def dequantize(self, dtype=torch.float16) -> torch.Tensor:
        """v = float32(q) * 2^scale_log2 (exact), then rounded once to ``dtype`` (fp32: returned as it is)"""
        v = self.q.to(torch.float32) * _exp2_f32(self.scale_log2)
        return v if dtype == torch.float32 else v.to(dtype)

    def save(self, path):
        save(self, path)

    @staticmethod
    def load(path, map_location="cpu") -> "Fp8Features":
        return load(path, map_location)


def _check_table(x, who):
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype in (torch.float16, torch.float32, torch.bfloat16)):
        raise ValueError(f"{who}: needs a 2-D fp16 / fp32 / bf16 tensor")
    if x.size(1) % 16 != 0:
        raise ValueError(f"{who}: the feature width ({x.size(1)}) must be a multiple of 16")
    # in row slabs (the fp32 temporaries of a whole table would be a multiple of the table itself)
    return max(1, (1 << 26) // max(1, x.size(1)))


def column_scales(x: torch.Tensor) -> torch.Tensor:
    """int8[F] on x's device: the per-column exponents ``quantize_e4m3(x)`` chooses.  Per column c with
    m = max_i |x[i, c]|:  clamp(ceil(log2(m / 448)), -64, 63) -- the smallest exponent with m * 2^-e <= 448 -- and 0
    for an all-zero column.  Non-finite input is a ValueError."""
    step = _check_table(x, "column_scales")
    m = torch.zeros(x.size(1), dtype=torch.float32, device=x.device)
    for r in range(0, x.size(0), step):
        a = x[r:r + step].to(torch.float32).abs()
        if not bool(torch.isfinite(a).all()):
            raise ValueError("quantize_e4m3: the table holds inf or NaN")
        m = torch.maximum(m, a.amax(dim=0))
    # ceil(log2(m / 448)) without a logarithm: m = f * 2^k with f in [0.5, 1) and 448 = 0.875 * 2^9, so
    # m <= 448 * 2^e  <=>  f * 2^k <= 0.875 * 2^(9 + e):  e = k - 9 when f <= 0.875, else k - 8.  (fp32 subnormal m: frexp
    # normalises them, and the clamp at -64 applies long before.)
    f, k = torch.frexp(m)
    e = torch.where(f <= 0.875, k - 9, k - 8)
    e = torch.where(m == 0, torch.zeros_like(e), e).clamp(SCALE_LOG2_MIN, SCALE_LOG2_MAX)
    return e.to(torch.int8)


def quantize_e4m3(x: torch.Tensor, scale_log2: Optional[torch.Tensor] = None) -> Fp8Features:
    """Quantise an fp16 / fp32 / bf16 [N, F] table (F % 16 == 0), on the CPU or the GPU with the same result.

    ``scale_log2`` None: the exponents are ``column_scales(x)``;  q = (x * 2^-e).clamp(-448, 448) cast to e4m3 (round to
    nearest even).  The clamp is required: torch's cast does not saturate (500.0 becomes the NaN code).  Non-finite input
    is a ValueError, so q never holds a NaN code.

    ``scale_log2`` given (an integer tensor [F], every entry in [-64, 63]): x is quantised against THESE exponents --
    a slice of a table against the table's exponents, a rank's partition against the exponents all ranks agreed on.  A
    value that would overflow e4m3 under its column's exponent (|x| * 2^-e > 448) is a ValueError, not a saturation."""
    step = _check_table(x, "quantize_e4m3")
    if scale_log2 is None:
        e = column_scales(x)
    else:
        if not (isinstance(scale_log2, torch.Tensor) and scale_log2.dim() == 1 and scale_log2.numel() == x.size(1) and
                not scale_log2.dtype.is_floating_point and scale_log2.dtype != torch.bool):
            raise ValueError("quantize_e4m3: scale_log2 must be an integer tensor with one entry per feature column")
        if scale_log2.numel() and (int(scale_log2.min()) < SCALE_LOG2_MIN or int(scale_log2.max()) > SCALE_LOG2_MAX):
            raise ValueError(f"quantize_e4m3: scale_log2 outside [{SCALE_LOG2_MIN}, {SCALE_LOG2_MAX}]")
        e = scale_log2.to(device=x.device, dtype=torch.int8)
    inv = _exp2_f32(-e.to(torch.int32))
    q = torch.empty(x.shape, dtype=_FP8, device=x.device)
    for r in range(0, x.size(0), step):
        v = x[r:r + step].to(torch.float32) * inv
        if scale_log2 is not None and not bool((v.abs() <= E4M3_MAX).all()):      # (NaN and inf fail the comparison too)
            if not bool(torch.isfinite(x[r:r + step].to(torch.float32)).all()):
                raise ValueError("quantize_e4m3: the table holds inf or NaN")
            raise ValueError("quantize_e4m3: a value overflows e4m3 under the given scale_log2 (|x| * 2^-e > 448)")
        q[r:r + step] = v.clamp(-E4M3_MAX, E4M3_MAX).to(_FP8)
    return Fp8Features(q, e)


def save(f: Fp8Features, path) -> None:
    """the two tensors in one torch.save dict"""
    torch.save({"format": "spp-fp8-e4m3-colscale-1", "q": f.q.cpu().view(torch.uint8), "scale_log2": f.scale_log2.cpu()}, path)


def load(path, map_location="cpu") -> Fp8Features:
    d = torch.load(path, map_location=map_location)
    if not (isinstance(d, dict) and d.get("format") == "spp-fp8-e4m3-colscale-1"):
        raise ValueError(f"{path}: not an fp8 feature table written by salient_plusplus_amd.fp8.save")
    return Fp8Features(d["q"].view(_FP8), d["scale_log2"])
