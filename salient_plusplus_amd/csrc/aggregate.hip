// f3: mean aggregation over an MFG hop's CSR -- the message passing of SAGEConv(aggr='mean')
// (reference: driver/models.py:19-56 uses torch_geometric.nn.SAGEConv on (x, x_target), adj_t):
//     out[t,:]     = (1 / max(deg t, 1)) * sum_{e in row t} x[col[e],:]               forward
//     grad_x[s,:] += grad_out[t,:] / max(deg t, 1)   for every edge (t, s)            backward
// HBM/L2 bound gather-reduce: LPR lanes share a target row and stride over the feature dimension in
// 16-B pieces; the first layer reads the batch's fp16 features directly (fp16 -> fp32 is exact, so
// this equals converting the whole matrix first, which the reference model does, minus one pass
// over 150 MB).  The linear layers stay library GEMMs.
#include "act_keep.hip.h"
#include "agg_rows.hip.h"
#include "elem_io.hip.h"
#include "transpose_hop.hip.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <type_traits>

namespace spp {

// the same as float4, element 4*i .. 4*i+3 of p (the backward kernels' form)
__device__ __forceinline__ float4 ld4(const float* p, int64_t i) { return reinterpret_cast<const float4*>(p)[i]; }
__device__ __forceinline__ float4 ld4(const bf16* p, int64_t i) {
  const f4 v = load4(p + 4 * i);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4(float* p, int64_t i, float4 v) { reinterpret_cast<float4*>(p)[i] = v; }
__device__ __forceinline__ void st4(bf16* p, int64_t i, float4 v) { store4(p + 4 * i, f4{v.x, v.y, v.z, v.w}); }

// fp8 rows, their column factors (ColScale4 / ColScale1) and the row sources (Rows<Tin, Src>): agg_rows.hip.h

// ---- ReLU + dropout (driver/models.py:47-48: x = F.relu(x); x = F.dropout(x, p=0.5)) ----
// keep / drop from a counter-based generator: element i of the call with `seed` is kept iff
// hash(seed, i) < (1 - p) * 2^32; the output is relu(x) / (1 - p) where kept, 0 elsewhere.
// mix64, ActArgs and relu_dropout4 (the keep rule) live in act_keep.hip.h, shared with bn_act.hip

// ---- the epilogues: what a target's sum becomes (the backward kernels take the same types) ----
//   Mean (SAGEConv): sum / max(deg t, 1), with concat_target followed by the target's own row as fp32 ([mean | x_target]).
//     kAct (dense fp32 rows, VEC4): x is a PRE-activation; relu + dropout are applied to every row as it is loaded --
//     the same values a k_relu_dropout_fwd pass over x would have produced (same generator, same indices).
//   Sum (GINConv): fmaf(s, x[t], sum); with s == 0 the target's row is not read (a foreign x_target is added by the caller).
template <bool kAct_>
struct Mean {
  static constexpr bool kSum = false, kAct = kAct_;
  static constexpr float s = 0.f;
  int concat_target;
  ActArgs act;
};
struct Sum {
  static constexpr bool kSum = true, kAct = false;
  static constexpr int concat_target = 0;
  float s;
};

// LPR lanes share a target row; VEC4: F % 4 == 0 and rows 16-B (fp32) / 8-B (fp16, bf16) aligned.  The row's entries
// are added in CSR order, one at a time, in fp32; Tout = bf16 rounds each stored element once.
template <typename Tin, typename Tout, bool VEC4, class Src, class Epi>
__global__ __launch_bounds__(kAggNT) void k_agg_fwd(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                    int64_t T, const Tin* __restrict__ x, int64_t x_stride, int64_t F,
                                                    int lpr_log2, Tout* __restrict__ out, int64_t out_stride, Epi epi,
                                                    const int64_t* __restrict__ nid, int64_t x_rows) {
  static_assert(!Epi::kAct || (VEC4 && !std::is_same<Tin, __half>::value && std::is_same<Src, Dense>::value),
                "activation on load: dense fp32 / bf16 rows, vector form");
  constexpr bool kFp8 = std::is_same<Tin, fp8e4m3>::value;  // (then Epi is an Fp8<...> and carries the column exponents)
  static_assert(!kFp8 || !Epi::kAct, "fp8 rows are first-layer inputs: no activation on load");
  const Rows<Tin, Src> row{x, x_stride, nid, x_rows};
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kAggNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  const float inv = 1.0f / (float)(e > b ? e - b : 1);  // Mean
  const Tin* own = epi.s != 0.f ? row(t) : nullptr;      // Sum
  if (VEC4) {
    auto row4 = [&](int64_t j, int64_t c, const ColScale4<kFp8>& sc) {  // four columns of row j (activated on load with kAct)
      f4 v = load4(row(j) + c, sc);
      if constexpr (Epi::kAct) v = relu_dropout4(v, (j * x_stride + c) >> 2, epi.act);
      return v;
    };
    for (int64_t c = (int64_t)lane * 4; c < F; c += (int64_t)lpr * 4) {
      const ColScale4<kFp8> sc(epi, c);
      if (epi.concat_target) {  // [mean | x_target]: the target's own row (targets are the first rows of x), as fp32
        const f4 o = row4(t, c, sc);
        store4(out + t * out_stride + F + c, o);
      }
      f4 acc = {0.f, 0.f, 0.f, 0.f};
      int64_t k = b;
      for (; k + 1 < e; k += 2) {  // two independent rows in flight
        const f4 v0 = row4(col[k], c, sc), v1 = row4(col[k + 1], c, sc);
        acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
        acc.x += v1.x; acc.y += v1.y; acc.z += v1.z; acc.w += v1.w;
      }
      if (k < e) {
        const f4 v0 = row4(col[k], c, sc);
        acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
      }
      if (own) {
        const f4 o = load4(own + c, sc);
        acc = {fmaf(epi.s, o.x, acc.x), fmaf(epi.s, o.y, acc.y), fmaf(epi.s, o.z, acc.z), fmaf(epi.s, o.w, acc.w)};
      }
      if (!Epi::kSum) acc = {acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv};
      store4(out + t * out_stride + c, acc);
    }
  } else {
    for (int64_t c = lane; c < F; c += lpr) {
      const ColScale1<kFp8> sc(epi, c);
      if (epi.concat_target) {
        const float o = load1(row(t) + c, sc);
        store1(out + t * out_stride + F + c, o);
      }
      float acc = 0.f;
      for (int64_t k = b; k < e; ++k) acc += load1(row(col[k]) + c, sc);
      if (own) acc = fmaf(epi.s, load1(own + c, sc), acc);
      if (!Epi::kSum) acc *= inv;
      store1(out + t * out_stride + c, acc);
    }
  }
}

// the input gradient by scatter: grad_x[col[e],:] += w(t) * grad_out[t,:] for every edge (hardware fp32 atomics,
// summation order not fixed); Mean: w = 1 / deg(t) and empty rows are skipped, Sum: w = 1.  A bf16 grad_out is read
// exactly; grad_x stays an fp32 buffer (bf16 atomics would round every partial sum)
template <class Epi, typename Tg>
__global__ __launch_bounds__(kAggNT) void k_agg_bwd_scatter(const int64_t* __restrict__ rowptr,
                                                            const int64_t* __restrict__ col, int64_t T,
                                                            const Tg* __restrict__ grad_out, int64_t go_stride,
                                                            int64_t F, int lpr_log2, float* __restrict__ grad_x) {
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kAggNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  if (!Epi::kSum && e <= b) return;
  const float w = Epi::kSum ? 1.f : 1.0f / (float)(e - b);
  for (int64_t c = lane; c < F; c += lpr) {
    const float g = load1(grad_out + t * go_stride + c) * w;
    for (int64_t k = b; k < e; ++k) unsafeAtomicAdd(grad_x + col[k] * F + c, g);  // hardware fp32 atomic add
  }
}

// grad_x of the fused SAGE operand before the scatter of the mean's gradient: the first T source rows
// are the targets themselves and start from the gradient of the x_target half, the rest from zero
// (replaces a zero fill, the zero-padded gradient of the x[:T] slice and the add of the two).  grad_x is fp32.
template <typename Tg>
__global__ __launch_bounds__(kAggNT) void k_grad_init(const Tg* __restrict__ grad_out, int64_t go_stride, int64_t T,
                                                      int64_t S, int64_t F, float* __restrict__ grad_x) {
  const int64_t n4 = S * F / 4;  // F % 4 == 0 (checked by the caller)
  for (int64_t i = (int64_t)blockIdx.x * kAggNT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kAggNT) {
    const int64_t srow = (i * 4) / F, c = (i * 4) - srow * F;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (std::is_same<Tg, float>::value) {  // (the fp32 form's own addressing: it compiles tighter)
      if (srow < T) v = *reinterpret_cast<const float4*>(grad_out + srow * go_stride + F + c);
    } else {
      if (srow < T) v = ld4(grad_out + srow * go_stride + F + c, 0);
    }
    reinterpret_cast<float4*>(grad_x)[i] = v;
  }
}

// the same for the sum: rows < T start from s * grad_out (the self term), the others from zero; any F
template <typename Tg>
__global__ __launch_bounds__(kAggNT) void k_sum_grad_init(const Tg* __restrict__ g, int64_t go_stride, int64_t T,
                                                          int64_t S, int64_t F, float s, float* __restrict__ grad_x) {
  const int64_t n = S * F;
  for (int64_t i = (int64_t)blockIdx.x * kAggNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kAggNT) {
    const int64_t r = i / F, c = i - r * F;
    grad_x[i] = r < T ? s * load1(g + r * go_stride + c) : 0.f;
  }
}

// ---- ReLU + dropout in one pass (the stand-alone form; the SAGE stack applies them on load, see kAct) ----
// The backward pass needs no mask: y > 0 exactly where x > 0 and the element was kept.
__global__ __launch_bounds__(kAggNT) void k_relu_dropout_fwd(const float* __restrict__ x, int64_t n, uint32_t keep_thr,
                                                             float scale, uint64_t seed, int training,
                                                             float* __restrict__ y) {
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * kAggNT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kAggNT) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    float4 o;
    if (training) {
      const uint64_t r0 = mix64(seed + 2ull * (uint64_t)i * 0x9E3779B97F4A7C15ull);
      const uint64_t r1 = mix64(seed + (2ull * (uint64_t)i + 1ull) * 0x9E3779B97F4A7C15ull);
      o.x = (v.x > 0.f && (uint32_t)r0 < keep_thr) ? v.x * scale : 0.f;
      o.y = (v.y > 0.f && (uint32_t)(r0 >> 32) < keep_thr) ? v.y * scale : 0.f;
      o.z = (v.z > 0.f && (uint32_t)r1 < keep_thr) ? v.z * scale : 0.f;
      o.w = (v.w > 0.f && (uint32_t)(r1 >> 32) < keep_thr) ? v.w * scale : 0.f;
    } else {
      o = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
    }
    reinterpret_cast<float4*>(y)[i] = o;
  }
  // tail (n % 4 elements) by the first threads of block 0
  const int64_t t = n4 * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float v = x[t];
    const uint64_t r = mix64(seed + (uint64_t)t * 0xD1B54A32D192ED03ull);
    y[t] = training ? ((v > 0.f && (uint32_t)r < keep_thr) ? v * scale : 0.f) : fmaxf(v, 0.f);
  }
}

__global__ __launch_bounds__(kAggNT) void k_relu_dropout_bwd(const float* __restrict__ g, const float* __restrict__ y,
                                                             int64_t n, float scale, float* __restrict__ gx) {
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * kAggNT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kAggNT) {
    const float4 a = reinterpret_cast<const float4*>(g)[i], b = reinterpret_cast<const float4*>(y)[i];
    reinterpret_cast<float4*>(gx)[i] = make_float4(b.x > 0.f ? a.x * scale : 0.f, b.y > 0.f ? a.y * scale : 0.f,
                                                   b.z > 0.f ? a.z * scale : 0.f, b.w > 0.f ? a.w * scale : 0.f);
  }
  const int64_t t = n4 * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) gx[t] = y[t] > 0.f ? g[t] * scale : 0.f;
}

// the same backward from the PRE-activation z and the generator (no activated copy exists when the forward
// applied the activation on load): gx = g * scale where z > 0 and the element was kept.  g is the fp32 sum of a
// scatter; z fp32 or bf16; gx fp32 or bf16 (rounded once here).  !kAct: gx = g only (z not read; any n) -- the
// rounding pass of a bf16 scatter gradient without an activation.
template <typename Tz, typename Tout, bool kAct>
__global__ __launch_bounds__(kAggNT) void k_relu_dropout_bwd_pre(const float* __restrict__ g, const Tz* __restrict__ z,
                                                                 int64_t n, ActArgs act, Tout* __restrict__ gx) {
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * kAggNT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kAggNT) {
    const float4 a = ld4(g, i);
    if constexpr (kAct) {
      const float4 b = ld4(z, i);
      const f4 m = relu_dropout4(f4{b.x, b.y, b.z, b.w}, i, act);  // > 0 exactly where z > 0 and kept
      const float sc = act.training ? act.scale : 1.f;
      st4(gx, i, make_float4(m.x > 0.f ? a.x * sc : 0.f, m.y > 0.f ? a.y * sc : 0.f, m.z > 0.f ? a.z * sc : 0.f,
                             m.w > 0.f ? a.w * sc : 0.f));
    } else {
      st4(gx, i, a);
    }
  }
  if constexpr (!kAct) {
    const int64_t t = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && t < n) store1(gx + t, g[t]);
  }
}

// ---- backward of the fused operand by GATHER over the transposed hop: k_tr_count, k_tr_fill (transpose_hop.hip.h) ----
// the input gradient by GATHER over the targets t of source s (tcol[start[s] .. start[s+1])), two rows at a time:
//   Mean (SAGE's operand): (s < T ? grad_out[s, F:2F] : 0), added first, + sum_t grad_out[t, :F] * inv[t].  kAct: the
//     ReLU + dropout backward (k_relu_dropout_bwd_pre) of the pre-activation z (dense [S, F]) is applied to the row
//     before it is stored, instead of a separate read-modify-write pass over grad_x.
//   Sum: sum_t grad_out[t, :] (inv is not read), then fmaf(s, grad_out[s, :], acc) for s < T.
// grad_out (Tg) and z (Tz) fp32 or bf16, read exactly; fp32 sums; grad_x (Tout) fp32 or bf16, rounded once.
template <typename Tg, typename Tz, typename Tout, bool VEC4, class Epi>
__global__ __launch_bounds__(kAggNT) void k_agg_bwd_gather(const int32_t* __restrict__ start,
                                                           const int32_t* __restrict__ tcol,
                                                           const float* __restrict__ inv, int64_t T, int64_t S,
                                                           const Tg* __restrict__ g, int64_t go_stride, int64_t F,
                                                           int lpr_log2, Tout* __restrict__ grad_x,
                                                           const Tz* __restrict__ z, Epi epi) {
  static_assert(VEC4 || Epi::kSum, "the operand's gradient has the vector form only");
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t srow = ((int64_t)blockIdx.x * kAggNT + threadIdx.x) >> lpr_log2;
  if (srow >= S) return;
  const int32_t b = start[srow], e = start[srow + 1];
  if constexpr (VEC4) {
    auto w = [&](int32_t t) {  // the target's weight
      if constexpr (Epi::kSum) return 1.f;
      else return inv[t];
    };
    auto row4 = [&](int64_t t, int64_t c) { return ld4(g + t * go_stride + c, 0); };
    for (int64_t c = (int64_t)lane * 4; c < F; c += (int64_t)lpr * 4) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!Epi::kSum && srow < T) acc = row4(srow, F + c);
      int32_t k = b;
      for (; k + 1 < e; k += 2) {  // two independent rows in flight
        const int32_t t0 = tcol[k], t1 = tcol[k + 1];
        const float w0 = w(t0), w1 = w(t1);
        const float4 v0 = row4(t0, c), v1 = row4(t1, c);
        acc.x += v0.x * w0 + v1.x * w1; acc.y += v0.y * w0 + v1.y * w1;
        acc.z += v0.z * w0 + v1.z * w1; acc.w += v0.w * w0 + v1.w * w1;
      }
      if (k < e) {
        const int32_t t0 = tcol[k];
        const float w0 = w(t0);
        const float4 v0 = row4(t0, c);
        acc.x += v0.x * w0; acc.y += v0.y * w0; acc.z += v0.z * w0; acc.w += v0.w * w0;
      }
      if (Epi::kSum && srow < T) {
        const float4 o = row4(srow, c);
        acc = make_float4(fmaf(epi.s, o.x, acc.x), fmaf(epi.s, o.y, acc.y), fmaf(epi.s, o.z, acc.z), fmaf(epi.s, o.w, acc.w));
      }
      if constexpr (Epi::kAct) {
        const float4 zv = ld4(z + srow * F + c, 0);
        const f4 m = relu_dropout4(f4{zv.x, zv.y, zv.z, zv.w}, (srow * F + c) >> 2, epi.act);  // > 0: z > 0 and kept
        const float sc = epi.act.training ? epi.act.scale : 1.f;
        acc = make_float4(m.x > 0.f ? acc.x * sc : 0.f, m.y > 0.f ? acc.y * sc : 0.f, m.z > 0.f ? acc.z * sc : 0.f,
                          m.w > 0.f ? acc.w * sc : 0.f);
      }
      st4(grad_x + srow * F + c, 0, acc);
    }
  } else {  // Sum, any F: one column per lane and step
    for (int64_t c = lane; c < F; c += lpr) {
      float acc = 0.f;
      for (int32_t k = b; k < e; ++k) acc += load1(g + (int64_t)tcol[k] * go_stride + c);
      if (srow < T) acc = fmaf(epi.s, load1(g + srow * go_stride + c), acc);
      store1(grad_x + srow * F + c, acc);
    }
  }
}

// the fp16 flag of the entries that predate the element codes: any non-zero value means fp16
static int32_t half_elem(int32_t is_half) { return is_half ? SPP_ELEM_F16 : SPP_ELEM_F32; }

}  // namespace spp

using namespace spp;

// the grid of an element-wise kernel that strides over `items` work items
static unsigned elementwise_grid(int64_t items) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, kAggNT), 256 * 32));
}

// The forward of every mean / operand / sum entry (`who` names the public entry in the errors): validation, the
// choice of the vector form, the source x epilogue x element-type dispatch and the launch of k_agg_fwd.
//   source: DENSE (x = the batch's matrix), TABLE (x = the resident table, n_id = the batch's node ids, x_rows its rows)
//     or ROWS (n_id = the row addresses; x, x_stride unused)
//   vector form: F % 4 == 0 and every row aligned to 4 elements (row references: 8-byte aligned fp16 / bf16, 16-byte
//     aligned fp32 rows when F % 4 == 0, spp_mfg_out.row_addr); the activated operand and fp8 rows have no other form
//   fp8 rows (x_elem = SPP_ELEM_FP8_E4M3, spp_agg_forward_fp8 only): the same kernel with Tin = fp8e4m3 and the column
//     exponents fp8_scale_log2 in Fp8<Epi>; DENSE or TABLE, no activation on load
static spp_status agg_forward_desc(const char* who, const spp_agg_fwd_desc& d, const int8_t* fp8_scale_log2,
                                   void* stream) {
  const bool fp8 = d.x_elem == SPP_ELEM_FP8_E4M3, refs = d.source == SPP_AGG_ROWS;
  const bool act = d.epilogue == SPP_AGG_OPERAND_ACT, operand = act || d.epilogue == SPP_AGG_OPERAND;
  SPP_REQUIRE(d.source >= SPP_AGG_DENSE && d.source <= SPP_AGG_ROWS, "%s: unknown source %d", who, (int)d.source);
  SPP_REQUIRE(d.epilogue >= SPP_AGG_MEAN && d.epilogue <= SPP_AGG_SUM, "%s: unknown epilogue %d", who, (int)d.epilogue);
  SPP_REQUIRE((fp8 || elem_ok(d.x_elem)) && f32_bf16_ok(d.out_elem),
              "%s: unknown or unsupported element code (x %d, out %d)", who, (int)d.x_elem, (int)d.out_elem);
  SPP_REQUIRE(!fp8 || (!refs && !act), "%s: fp8 rows take dense rows or the table, and the mean, operand or sum epilogue",
              who);
  const int64_t T = d.num_targets, F = d.F;
  SPP_REQUIRE(T >= 0 && F >= 0, "%s: negative size", who);
  const int64_t width = operand ? 2 * F : F;
  const int64_t out_stride = d.out_stride_elems > 0 ? d.out_stride_elems : width;
  SPP_REQUIRE(out_stride >= width, "%s: output stride smaller than the output row", who);
  SPP_REQUIRE(!act || (d.p >= 0.f && d.p < 1.f), "%s: the activated operand needs 0 <= p < 1", who);
  if (T == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr_dev && d.out_dev && (!fp8 || fp8_scale_log2) &&
                  (refs ? d.n_id_dev != nullptr : d.x_dev && (d.source == SPP_AGG_DENSE || (d.n_id_dev && d.x_rows > 0))),
              "%s: NULL buffer or empty table", who);
  SPP_REQUIRE(refs || d.x_stride_elems >= F, "%s: row stride smaller than the row", who);
  const bool vec = F % 4 == 0 && out_stride % 4 == 0 && aligned_to(d.out_dev, 4 * elem_bytes(d.out_elem)) &&
                   (refs || (d.x_stride_elems % 4 == 0 && aligned_to(d.x_dev, 4 * elem_bytes(d.x_elem)))) &&
                   (!fp8 || aligned_to(fp8_scale_log2, 4));
  if (act)
    SPP_REQUIRE(d.source == SPP_AGG_DENSE && f32_bf16_ok(d.x_elem) && d.x_stride_elems == F && vec,
                "%s: the activated operand needs dense fp32 / bf16 rows, F %% 4 == 0 and aligned buffers", who);
  if (fp8)
    SPP_REQUIRE(vec, "%s: needs F %% 4 == 0, 4-byte aligned rows and exponents and an aligned output (F = %lld)", who,
                (long long)F);
  const int lpr_log2 = lanes_log2(vec ? F / 4 : F);
  const unsigned grid = (unsigned)ceil_div(T << lpr_log2, kAggNT);
  auto launch = [&](auto tin, auto tout, auto v, auto src, auto epi) {
    using Tin = typename decltype(tin)::type;
    using Tout = typename decltype(tout)::type;
    hipLaunchKernelGGL((k_agg_fwd<Tin, Tout, decltype(v)::value, decltype(src), decltype(epi)>), dim3(grid), dim3(kAggNT),
                       0, as_stream(stream), d.rowptr_dev, d.col_dev, T, static_cast<const Tin*>(d.x_dev),
                       d.x_stride_elems, F, lpr_log2, static_cast<Tout*>(d.out_dev), out_stride, epi, d.n_id_dev, d.x_rows);
  };
  auto by_type = [&](auto src, auto epi) {
    using Epi = decltype(epi);
    with_f32_bf16(d.out_elem, [&](auto tout) {
      if constexpr (Epi::kAct)
        with_f32_bf16(d.x_elem, [&](auto tin) { launch(tin, tout, std::true_type{}, src, epi); });
      else if (!fp8)
        with_elem_vec(d.x_elem, vec, [&](auto tin, auto v) { launch(tin, tout, v, src, epi); });
      else if constexpr (!std::is_same<decltype(src), Refs>::value)
        launch(Type<fp8e4m3>{}, tout, std::true_type{}, src, Fp8<Epi>{epi, fp8_scale_log2});
    });
  };
  auto by_epilogue = [&](auto src) {
    if (d.epilogue == SPP_AGG_SUM)
      by_type(src, Sum{d.self_scale});
    else if (!act)
      by_type(src, Mean<false>{operand ? 1 : 0, {}});
    else if constexpr (std::is_same<decltype(src), Dense>::value)
      by_type(src, Mean<true>{1, act_args(d.p, d.training, d.seed)});
  };
  d.source == SPP_AGG_TABLE ? by_epilogue(Table{}) : refs ? by_epilogue(Refs{}) : by_epilogue(Dense{});
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

template <class Epi, typename Tg>
static void launch_agg_bwd_scatter(const int64_t* rowptr, const int64_t* col, int64_t T, const Tg* grad_out,
                                   int64_t go_stride, int64_t F, float* grad_x, hipStream_t st) {
  const int lpr_log2 = lanes_log2(F);
  const unsigned grid = (unsigned)ceil_div(T << lpr_log2, kAggNT);
  hipLaunchKernelGGL((k_agg_bwd_scatter<Epi, Tg>), dim3(grid), dim3(kAggNT), 0, st, rowptr, col, T, grad_out, go_stride,
                     F, lpr_log2, grad_x);
}

// the bare scatter step of the mean's gradient: no num_sources, and it ADDS into a grad_x the caller zeroed
extern "C" spp_status spp_csr_mean_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                            const float* grad_out_dev, int64_t grad_out_stride_elems, int64_t F,
                                            float* grad_x_dev, void* stream) {
  SPP_REQUIRE(num_targets >= 0 && F >= 0, "spp_csr_mean_backward: negative size");
  if (num_targets == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(rowptr_dev && grad_out_dev && grad_x_dev, "spp_csr_mean_backward: NULL buffer");
  if (grad_out_stride_elems <= 0) grad_out_stride_elems = F;
  SPP_REQUIRE(grad_out_stride_elems >= F, "spp_csr_mean_backward: gradient stride smaller than the row");
  launch_agg_bwd_scatter<Mean<false>, float>(rowptr_dev, col_dev, num_targets, grad_out_dev, grad_out_stride_elems, F,
                                      grad_x_dev, as_stream(stream));
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// transpose_hop_bytes, TransposedHop and transpose_hop: transpose_hop.hip.h
extern "C" int64_t spp_sage_operand_backward_workspace_bytes(int64_t num_targets, int64_t num_sources,
                                                               int64_t num_edges) {
  return transpose_hop_bytes(num_targets, num_sources, num_edges, false);
}

// The backward of every operand / sum / mean entry but spp_csr_mean_backward (`who` names the public entry in the
// errors); grad_x [S, F] dense is written completely.
//   gather: the transposed hop in the workspace, then k_agg_bwd_gather (fixed summation order).  The operand's gradient
//     has the vector form only; the sum's takes any F and row stride.
//   scatter: fp32 atomics into an fp32 buffer (grad_x itself when it is fp32, else the workspace) that an init pass has
//     filled with the targets' own term, then one pass that applies the activation's backward and / or rounds to bf16.
// grad_out, z and grad_x are fp32 or bf16 (vector form: rows aligned to 4 elements); z is read by OPERAND_ACT only.
static spp_status agg_backward_desc(const char* who, const spp_agg_bwd_desc& d, void* workspace_dev,
                                    int64_t workspace_bytes, void* stream) {
  SPP_REQUIRE(d.form == SPP_AGG_SCATTER || d.form == SPP_AGG_GATHER, "%s: unknown form %d", who, (int)d.form);
  SPP_REQUIRE(d.epilogue >= SPP_AGG_MEAN && d.epilogue <= SPP_AGG_SUM, "%s: unknown epilogue %d", who, (int)d.epilogue);
  SPP_REQUIRE(f32_bf16_ok(d.grad_elem) && f32_bf16_ok(d.out_elem) && f32_bf16_ok(d.z_elem),
              "%s: unknown or unsupported element code (grad %d, out %d, z %d)", who, (int)d.grad_elem, (int)d.out_elem,
              (int)d.z_elem);
  const bool gather = d.form == SPP_AGG_GATHER, sum = d.epilogue == SPP_AGG_SUM;
  const bool act = d.epilogue == SPP_AGG_OPERAND_ACT, operand = act || d.epilogue == SPP_AGG_OPERAND;
  SPP_REQUIRE(!gather || operand || sum, "%s: the plain mean has the scatter form only", who);
  if (act)
    SPP_REQUIRE(d.z_dev && aligned_to(d.z_dev, 4 * elem_bytes(d.z_elem)) && d.p >= 0.f && d.p < 1.f,
                "%s: NULL / unaligned pre-activation or bad p", who);
  const int64_t T = d.num_targets, S = d.num_sources, E = d.num_edges, F = d.F;
  SPP_REQUIRE(T >= 0 && S >= T && F >= 0 && (!gather || E >= 0), "%s: bad sizes", who);
  if (S == 0 || F == 0) return SPP_OK;
  const int64_t n = S * F;
  SPP_REQUIRE(!gather || (S < (1ll << 31) && E < (1ll << 31)), "%s: 32-bit indices", who);
  SPP_REQUIRE(d.grad_x_dev && ((d.grad_out_dev && d.rowptr_dev) || T == 0) && (!gather || workspace_dev),
              "%s: NULL buffer", who);
  const int64_t width = operand ? 2 * F : F;
  const int64_t gs = d.grad_out_stride_elems > 0 ? d.grad_out_stride_elems : width;
  SPP_REQUIRE(gs >= width, "%s: gradient stride smaller than the row", who);
  const bool vec = F % 4 == 0 && gs % 4 == 0 && aligned_to(d.grad_out_dev, 4 * elem_bytes(d.grad_elem)) &&
                   aligned_to(d.grad_x_dev, 4 * elem_bytes(d.out_elem));
  SPP_REQUIRE(vec || !operand, "%s: the operand's gradient needs F %% 4 == 0 and rows aligned to 4 elements", who);
  const bool rounds = d.out_elem != SPP_ELEM_F32;  // scatter: the atomics' fp32 buffer is the workspace
  if (gather) {
    SPP_REQUIRE(aligned_to(workspace_dev, 16), "%s: unaligned workspace", who);
    SPP_REQUIRE(workspace_bytes >= transpose_hop_bytes(T, S, E, false), "%s: workspace too small", who);
  } else if (rounds) {
    SPP_REQUIRE(workspace_dev && aligned_to(workspace_dev, 16) && workspace_bytes >= 4 * n,
                "%s: a bf16 scatter gradient needs a 16-byte aligned fp32 workspace of 4 * S * F bytes", who);
  }
  hipStream_t st = as_stream(stream);
  const ActArgs aa = act ? act_args(d.p, d.training, d.seed) : ActArgs{};
  float* acc = static_cast<float*>(rounds ? workspace_dev : d.grad_x_dev);
  TransposedHop hop{};
  if (gather)
    SPP_TRY(transpose_hop(d.rowptr_dev, d.col_dev, T, S, E, false, workspace_dev, workspace_bytes, st, &hop));
  else if (d.epilogue == SPP_AGG_MEAN)
    SPP_HIP_TRY(hipMemsetAsync(acc, 0, 4 * (size_t)n, st));
  const int lpr_log2 = lanes_log2(vec ? F / 4 : F);
  const unsigned grid = (unsigned)ceil_div(S << lpr_log2, kAggNT);  // (gather)
  with_f32_bf16(d.grad_elem, [&](auto tg) {
    with_f32_bf16(d.out_elem, [&](auto tout) {
      using Tg = typename decltype(tg)::type;
      using Tout = typename decltype(tout)::type;
      const Tg* g = static_cast<const Tg*>(d.grad_out_dev);
      Tout* gx = static_cast<Tout*>(d.grad_x_dev);
      auto gather_rows = [&](auto v, auto tz, auto epi) {
        using Tz = typename decltype(tz)::type;
        hipLaunchKernelGGL((k_agg_bwd_gather<Tg, Tz, Tout, decltype(v)::value, decltype(epi)>), dim3(grid), dim3(kAggNT), 0,
                           st, hop.start, hop.tcol, hop.inv, T, S, g, gs, F, lpr_log2, gx,
                           static_cast<const Tz*>(act ? d.z_dev : nullptr), epi);
      };
      if (gather) {
        if (act)
          with_f32_bf16(d.z_elem, [&](auto tz) { gather_rows(std::true_type{}, tz, Mean<true>{1, aa}); });
        else if (operand)
          gather_rows(std::true_type{}, Type<float>{}, Mean<false>{1, {}});
        else if (vec)
          gather_rows(std::true_type{}, Type<float>{}, Sum{d.self_scale});
        else
          gather_rows(std::false_type{}, Type<float>{}, Sum{d.self_scale});
        return;
      }
      if (operand)
        hipLaunchKernelGGL(k_grad_init<Tg>, dim3(elementwise_grid(n / 4)), dim3(kAggNT), 0, st, g, gs, T, S, F, acc);
      else if (sum)
        hipLaunchKernelGGL(k_sum_grad_init<Tg>, dim3(elementwise_grid(n)), dim3(kAggNT), 0, st, g, gs, T, S, F,
                           d.self_scale, acc);
      if (T > 0)
        sum ? launch_agg_bwd_scatter<Sum>(d.rowptr_dev, d.col_dev, T, g, gs, F, acc, st)
            : launch_agg_bwd_scatter<Mean<false>>(d.rowptr_dev, d.col_dev, T, g, gs, F, acc, st);
      if (act)
        with_f32_bf16(d.z_elem, [&](auto tz) {
          using Tz = typename decltype(tz)::type;
          hipLaunchKernelGGL((k_relu_dropout_bwd_pre<Tz, Tout, true>), dim3(elementwise_grid(n / 4)), dim3(kAggNT), 0, st,
                             acc, static_cast<const Tz*>(d.z_dev), n, aa, gx);
        });
      else if (rounds)
        hipLaunchKernelGGL((k_relu_dropout_bwd_pre<float, Tout, false>), dim3(elementwise_grid(n / 4)), dim3(kAggNT), 0,
                           st, acc, (const float*)nullptr, n, ActArgs{}, gx);
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// ---- the entries that predate the descriptors: fixed-type spellings of agg_forward_desc / agg_backward_desc ----
// fp32 out / grad / z; x fp32 or fp16 by the old flag; each keeps only the restrictions the descriptor path lacks.
static spp_agg_fwd_desc fwd_desc(int32_t source, int32_t epilogue, const int64_t* rowptr_dev, const int64_t* col_dev,
                                 int64_t num_targets, const void* x_dev, int32_t x_is_half, int64_t x_stride_elems,
                                 int64_t x_rows, const int64_t* n_id_dev, int64_t F, float self_scale, float* out_dev,
                                 int64_t out_stride_elems) {
  spp_agg_fwd_desc d{};
  d.source = source, d.epilogue = epilogue, d.x_elem = half_elem(x_is_half), d.out_elem = SPP_ELEM_F32;
  d.rowptr_dev = rowptr_dev, d.col_dev = col_dev, d.num_targets = num_targets;
  d.x_dev = x_dev, d.x_stride_elems = x_stride_elems, d.x_rows = x_rows, d.n_id_dev = n_id_dev, d.F = F;
  d.out_dev = out_dev, d.out_stride_elems = out_stride_elems, d.self_scale = self_scale;
  return d;
}

static spp_agg_bwd_desc bwd_desc(int32_t form, int32_t epilogue, const int64_t* rowptr_dev, const int64_t* col_dev,
                                 int64_t num_targets, int64_t num_sources, int64_t num_edges, const float* grad_out_dev,
                                 int64_t grad_out_stride_elems, int64_t F, float self_scale, float* grad_x_dev) {
  spp_agg_bwd_desc d{};
  d.form = form, d.epilogue = epilogue, d.grad_elem = d.out_elem = d.z_elem = SPP_ELEM_F32;
  d.rowptr_dev = rowptr_dev, d.col_dev = col_dev;
  d.num_targets = num_targets, d.num_sources = num_sources, d.num_edges = num_edges;
  d.grad_out_dev = grad_out_dev, d.grad_out_stride_elems = grad_out_stride_elems, d.F = F;
  d.grad_x_dev = grad_x_dev, d.self_scale = self_scale;
  return d;
}

extern "C" spp_status spp_csr_mean_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                           const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t F,
                                           float* out_dev, int64_t out_stride_elems, void* stream) {
  return agg_forward_desc("spp_csr_mean_forward",
                          fwd_desc(SPP_AGG_DENSE, SPP_AGG_MEAN, rowptr_dev, col_dev, num_targets, x_dev, x_is_half,
                                   x_stride_elems, 0, nullptr, F, 0.f, out_dev, out_stride_elems),
                          nullptr, stream);
}

extern "C" spp_status spp_sage_operand_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                               const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t F,
                                               float* out_dev, int64_t out_stride_elems, void* stream) {
  SPP_REQUIRE(out_stride_elems >= 2 * F, "spp_sage_operand_forward: the operand [mean | x_target] needs 2F columns");
  return agg_forward_desc("spp_sage_operand_forward",
                          fwd_desc(SPP_AGG_DENSE, SPP_AGG_OPERAND, rowptr_dev, col_dev, num_targets, x_dev, x_is_half,
                                   x_stride_elems, 0, nullptr, F, 0.f, out_dev, out_stride_elems),
                          nullptr, stream);
}

extern "C" spp_status spp_sage_operand_forward_table(const int64_t* rowptr_dev, const int64_t* col_dev,
                                                     int64_t num_targets, const void* table_dev, int32_t table_is_half,
                                                     int64_t table_stride_elems, int64_t table_rows,
                                                     const int64_t* n_id_dev, int64_t F, float* out_dev,
                                                     int64_t out_stride_elems, void* stream) {
  SPP_REQUIRE(out_stride_elems >= 2 * F, "spp_sage_operand_forward_table: the operand [mean | x_target] needs 2F columns");
  SPP_REQUIRE(num_targets == 0 || (n_id_dev && table_dev && table_rows > 0),
              "spp_sage_operand_forward_table: needs the feature table and the batch's node ids");
  return agg_forward_desc("spp_sage_operand_forward_table",
                          fwd_desc(SPP_AGG_TABLE, SPP_AGG_OPERAND, rowptr_dev, col_dev, num_targets, table_dev,
                                   table_is_half, table_stride_elems, table_rows, n_id_dev, F, 0.f, out_dev,
                                   out_stride_elems),
                          nullptr, stream);
}

extern "C" spp_status spp_sage_operand_forward_rows(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                                    const int64_t* row_addr_dev, int32_t rows_are_half, int64_t F,
                                                    float* out_dev, int64_t out_stride_elems, void* stream) {
  SPP_REQUIRE(out_stride_elems >= 2 * F, "spp_sage_operand_forward_rows: the operand [mean | x_target] needs 2F columns");
  SPP_REQUIRE(F % 4 == 0 && aligned_to(out_dev, 16) && out_stride_elems % 4 == 0,
              "spp_sage_operand_forward_rows: needs F %% 4 == 0 and a 16-byte aligned operand (F = %lld)", (long long)F);
  return agg_forward_desc("spp_sage_operand_forward_rows",
                          fwd_desc(SPP_AGG_ROWS, SPP_AGG_OPERAND, rowptr_dev, col_dev, num_targets, nullptr,
                                   rows_are_half, 0, 0, row_addr_dev, F, 0.f, out_dev, out_stride_elems),
                          nullptr, stream);
}

// [mean | x_target] of relu_dropout(x) without materialising the activation (see kAct)
extern "C" spp_status spp_sage_operand_forward_act(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                                   const float* x_dev, int64_t F, float* out_dev, int64_t out_stride_elems,
                                                   float p, int32_t training, uint64_t seed, void* stream) {
  SPP_REQUIRE(out_stride_elems >= 2 * F, "spp_sage_operand_forward_act: the operand [mean | x_target] needs 2F columns");
  spp_agg_fwd_desc d = fwd_desc(SPP_AGG_DENSE, SPP_AGG_OPERAND_ACT, rowptr_dev, col_dev, num_targets, x_dev, 0, F, 0,
                                nullptr, F, 0.f, out_dev, out_stride_elems);
  d.p = p, d.training = training, d.seed = seed;
  return agg_forward_desc("spp_sage_operand_forward_act", d, nullptr, stream);
}

// (the operand's backward entries refuse a gradient stride of 0; the descriptor defaults it)
extern "C" spp_status spp_sage_operand_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                                int64_t num_sources, const float* grad_out_dev,
                                                int64_t grad_out_stride_elems, int64_t F, float* grad_x_dev,
                                                void* stream) {
  SPP_REQUIRE(grad_out_stride_elems >= 2 * F, "spp_sage_operand_backward: the operand's gradient needs 2F columns");
  return agg_backward_desc("spp_sage_operand_backward",
                           bwd_desc(SPP_AGG_SCATTER, SPP_AGG_OPERAND, rowptr_dev, col_dev, num_targets, num_sources, 0,
                                    grad_out_dev, grad_out_stride_elems, F, 0.f, grad_x_dev),
                           nullptr, 0, stream);
}

extern "C" spp_status spp_sage_operand_backward_gather(const int64_t* rowptr_dev, const int64_t* col_dev,
                                                       int64_t num_targets, int64_t num_sources, int64_t num_edges,
                                                       const float* grad_out_dev, int64_t grad_out_stride_elems,
                                                       int64_t F, float* grad_x_dev, void* workspace_dev,
                                                       int64_t workspace_bytes, void* stream) {
  SPP_REQUIRE(grad_out_stride_elems >= 2 * F, "spp_sage_operand_backward_gather: the operand's gradient needs 2F columns");
  return agg_backward_desc("spp_sage_operand_backward_gather",
                           bwd_desc(SPP_AGG_GATHER, SPP_AGG_OPERAND, rowptr_dev, col_dev, num_targets, num_sources,
                                    num_edges, grad_out_dev, grad_out_stride_elems, F, 0.f, grad_x_dev),
                           workspace_dev, workspace_bytes, stream);
}

// the same, followed in the same pass by the ReLU + dropout backward of spp_relu_dropout_backward_pre: grad_x
// becomes the gradient w.r.t. the PRE-activation z_pre_dev (dense fp32 [S, F]) of the rows the forward activated on load
extern "C" spp_status spp_sage_operand_backward_gather_act(const int64_t* rowptr_dev, const int64_t* col_dev,
                                                           int64_t num_targets, int64_t num_sources, int64_t num_edges,
                                                           const float* grad_out_dev, int64_t grad_out_stride_elems,
                                                           int64_t F, float* grad_x_dev, void* workspace_dev,
                                                           int64_t workspace_bytes, const float* z_pre_dev, float p,
                                                           int32_t training, uint64_t seed, void* stream) {
  SPP_REQUIRE(grad_out_stride_elems >= 2 * F,
              "spp_sage_operand_backward_gather_act: the operand's gradient needs 2F columns");
  spp_agg_bwd_desc d = bwd_desc(SPP_AGG_GATHER, SPP_AGG_OPERAND_ACT, rowptr_dev, col_dev, num_targets, num_sources,
                                num_edges, grad_out_dev, grad_out_stride_elems, F, 0.f, grad_x_dev);
  d.z_dev = z_pre_dev, d.p = p, d.training = training, d.seed = seed;
  return agg_backward_desc("spp_sage_operand_backward_gather_act", d, workspace_dev, workspace_bytes, stream);
}

// ---- ReLU + dropout, element-wise (the stand-alone forms) ----
extern "C" spp_status spp_relu_dropout_forward(const float* x_dev, int64_t n, float p, int32_t training, uint64_t seed,
                                               float* y_dev, void* stream) {
  SPP_REQUIRE(n >= 0 && p >= 0.f && p < 1.f, "spp_relu_dropout_forward: bad arguments");
  if (n == 0) return SPP_OK;
  SPP_REQUIRE(x_dev && y_dev && aligned_to(x_dev, 16) && aligned_to(y_dev, 16),
              "spp_relu_dropout_forward: NULL or unaligned buffer");
  const ActArgs a = act_args(p, training, seed);
  hipLaunchKernelGGL(k_relu_dropout_fwd, dim3(elementwise_grid(n / 4)), dim3(kAggNT), 0, as_stream(stream), x_dev, n,
                     a.keep_thr, a.scale, seed, training, y_dev);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_relu_dropout_backward(const float* grad_dev, const float* y_dev, int64_t n, float scale,
                                                float* grad_x_dev, void* stream) {
  SPP_REQUIRE(n >= 0, "spp_relu_dropout_backward: negative size");
  if (n == 0) return SPP_OK;
  SPP_REQUIRE(grad_dev && y_dev && grad_x_dev, "spp_relu_dropout_backward: NULL buffer");
  SPP_REQUIRE(aligned_to(grad_dev, 16) && aligned_to(y_dev, 16) && aligned_to(grad_x_dev, 16),
              "spp_relu_dropout_backward: unaligned buffer");
  hipLaunchKernelGGL(k_relu_dropout_bwd, dim3(elementwise_grid(n / 4)), dim3(kAggNT), 0, as_stream(stream), grad_dev,
                     y_dev, n, scale, grad_x_dev);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_relu_dropout_backward_pre(const float* grad_dev, const float* z_dev, int64_t n, float p,
                                                    int32_t training, uint64_t seed, float* grad_x_dev, void* stream) {
  SPP_REQUIRE(n >= 0 && p >= 0.f && p < 1.f, "spp_relu_dropout_backward_pre: bad arguments");
  if (n == 0) return SPP_OK;
  SPP_REQUIRE(grad_dev && z_dev && grad_x_dev && n % 4 == 0 && aligned_to(grad_dev, 16) && aligned_to(z_dev, 16) &&
                  aligned_to(grad_x_dev, 16),
              "spp_relu_dropout_backward_pre: needs n %% 4 == 0 and 16-byte aligned buffers");
  hipLaunchKernelGGL((k_relu_dropout_bwd_pre<float, float, true>), dim3(elementwise_grid(n / 4)), dim3(kAggNT), 0,
                     as_stream(stream), grad_dev, z_dev, n, act_args(p, training, seed), grad_x_dev);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// ================================================================================================
// GINConv sum aggregation over an MFG hop (reference: driver/models.py:234-283 uses
// torch_geometric.nn.GINConv(nn, eps=0, train_eps=False), aggr='add', on ((x, x_target), adj_t)):
//     out[t,:]    = s * x[t,:] + sum_{e in row t} x[col[e],:]                    s = 1 + eps   forward
//     grad_x[j,:] = (j < T ? s * grad_out[j,:] : 0) + sum_{e: col[e] = j} grad_out[row e,:]    backward
// Every entry of the row counts (duplicates and self edges included); targets are the first T rows of x.
// The mean's kernels and row sources with the Sum epilogue; the same transposed hop for the gather backward.
// ================================================================================================
extern "C" spp_status spp_csr_sum_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                          const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t F,
                                          float self_scale, float* out_dev, int64_t out_stride_elems, void* stream) {
  return agg_forward_desc("spp_csr_sum_forward",
                          fwd_desc(SPP_AGG_DENSE, SPP_AGG_SUM, rowptr_dev, col_dev, num_targets, x_dev, x_is_half,
                                   x_stride_elems, 0, nullptr, F, self_scale, out_dev, out_stride_elems),
                          nullptr, stream);
}

extern "C" spp_status spp_csr_sum_forward_table(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                                const void* table_dev, int32_t table_is_half, int64_t table_stride_elems,
                                                int64_t table_rows, const int64_t* n_id_dev, int64_t F, float self_scale,
                                                float* out_dev, int64_t out_stride_elems, void* stream) {
  SPP_REQUIRE(num_targets == 0 || (n_id_dev && table_dev && table_rows > 0),
              "spp_csr_sum_forward_table: needs the feature table and the batch's node ids");
  return agg_forward_desc("spp_csr_sum_forward_table",
                          fwd_desc(SPP_AGG_TABLE, SPP_AGG_SUM, rowptr_dev, col_dev, num_targets, table_dev, table_is_half,
                                   table_stride_elems, table_rows, n_id_dev, F, self_scale, out_dev, out_stride_elems),
                          nullptr, stream);
}

extern "C" spp_status spp_csr_sum_forward_rows(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                               const int64_t* row_addr_dev, int32_t rows_are_half, int64_t F,
                                               float self_scale, float* out_dev, int64_t out_stride_elems, void* stream) {
  return agg_forward_desc("spp_csr_sum_forward_rows",
                          fwd_desc(SPP_AGG_ROWS, SPP_AGG_SUM, rowptr_dev, col_dev, num_targets, nullptr, rows_are_half, 0,
                                   0, row_addr_dev, F, self_scale, out_dev, out_stride_elems),
                          nullptr, stream);
}

extern "C" spp_status spp_csr_sum_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                           int64_t num_sources, const float* grad_out_dev, int64_t grad_out_stride_elems,
                                           int64_t F, float self_scale, float* grad_x_dev, void* stream) {
  return agg_backward_desc("spp_csr_sum_backward",
                           bwd_desc(SPP_AGG_SCATTER, SPP_AGG_SUM, rowptr_dev, col_dev, num_targets, num_sources, 0,
                                    grad_out_dev, grad_out_stride_elems, F, self_scale, grad_x_dev),
                           nullptr, 0, stream);
}

extern "C" spp_status spp_csr_sum_backward_gather(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                                  int64_t num_sources, int64_t num_edges, const float* grad_out_dev,
                                                  int64_t grad_out_stride_elems, int64_t F, float self_scale,
                                                  float* grad_x_dev, void* workspace_dev, int64_t workspace_bytes,
                                                  void* stream) {
  return agg_backward_desc("spp_csr_sum_backward_gather",
                           bwd_desc(SPP_AGG_GATHER, SPP_AGG_SUM, rowptr_dev, col_dev, num_targets, num_sources, num_edges,
                                    grad_out_dev, grad_out_stride_elems, F, self_scale, grad_x_dev),
                           workspace_dev, workspace_bytes, stream);
}

// ================================================================================================
// Aggregation by descriptor (include/spp.h: spp_agg_fwd_desc, spp_agg_bwd_desc): agg_forward_desc / agg_backward_desc
// with the element types chosen per call -- fp32 / fp16 / bf16 (or, through its own entry, fp8) rows in, fp32 / bf16
// out -- for bf16 autocast training.
// ================================================================================================
extern "C" spp_status spp_agg_forward(const spp_agg_fwd_desc* desc, void* stream) {
  SPP_REQUIRE(desc, "spp_agg_forward: NULL descriptor");
  SPP_REQUIRE(desc->x_elem != SPP_ELEM_FP8_E4M3, "spp_agg_forward: unsupported element code (x %d): fp8 rows and their "
              "column exponents go through spp_agg_forward_fp8", (int)desc->x_elem);
  return agg_forward_desc("spp_agg_forward", *desc, nullptr, stream);
}

// spp_agg_forward over an fp8 table (f3c)
extern "C" spp_status spp_agg_forward_fp8(const spp_agg_fwd_desc* desc, const int8_t* scale_log2_dev, void* stream) {
  SPP_REQUIRE(desc, "spp_agg_forward_fp8: NULL descriptor");
  SPP_REQUIRE(desc->x_elem == SPP_ELEM_FP8_E4M3, "spp_agg_forward_fp8: x_elem must be SPP_ELEM_FP8_E4M3, got %d",
              (int)desc->x_elem);
  return agg_forward_desc("spp_agg_forward_fp8", *desc, scale_log2_dev, stream);
}

extern "C" spp_status spp_agg_backward(const spp_agg_bwd_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                       void* stream) {
  SPP_REQUIRE(desc, "spp_agg_backward: NULL descriptor");
  return agg_backward_desc("spp_agg_backward", *desc, workspace_dev, workspace_bytes, stream);
}
