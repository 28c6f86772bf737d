// f3r: edge-weighted sum aggregation over an MFG hop's CSR -- the message passing of GCNConv, and of any layer whose
// adjacency carries one fp32 value per entry:
//     out[t,:]      = sum_{k in row t} w[k] * x[col[k],:]  (+ self_w[t] * x[t,:], last)                  forward
//     grad_x[s,:]   = sum_{k = (t, s)} w[k] * g[t,:]       (+ self_w[s] * g[s,:] for s < T)              backward
//     grad_w[k]     = <g[t,:], x[col[k],:]>,  grad_self_w[t] = <g[t,:], x[t,:]>                          weight gradient
//     coef, self_coef = PyG's gcn_norm of the hop padded to [S, S]                                         spp_gcn_norm
// The forward is k_agg_fwd's gather-reduce (aggregate.hip) with an fmaf in place of the addition: the same lanes, the same
// loads (agg_rows.hip.h), deg * F * s bytes of rows per target plus 4 bytes of weight per entry.  The backward is the
// same gather over the transposed hop with edge ids (transpose_hop.hip.h): no atomic touches an accumulator.
#include "agg_rows.hip.h"
#include "elem_io.hip.h"
#include "transpose_hop.hip.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace spp {
namespace agg_w {

constexpr int kNT = 256;

// LPR lanes share a target row; VEC4: F % 4 == 0 and rows and outputs aligned to 4 elements.  One fmaf per entry and
// column, applied in CSR order to an accumulator that starts at 0, the self term last: a row's result depends on the
// row alone, not on how the loop pairs its entries.  Tout = bf16 rounds each stored element once.
template <typename Tin, typename Tout, bool VEC4, class Src>
__global__ __launch_bounds__(kNT) void k_agg_w_fwd(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                   const float* __restrict__ w, const float* __restrict__ self_w,
                                                   int64_t T, const Tin* __restrict__ x, int64_t x_stride, int64_t F,
                                                   int lpr_log2, Tout* __restrict__ out, int64_t out_stride,
                                                   const int64_t* __restrict__ nid, int64_t x_rows) {
  using P = Piece<VEC4>;
  const Rows<Tin, Src> row{x, x_stride, nid, x_rows};
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  for (int64_t c = (int64_t)lane * P::kWidth; c < F; c += (int64_t)lpr * P::kWidth) {
    auto acc = P::zero();
    int64_t k = b;
    for (; k + 1 < e; k += 2) {  // two independent rows in flight: both loads, then both fmafs
      const int64_t j0 = col[k], j1 = col[k + 1];
      const float w0 = w[k], w1 = w[k + 1];
      const auto v0 = P::load(row(j0) + c), v1 = P::load(row(j1) + c);
      acc = P::fma(w0, v0, acc);
      acc = P::fma(w1, v1, acc);
    }
    if (k < e) acc = P::fma(w[k], P::load(row(col[k]) + c), acc);
    if (self_w) acc = P::fma(self_w[t], P::load(row(t) + c), acc);
    P::store(out + t * out_stride + c, acc);
  }
}

// the input gradient by GATHER over the entries (t, s) of source s: tcol names the row of g, tedge the weight.  g (Tg)
// fp32 or bf16, read exactly; fp32 fmaf chain in the segment's order, the self term last; grad_x (Tout) rounded once.
template <typename Tg, typename Tout, bool VEC4>
__global__ __launch_bounds__(kNT) void k_agg_w_bwd(const int32_t* __restrict__ start, const int32_t* __restrict__ tcol,
                                                   const int32_t* __restrict__ tedge, const float* __restrict__ w,
                                                   const float* __restrict__ self_w, int64_t T, int64_t S,
                                                   const Tg* __restrict__ g, int64_t go_stride, int64_t F, int lpr_log2,
                                                   Tout* __restrict__ grad_x) {
  using P = Piece<VEC4>;
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t srow = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> lpr_log2;
  if (srow >= S) return;
  const int32_t b = start[srow], e = start[srow + 1];
  for (int64_t c = (int64_t)lane * P::kWidth; c < F; c += (int64_t)lpr * P::kWidth) {
    auto acc = P::zero();
    int32_t k = b;
    for (; k + 1 < e; k += 2) {
      const int64_t t0 = tcol[k], t1 = tcol[k + 1];
      const float w0 = w[tedge[k]], w1 = w[tedge[k + 1]];
      const auto v0 = P::load(g + t0 * go_stride + c), v1 = P::load(g + t1 * go_stride + c);
      acc = P::fma(w0, v0, acc);
      acc = P::fma(w1, v1, acc);
    }
    if (k < e) acc = P::fma(w[tedge[k]], P::load(g + (int64_t)tcol[k] * go_stride + c), acc);
    if (self_w && srow < T) acc = P::fma(self_w[srow], P::load(g + srow * go_stride + c), acc);
    P::store(grad_x + srow * F + c, acc);
  }
}

__device__ __forceinline__ float dot_add(f4 a, f4 v, float s) {
  return fmaf(a.w, v.w, fmaf(a.z, v.z, fmaf(a.y, v.y, fmaf(a.x, v.x, s))));
}
__device__ __forceinline__ float dot_add(float a, float v, float s) { return fmaf(a, v, s); }

// the sum of v over the lpr lanes that share a row: a butterfly of fixed shape, every lane ends with the same bits
__device__ __forceinline__ float group_sum(float v, int lpr) {
  for (int m = lpr >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// The weights' gradient, one dot product per entry.  The lpr lanes of target t hold their columns of g[t,:] in registers
// (kWgradSteps column steps at a time; a wider row takes another round, whose sums the storing lane adds to what it
// stored in the round before) while they walk the row's entries; each lane's products accumulate in fp32 in column
// order, the group reduces by group_sum and lane 0 stores.  No atomics, no LDS; a result depends on its row alone.
constexpr int kWgradSteps = 4;
template <typename Tin, typename Tg, bool VEC4, class Src>
__global__ __launch_bounds__(kNT) void k_agg_w_wgrad(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                     int64_t T, const Tin* __restrict__ x, int64_t x_stride, int64_t F,
                                                     int lpr_log2, const Tg* __restrict__ g, int64_t go_stride,
                                                     float* __restrict__ grad_w, float* __restrict__ grad_self_w,
                                                     const int64_t* __restrict__ nid, int64_t x_rows) {
  using P = Piece<VEC4>;
  const Rows<Tin, Src> row{x, x_stride, nid, x_rows};
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  const int64_t step = (int64_t)lpr * P::kWidth;
  for (int64_t c0 = (int64_t)lane * P::kWidth, base = 0; base < F; c0 += step * kWgradSteps, base += step * kWgradSteps) {
    typename P::type gr[kWgradSteps];
#pragma unroll
    for (int i = 0; i < kWgradSteps; ++i) gr[i] = c0 + i * step < F ? P::load(g + t * go_stride + c0 + i * step) : P::zero();
    auto dot = [&](const Tin* r) {  // this lane's share of <g[t, round], r[round]>
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < kWgradSteps; ++i)
        if (c0 + i * step < F) s = dot_add(gr[i], P::load(r + c0 + i * step), s);
      return s;
    };
    int64_t k = b;
    for (; k + 1 < e; k += 2) {  // two independent rows in flight
      const Tin *r0 = row(col[k]), *r1 = row(col[k + 1]);
      float s0 = dot(r0), s1 = dot(r1);
      s0 = group_sum(s0, lpr);
      s1 = group_sum(s1, lpr);
      if (lane == 0) {
        grad_w[k] = base == 0 ? s0 : grad_w[k] + s0;
        grad_w[k + 1] = base == 0 ? s1 : grad_w[k + 1] + s1;
      }
    }
    if (k < e) {
      const float s0 = group_sum(dot(row(col[k])), lpr);
      if (lane == 0) grad_w[k] = base == 0 ? s0 : grad_w[k] + s0;
    }
    if (grad_self_w) {
      const float s0 = group_sum(dot(row(t)), lpr);
      if (lane == 0) grad_self_w[t] = base == 0 ? s0 : grad_self_w[t] + s0;
    }
  }
}

// gcn_norm, pass 1: dinv[t] = (fill + the row's weight sum, CSR order)^-1/2, 0 where that is inf
__global__ __launch_bounds__(kNT) void k_gcn_dinv(const int64_t* __restrict__ rowptr, const float* __restrict__ w, int64_t T,
                                                  float fill, float* __restrict__ dinv) {
  const int64_t t = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  float s = 0.f;
  if (w)
    for (int64_t k = b; k < e; ++k) s += w[k];
  else
    s = (float)(e - b);
  const float d = 1.0f / sqrtf(fill + s);
  dinv[t] = isinf(d) ? 0.f : d;
}

// pass 2: coef[k] = dinv[t] * w[k] * dinv[col[k]] (a source that is no target has degree fill: fill_dinv, no read),
// self_coef[t] = fill * dinv[t]^2
__global__ __launch_bounds__(kNT) void k_gcn_coef(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                  const float* __restrict__ w, int64_t T, float fill, float fill_dinv,
                                                  const float* __restrict__ dinv, float* __restrict__ coef,
                                                  float* __restrict__ self_coef) {
  const int64_t t = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  const float dt = dinv[t];
  for (int64_t k = b; k < e; ++k) {
    const int64_t s = col[k];
    const float ds = (uint64_t)s < (uint64_t)T ? dinv[s] : fill_dinv;
    coef[k] = dt * (w ? w[k] : 1.f) * ds;
  }
  if (self_coef) self_coef[t] = dt * fill * dt;
}

constexpr int64_t kMaxElems = (int64_t)1 << 62;
constexpr int64_t kMaxIndex = (int64_t)1 << 31;

// what the forward and the weight gradient check alike: the sizes and the row source
struct RowsIn {
  int32_t source, x_elem;
  const int64_t *rowptr, *col;
  int64_t T, E;
  const void* x;
  int64_t x_stride, x_rows;
  const int64_t* nid;
  int64_t F;
};

static spp_status check_codes(const char* who, const RowsIn& r) {
  SPP_REQUIRE(r.source >= SPP_AGG_DENSE && r.source <= SPP_AGG_ROWS, "%s: unknown source %d", who, (int)r.source);
  SPP_REQUIRE(r.x_elem != SPP_ELEM_FP8_E4M3, "%s: fp8 rows are not supported (fp32, fp16 or bf16 rows)", who);
  SPP_REQUIRE(elem_ok(r.x_elem), "%s: unknown or unsupported element code (x %d)", who, (int)r.x_elem);
  SPP_REQUIRE(r.T >= 0 && r.F >= 0 && r.E >= 0, "%s: negative size (T %lld, F %lld, E %lld)", who, (long long)r.T,
              (long long)r.F, (long long)r.E);
  SPP_REQUIRE(r.F == 0 || r.T < kMaxElems / (2 * r.F), "%s: T * F out of range", who);
  return SPP_OK;
}

static spp_status check_rows(const char* who, const RowsIn& r) {
  const bool refs = r.source == SPP_AGG_ROWS;
  SPP_REQUIRE(r.rowptr && (r.col || r.E == 0) &&
                  (refs ? r.nid != nullptr : r.x && (r.source == SPP_AGG_DENSE || (r.nid && r.x_rows > 0))),
              "%s: NULL buffer or empty table", who);
  SPP_REQUIRE(refs || r.x_stride >= r.F, "%s: row stride smaller than the row", who);
  SPP_REQUIRE(refs || aligned_to(r.x, elem_bytes(r.x_elem)), "%s: misaligned buffer (x is not aligned to its element)", who);
  return SPP_OK;
}

static bool rows_vec(const RowsIn& r) {
  return r.F % 4 == 0 && (r.source == SPP_AGG_ROWS || (r.x_stride % 4 == 0 && aligned_to(r.x, 4 * elem_bytes(r.x_elem))));
}

template <class Fn>
static void with_source(int32_t source, Fn&& fn) {
  source == SPP_AGG_TABLE ? fn(Table{}) : source == SPP_AGG_ROWS ? fn(Refs{}) : fn(Dense{});
}

}  // namespace agg_w
}  // namespace spp

using namespace spp;
using namespace spp::agg_w;

extern "C" spp_status spp_agg_weighted_forward(const spp_agg_weighted_fwd_desc* desc, void* stream) {
  const char* who = "spp_agg_weighted_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_agg_weighted_fwd_desc& d = *desc;
  const RowsIn r{d.source, d.x_elem, d.rowptr_dev, d.col_dev, d.num_targets, d.num_edges, d.x_dev, d.x_stride_elems,
                 d.x_rows, d.n_id_dev, d.F};
  SPP_TRY(check_codes(who, r));
  SPP_REQUIRE(f32_bf16_ok(d.out_elem), "%s: unknown or unsupported element code (out %d; the output is fp32 or bf16)", who,
              (int)d.out_elem);
  const int64_t T = d.num_targets, F = d.F;
  SPP_REQUIRE(d.out_stride_elems >= 0 && (d.out_stride_elems == 0 || d.out_stride_elems >= F),
              "%s: output stride smaller than the output row", who);
  const int64_t out_stride = d.out_stride_elems > 0 ? d.out_stride_elems : F;
  if (T == 0 || F == 0) return SPP_OK;
  SPP_TRY(check_rows(who, r));
  SPP_REQUIRE(d.out_dev && (d.w_dev || d.num_edges == 0), "%s: NULL buffer (out or w)", who);
  SPP_REQUIRE(aligned_to(d.out_dev, elem_bytes(d.out_elem)) && aligned_to(d.w_dev, 4) && aligned_to(d.self_w_dev, 4),
              "%s: misaligned buffer (out, w or self_w is not aligned to its element)", who);
  const bool vec = rows_vec(r) && out_stride % 4 == 0 && aligned_to(d.out_dev, 4 * elem_bytes(d.out_elem));
  const int lpr_log2 = lanes_log2(vec ? F / 4 : F);
  const unsigned grid = (unsigned)ceil_div(T << lpr_log2, kNT);
  with_source(d.source, [&](auto src) {
    with_in_out_vec(d.x_elem, d.out_elem, vec, [&](auto tin, auto tout, auto v) {
      using Tin = typename decltype(tin)::type;
      using Tout = typename decltype(tout)::type;
      hipLaunchKernelGGL((k_agg_w_fwd<Tin, Tout, decltype(v)::value, decltype(src)>), dim3(grid), dim3(kNT), 0,
                         as_stream(stream), d.rowptr_dev, d.col_dev, d.w_dev, d.self_w_dev, T,
                         static_cast<const Tin*>(d.x_dev), d.x_stride_elems, F, lpr_log2, static_cast<Tout*>(d.out_dev),
                         out_stride, d.n_id_dev, d.x_rows);
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" int64_t spp_agg_weighted_backward_workspace_bytes(int64_t num_targets, int64_t num_sources, int64_t num_edges) {
  if (num_targets < 0 || num_sources < num_targets || num_edges < 0 || num_sources >= kMaxIndex || num_edges >= kMaxIndex)
    return -1;
  return transpose_hop_bytes(num_targets, num_sources, num_edges, true);
}

extern "C" spp_status spp_agg_weighted_backward(const spp_agg_weighted_bwd_desc* desc, void* workspace_dev,
                                                int64_t workspace_bytes, void* stream) {
  const char* who = "spp_agg_weighted_backward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_agg_weighted_bwd_desc& d = *desc;
  SPP_REQUIRE(f32_bf16_ok(d.grad_elem) && f32_bf16_ok(d.out_elem),
              "%s: unknown or unsupported element code (grad %d, out %d; fp32 or bf16)", who, (int)d.grad_elem,
              (int)d.out_elem);
  const int64_t T = d.num_targets, S = d.num_sources, E = d.num_edges, F = d.F;
  SPP_REQUIRE(T >= 0 && S >= T && F >= 0 && E >= 0, "%s: bad sizes (T %lld, S %lld, E %lld, F %lld)", who, (long long)T,
              (long long)S, (long long)E, (long long)F);
  SPP_REQUIRE(S < kMaxIndex && E < kMaxIndex, "%s: S or E beyond 2^31 (the transposed hop has 32-bit indices)", who);
  SPP_REQUIRE(F == 0 || S < kMaxElems / (2 * F), "%s: S * F out of range", who);
  SPP_REQUIRE(d.grad_out_stride_elems >= 0 && (d.grad_out_stride_elems == 0 || d.grad_out_stride_elems >= F),
              "%s: gradient stride smaller than the row", who);
  const int64_t gs = d.grad_out_stride_elems > 0 ? d.grad_out_stride_elems : F;
  if (S == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(d.grad_x_dev && ((d.grad_out_dev && d.rowptr_dev) || T == 0) && ((d.col_dev && d.w_dev) || E == 0),
              "%s: NULL buffer", who);
  SPP_REQUIRE(aligned_to(d.grad_x_dev, elem_bytes(d.out_elem)) && aligned_to(d.grad_out_dev, elem_bytes(d.grad_elem)) &&
                  aligned_to(d.w_dev, 4) && aligned_to(d.self_w_dev, 4),
              "%s: misaligned buffer (grad_x, grad_out, w or self_w is not aligned to its element)", who);
  SPP_REQUIRE(workspace_dev && aligned_to(workspace_dev, 16) && workspace_bytes >= transpose_hop_bytes(T, S, E, true),
              "%s: missing, misaligned or too small workspace (spp_agg_weighted_backward_workspace_bytes, 16-byte aligned)",
              who);
  hipStream_t st = as_stream(stream);
  TransposedHop hop{};
  SPP_TRY(transpose_hop(d.rowptr_dev, d.col_dev, T, S, E, true, workspace_dev, workspace_bytes, st, &hop));
  const bool vec = F % 4 == 0 && gs % 4 == 0 && aligned_to(d.grad_out_dev, 4 * elem_bytes(d.grad_elem)) &&
                   aligned_to(d.grad_x_dev, 4 * elem_bytes(d.out_elem));
  const int lpr_log2 = lanes_log2(vec ? F / 4 : F);
  const unsigned grid = (unsigned)ceil_div(S << lpr_log2, kNT);
  auto by_vec = [&](auto v) {
    with_f32_bf16(d.grad_elem, [&](auto tg) {
      with_f32_bf16(d.out_elem, [&](auto tout) {
        using Tg = typename decltype(tg)::type;
        using Tout = typename decltype(tout)::type;
        hipLaunchKernelGGL((k_agg_w_bwd<Tg, Tout, decltype(v)::value>), dim3(grid), dim3(kNT), 0, st, hop.start, hop.tcol,
                           hop.tedge, d.w_dev, d.self_w_dev, T, S, static_cast<const Tg*>(d.grad_out_dev), gs, F,
                           lpr_log2, static_cast<Tout*>(d.grad_x_dev));
      });
    });
  };
  vec ? by_vec(std::true_type{}) : by_vec(std::false_type{});
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_agg_weighted_wgrad(const spp_agg_weighted_wgrad_desc* desc, void* stream) {
  const char* who = "spp_agg_weighted_wgrad";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_agg_weighted_wgrad_desc& d = *desc;
  const RowsIn r{d.source, d.x_elem, d.rowptr_dev, d.col_dev, d.num_targets, d.num_edges, d.x_dev, d.x_stride_elems,
                 d.x_rows, d.n_id_dev, d.F};
  SPP_TRY(check_codes(who, r));
  SPP_REQUIRE(f32_bf16_ok(d.grad_elem), "%s: unknown or unsupported element code (grad %d; fp32 or bf16)", who,
              (int)d.grad_elem);
  const int64_t T = d.num_targets, F = d.F;
  SPP_REQUIRE(d.grad_out_stride_elems >= 0 && (d.grad_out_stride_elems == 0 || d.grad_out_stride_elems >= F),
              "%s: gradient stride smaller than the row", who);
  const int64_t gs = d.grad_out_stride_elems > 0 ? d.grad_out_stride_elems : F;
  if (T == 0) return SPP_OK;
  SPP_REQUIRE(d.grad_w_dev || d.num_edges == 0, "%s: NULL buffer (grad_w)", who);
  SPP_REQUIRE(aligned_to(d.grad_w_dev, 4) && aligned_to(d.grad_self_w_dev, 4),
              "%s: misaligned buffer (grad_w or grad_self_w is not aligned to its element)", who);
  hipStream_t st = as_stream(stream);
  if (F == 0) {  // empty dot products
    if (d.num_edges > 0) SPP_HIP_TRY(hipMemsetAsync(d.grad_w_dev, 0, 4 * (size_t)d.num_edges, st));
    if (d.grad_self_w_dev) SPP_HIP_TRY(hipMemsetAsync(d.grad_self_w_dev, 0, 4 * (size_t)T, st));
    return SPP_OK;
  }
  SPP_TRY(check_rows(who, r));
  SPP_REQUIRE(d.grad_out_dev, "%s: NULL buffer (grad_out)", who);
  SPP_REQUIRE(aligned_to(d.grad_out_dev, elem_bytes(d.grad_elem)),
              "%s: misaligned buffer (grad_out is not aligned to its element)", who);
  const bool vec = rows_vec(r) && gs % 4 == 0 && aligned_to(d.grad_out_dev, 4 * elem_bytes(d.grad_elem));
  const int lpr_log2 = lanes_log2(vec ? F / 4 : F);
  const unsigned grid = (unsigned)ceil_div(T << lpr_log2, kNT);
  with_source(d.source, [&](auto src) {
    with_elem_vec(d.x_elem, vec, [&](auto tin, auto v) {
      with_f32_bf16(d.grad_elem, [&](auto tg) {
        using Tin = typename decltype(tin)::type;
        using Tg = typename decltype(tg)::type;
        hipLaunchKernelGGL((k_agg_w_wgrad<Tin, Tg, decltype(v)::value, decltype(src)>), dim3(grid), dim3(kNT), 0, st,
                           d.rowptr_dev, d.col_dev, T, static_cast<const Tin*>(d.x_dev), d.x_stride_elems, F, lpr_log2,
                           static_cast<const Tg*>(d.grad_out_dev), gs, d.grad_w_dev, d.grad_self_w_dev, d.n_id_dev,
                           d.x_rows);
      });
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_gcn_norm(const spp_gcn_norm_desc* desc, void* stream) {
  const char* who = "spp_gcn_norm";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_gcn_norm_desc& d = *desc;
  SPP_REQUIRE(d.fill >= 0 && d.fill <= 2, "%s: unknown fill %d (1, 2 for improved, 0 for no self loops)", who, (int)d.fill);
  const int64_t T = d.num_targets, S = d.num_sources, E = d.num_edges;
  SPP_REQUIRE(T >= 0 && S >= T && E >= 0, "%s: bad sizes (T %lld, S %lld, E %lld)", who, (long long)T, (long long)S,
              (long long)E);
  SPP_REQUIRE(T < kMaxElems / 8 && E < kMaxElems / 8, "%s: T or E out of range", who);
  if (T == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr_dev && ((d.col_dev && d.coef_dev) || E == 0), "%s: NULL buffer", who);
  SPP_REQUIRE(d.dinv_dev, "%s: missing workspace (dinv_dev: fp32 [T])", who);
  SPP_REQUIRE(aligned_to(d.w_dev, 4) && aligned_to(d.dinv_dev, 4) && aligned_to(d.coef_dev, 4) &&
                  aligned_to(d.self_coef_dev, 4),
              "%s: misaligned buffer (w, dinv, coef or self_coef is not aligned to its element)", who);
  hipStream_t st = as_stream(stream);
  const float fill = (float)d.fill;
  const float fill_dinv = d.fill ? 1.0f / sqrtf(fill) : 0.f;  // the degree of a source that is no target is `fill`
  const unsigned grid = (unsigned)ceil_div(T, kNT);
  hipLaunchKernelGGL(k_gcn_dinv, dim3(grid), dim3(kNT), 0, st, d.rowptr_dev, d.w_dev, T, fill, d.dinv_dev);
  hipLaunchKernelGGL(k_gcn_coef, dim3(grid), dim3(kNT), 0, st, d.rowptr_dev, d.col_dev, d.w_dev, T, fill, fill_dinv,
                     d.dinv_dev, d.coef_dev, d.self_coef_dev);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// f3s: the first pass alone, over all the rows of a graph -- the per-node factors spp_graph_agg_weighted_forward forms its
// coefficients from.  The same kernel as above, so the same bits; no [E] array.  (With weights one thread walks a whole
// row, a hub's included: once per model evaluation.)
extern "C" spp_status spp_gcn_dinv(const spp_gcn_dinv_desc* desc, void* stream) {
  const char* who = "spp_gcn_dinv";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_gcn_dinv_desc& d = *desc;
  SPP_REQUIRE(d.fill >= 0 && d.fill <= 2, "%s: unknown fill %d (1, 2 for improved, 0 for no self loops)", who, (int)d.fill);
  const int64_t N = d.num_nodes;
  SPP_REQUIRE(N >= 0 && N < kMaxIndex * kNT, "%s: num_nodes %lld negative or too many for one launch", who, (long long)N);
  if (N == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr_dev && d.dinv_dev, "%s: NULL buffer (rowptr or dinv)", who);
  SPP_REQUIRE(aligned_to(d.w_dev, 4) && aligned_to(d.dinv_dev, 4),
              "%s: misaligned buffer (w or dinv is not aligned to its element)", who);
  hipLaunchKernelGGL(k_gcn_dinv, dim3((unsigned)ceil_div(N, kNT)), dim3(kNT), 0, as_stream(stream), d.rowptr_dev, d.w_dev, N,
                     (float)d.fill, d.dinv_dev);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
