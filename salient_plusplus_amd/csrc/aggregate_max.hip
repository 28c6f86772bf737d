// f3q: max aggregation over an MFG hop's CSR -- the message passing of SAGEConv(aggr='max'):
//     out[t,:]  = max_{e in row t} x[col[e],:]   (element-wise; an empty row gives 0)                    forward
//     arg[t,c]  = the source row of the FIRST entry that attains out[t,c] (-1 for an empty row)
//     grad_x[arg[t,c], c] += grad_out[t,c]                                                                backward
// The forward is k_agg_fwd's gather-reduce (aggregate.hip) with a comparison in place of the addition: the same lanes,
// the same loads (agg_rows.hip.h), the same deg * F * s bytes read per target, plus 4 * F bytes of argmax written.  A
// maximum rounds nothing and does not depend on evaluation order, so it is the bits of one of the row's entries.
#include "agg_rows.hip.h"
#include "elem_io.hip.h"

#include <algorithm>
#include <type_traits>

namespace spp {
namespace agg_max {

constexpr int kNT = 256;

// what rides with the launch besides the rows: (scale_log2 is what ColScale4 / ColScale1 read for fp8 rows)
struct MaxArgs {
  int concat_target;
  const int8_t* scale_log2;
  int32_t* arg;  // [T, F] dense, or NULL
};

// The comparison rule (include/spp.h f3q; classify.hip's): v, a LATER entry, replaces the best only if it is strictly
// above or a NaN -- !(v <= best) -- and the best is not a NaN already.
__device__ __forceinline__ void take(float& best, int32_t& at, float v, int32_t j) {
  const bool w = !(v <= best) && best == best;
  best = w ? v : best;
  at = w ? j : at;
}
__device__ __forceinline__ void take4(f4& best, int4& at, f4 v, int32_t j) {
  take(best.x, at.x, v.x, j);
  take(best.y, at.y, v.y, j);
  take(best.z, at.z, v.z, j);
  take(best.w, at.w, v.w, j);
}

// LPR lanes share a target row; VEC4: F % 4 == 0 and rows, outputs and arg aligned to 4 elements.  The row's entries
// are compared in CSR order starting from the first; Tout = bf16 rounds each stored element once.
template <typename Tin, typename Tout, bool VEC4, class Src>
__global__ __launch_bounds__(kNT) void k_agg_max_fwd(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                     int64_t T, const Tin* __restrict__ x, int64_t x_stride, int64_t F,
                                                     int lpr_log2, Tout* __restrict__ out, int64_t out_stride, MaxArgs a,
                                                     const int64_t* __restrict__ nid, int64_t x_rows) {
  constexpr bool kFp8 = std::is_same<Tin, fp8e4m3>::value;
  static_assert(!kFp8 || VEC4, "fp8 rows have the vector form only");
  const Rows<Tin, Src> row{x, x_stride, nid, x_rows};
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  if constexpr (VEC4) {
    for (int64_t c = (int64_t)lane * 4; c < F; c += (int64_t)lpr * 4) {
      const ColScale4<kFp8> sc(a, c);
      if (a.concat_target) store4(out + t * out_stride + F + c, load4(row(t) + c, sc));  // [max | x_target]
      f4 best = {0.f, 0.f, 0.f, 0.f};
      int4 at = make_int4(-1, -1, -1, -1);
      if (b < e) {
        const int64_t j = col[b];
        best = load4(row(j) + c, sc);
        at = make_int4((int32_t)j, (int32_t)j, (int32_t)j, (int32_t)j);
      }
      int64_t k = b + 1;
      for (; k + 1 < e; k += 2) {  // two independent rows in flight
        const int64_t j0 = col[k], j1 = col[k + 1];
        const f4 v0 = load4(row(j0) + c, sc), v1 = load4(row(j1) + c, sc);
        take4(best, at, v0, (int32_t)j0);
        take4(best, at, v1, (int32_t)j1);
      }
      if (k < e) {
        const int64_t j0 = col[k];
        take4(best, at, load4(row(j0) + c, sc), (int32_t)j0);
      }
      store4(out + t * out_stride + c, best);
      if (a.arg) *reinterpret_cast<int4*>(a.arg + t * F + c) = at;
    }
  } else {
    for (int64_t c = lane; c < F; c += lpr) {
      const ColScale1<kFp8> sc(a, c);
      if (a.concat_target) store1(out + t * out_stride + F + c, load1(row(t) + c, sc));
      float best = 0.f;
      int32_t at = -1;
      if (b < e) {
        const int64_t j = col[b];
        best = load1(row(j) + c, sc);
        at = (int32_t)j;
      }
      int64_t k = b + 1;
      for (; k + 1 < e; k += 2) {
        const int64_t j0 = col[k], j1 = col[k + 1];
        const float v0 = load1(row(j0) + c, sc), v1 = load1(row(j1) + c, sc);
        take(best, at, v0, (int32_t)j0);
        take(best, at, v1, (int32_t)j1);
      }
      if (k < e) {
        const int64_t j0 = col[k];
        take(best, at, load1(row(j0) + c, sc), (int32_t)j0);
      }
      store1(out + t * out_stride + c, best);
      if (a.arg) a.arg[t * F + c] = at;
    }
  }
}

// grad_x before the scatter, with concat_target: the first T source rows are the targets themselves and start from the
// gradient of the x_target half, the rest from zero (without concat_target a memset does it).  acc is fp32 [S, F]; any F.
template <typename Tg>
__global__ __launch_bounds__(kNT) void k_agg_max_grad_init(const Tg* __restrict__ g, int64_t go_stride, int64_t T,
                                                           int64_t S, int64_t F, float* __restrict__ acc) {
  const int64_t n = S * F;
  for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNT) {
    const int64_t r = i / F, c = i - r * F;
    acc[i] = r < T ? load1(g + r * go_stride + F + c) : 0.f;
  }
}

// acc[arg[t,c], c] += g[t,c]: one hardware fp32 atomic per (target, column) whose row was not empty
template <typename Tg>
__global__ __launch_bounds__(kNT) void k_agg_max_bwd(const int32_t* __restrict__ arg, const Tg* __restrict__ g,
                                                     int64_t go_stride, int64_t T, int64_t S, int64_t F,
                                                     float* __restrict__ acc) {
  const int64_t n = T * F;
  for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNT) {
    const int64_t t = i / F, c = i - t * F;
    const int64_t s = arg[i];
    if ((uint64_t)s < (uint64_t)S) unsafeAtomicAdd(acc + s * F + c, load1(g + t * go_stride + c));
  }
}

// the bf16 gradient: the atomics' fp32 sums rounded once
__global__ __launch_bounds__(kNT) void k_agg_max_round(const float* __restrict__ acc, int64_t n, bf16* __restrict__ gx) {
  for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNT) store1(gx + i, acc[i]);
}

static unsigned elementwise_grid(int64_t items) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, kNT), 256 * 32));
}

constexpr int64_t kMaxElems = (int64_t)1 << 62;

}  // namespace agg_max
}  // namespace spp

using namespace spp;
using namespace spp::agg_max;

extern "C" spp_status spp_agg_max_forward(const spp_agg_max_fwd_desc* desc, void* stream) {
  const char* who = "spp_agg_max_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_agg_max_fwd_desc& d = *desc;
  const bool fp8 = d.x_elem == SPP_ELEM_FP8_E4M3, refs = d.source == SPP_AGG_ROWS;
  SPP_REQUIRE(d.source >= SPP_AGG_DENSE && d.source <= SPP_AGG_ROWS, "%s: unknown source %d", who, (int)d.source);
  SPP_REQUIRE((fp8 || elem_ok(d.x_elem)) && f32_bf16_ok(d.out_elem),
              "%s: unknown or unsupported element code (x %d, out %d; the output is fp32 or bf16)", who, (int)d.x_elem,
              (int)d.out_elem);
  SPP_REQUIRE(!fp8 || !refs, "%s: fp8 rows take dense rows or the table", who);
  SPP_REQUIRE(!fp8 || d.scale_log2_dev, "%s: fp8 rows need their column exponents (scale_log2_dev)", who);
  const int64_t T = d.num_targets, F = d.F;
  SPP_REQUIRE(T >= 0 && F >= 0, "%s: negative size (T %lld, F %lld)", who, (long long)T, (long long)F);
  SPP_REQUIRE(F == 0 || T < kMaxElems / (2 * F), "%s: T * F out of range", who);
  const int64_t width = d.concat_target ? 2 * F : F;
  SPP_REQUIRE(d.out_stride_elems >= 0 && (d.out_stride_elems == 0 || d.out_stride_elems >= width),
              "%s: output stride smaller than the output row", who);
  const int64_t out_stride = d.out_stride_elems > 0 ? d.out_stride_elems : width;
  if (T == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr_dev && d.col_dev && d.out_dev &&
                  (refs ? d.n_id_dev != nullptr : d.x_dev && (d.source == SPP_AGG_DENSE || (d.n_id_dev && d.x_rows > 0))),
              "%s: NULL buffer or empty table", who);
  SPP_REQUIRE(refs || d.x_stride_elems >= F, "%s: row stride smaller than the row", who);
  SPP_REQUIRE(aligned_to(d.out_dev, elem_bytes(d.out_elem)) && aligned_to(d.arg_dev, 4) &&
                  (refs || aligned_to(d.x_dev, elem_bytes(d.x_elem))),
              "%s: misaligned buffer (x, out or arg is not aligned to its element)", who);
  const bool vec = F % 4 == 0 && out_stride % 4 == 0 && aligned_to(d.out_dev, 4 * elem_bytes(d.out_elem)) &&
                   aligned_to(d.arg_dev, 16) &&
                   (refs || (d.x_stride_elems % 4 == 0 && aligned_to(d.x_dev, 4 * elem_bytes(d.x_elem)))) &&
                   (!fp8 || aligned_to(d.scale_log2_dev, 4));
  if (fp8)
    SPP_REQUIRE(vec, "%s: fp8 rows need F %% 4 == 0, 4-byte aligned rows and exponents and an aligned output and arg (F = %lld)",
                who, (long long)F);
  const int lpr_log2 = lanes_log2(vec ? F / 4 : F);
  const unsigned grid = (unsigned)ceil_div(T << lpr_log2, kNT);
  const MaxArgs a{d.concat_target != 0, d.scale_log2_dev, d.arg_dev};
  auto launch = [&](auto tin, auto tout, auto v, auto src) {
    using Tin = typename decltype(tin)::type;
    using Tout = typename decltype(tout)::type;
    hipLaunchKernelGGL((k_agg_max_fwd<Tin, Tout, decltype(v)::value, decltype(src)>), dim3(grid), dim3(kNT), 0,
                       as_stream(stream), d.rowptr_dev, d.col_dev, T, static_cast<const Tin*>(d.x_dev), d.x_stride_elems, F,
                       lpr_log2, static_cast<Tout*>(d.out_dev), out_stride, a, d.n_id_dev, d.x_rows);
  };
  auto by_type = [&](auto src) {
    with_f32_bf16(d.out_elem, [&](auto tout) {
      if (!fp8)
        with_elem_vec(d.x_elem, vec, [&](auto tin, auto v) { launch(tin, tout, v, src); });
      else if constexpr (!std::is_same<decltype(src), Refs>::value)
        launch(Type<fp8e4m3>{}, tout, std::true_type{}, src);
    });
  };
  d.source == SPP_AGG_TABLE ? by_type(Table{}) : refs ? by_type(Refs{}) : by_type(Dense{});
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_agg_max_backward(const spp_agg_max_bwd_desc* desc, void* stream) {
  const char* who = "spp_agg_max_backward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_agg_max_bwd_desc& d = *desc;
  SPP_REQUIRE(f32_bf16_ok(d.grad_elem) && f32_bf16_ok(d.out_elem),
              "%s: unknown or unsupported element code (grad %d, out %d; fp32 or bf16)", who, (int)d.grad_elem,
              (int)d.out_elem);
  const int64_t T = d.num_targets, S = d.num_sources, F = d.F;
  SPP_REQUIRE(T >= 0 && S >= T && F >= 0, "%s: bad sizes (T %lld, S %lld, F %lld)", who, (long long)T, (long long)S,
              (long long)F);
  SPP_REQUIRE(S < ((int64_t)1 << 31), "%s: S beyond 2^31 (arg is int32)", who);
  SPP_REQUIRE(F == 0 || S < kMaxElems / (2 * F), "%s: S * F out of range", who);
  const int64_t width = d.concat_target ? 2 * F : F;
  SPP_REQUIRE(d.grad_out_stride_elems >= 0 && (d.grad_out_stride_elems == 0 || d.grad_out_stride_elems >= width),
              "%s: gradient stride smaller than the row", who);
  const int64_t gs = d.grad_out_stride_elems > 0 ? d.grad_out_stride_elems : width;
  if (S == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(d.grad_x_dev && ((d.grad_out_dev && d.arg_dev) || T == 0), "%s: NULL buffer", who);
  SPP_REQUIRE(aligned_to(d.grad_x_dev, elem_bytes(d.out_elem)) && aligned_to(d.grad_out_dev, elem_bytes(d.grad_elem)) &&
                  aligned_to(d.arg_dev, 4),
              "%s: misaligned buffer (grad_x, grad_out or arg is not aligned to its element)", who);
  const int64_t n = S * F;
  const bool rounds = d.out_elem != SPP_ELEM_F32;
  if (rounds)
    SPP_REQUIRE(d.workspace_dev && aligned_to(d.workspace_dev, 16) && d.workspace_bytes >= 4 * n,
                "%s: a bf16 gradient needs a 16-byte aligned fp32 workspace of 4 * S * F bytes", who);
  hipStream_t st = as_stream(stream);
  float* acc = static_cast<float*>(rounds ? d.workspace_dev : d.grad_x_dev);
  const bool own = d.concat_target && T > 0;
  if (!own) SPP_HIP_TRY(hipMemsetAsync(acc, 0, 4 * (size_t)n, st));
  with_f32_bf16(d.grad_elem, [&](auto tg) {
    using Tg = typename decltype(tg)::type;
    const Tg* g = static_cast<const Tg*>(d.grad_out_dev);
    if (own)
      hipLaunchKernelGGL(k_agg_max_grad_init<Tg>, dim3(elementwise_grid(n)), dim3(kNT), 0, st, g, gs, T, S, F, acc);
    if (T > 0)
      hipLaunchKernelGGL(k_agg_max_bwd<Tg>, dim3(elementwise_grid(T * F)), dim3(kNT), 0, st, d.arg_dev, g, gs, T, S, F, acc);
  });
  if (rounds)
    hipLaunchKernelGGL(k_agg_max_round, dim3(elementwise_grid(n)), dim3(kNT), 0, st, acc, n,
                       static_cast<bf16*>(d.grad_x_dev));
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
