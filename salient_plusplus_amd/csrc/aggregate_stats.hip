// f4b: mean / min / max / std of an MFG hop's neighbour rows in ONE pass -- the message passing of PNAConv (Principal
// Neighbourhood Aggregation), forward and backward.  For target t with the d entries k of its CSR row, v_k = x[col[k]]:
//     mean_b = K + s1 / d,  s1 = sum (v_k - K)            K = the row's FIRST entry, per column
//     var    = max(s2 / d - (s1 / d)^2, 0),  s2 = sum (v_k - K)^2         std = sqrt(var + eps)
//     min, max by aggregate_max.hip's rule and its mirror image, with the CSR position k of the entry that won
//     out[t] = [scaler][mean + add | min + add | max + add | std][F], scalers 1, log(d + 1) / delta, delta / log(d + 1)
// The forward is k_agg_max_fwd's gather-reduce with seven values a column in registers instead of two: the same lanes,
// the same loads, the same deg * F * s bytes read per target -- four aggregators for the traffic of one.  The backward
// walks the same rows again, target-major: the target's state is loaded once per column chunk and every entry sends ONE
// fp32 atomic per column to its source row (DESIGN section 7 f4b has the argument against the gather form).
#include "elem_io.hip.h"

#include <algorithm>

namespace spp {
namespace agg_stats {

constexpr int kNT = 256;
constexpr int kMaxScalers = 3;

// what rides with either launch besides the rows
struct StatsArgs {
  int n_scalers;
  int kind[kMaxScalers];  // 0 identity, 1 amplification, 2 attenuation: the enabled ones, in that order
  float delta, eps;
  const float* add;  // [T, F] dense, or NULL
  float* stats;      // [T, 2F] dense: mean_b | std
  int32_t* pos;      // [T, 2F] dense: kmin | kmax
};

// aggregate_max.hip's comparison rule and its mirror image: v, a LATER entry, replaces the best only if it is strictly
// better or a NaN, and the best is not a NaN already.  `at` is the entry's CSR position.
__device__ __forceinline__ void take_max(float& best, int32_t& at, float v, int32_t k) {
  const bool w = !(v <= best) && best == best;
  best = w ? v : best;
  at = w ? k : at;
}
__device__ __forceinline__ void take_min(float& best, int32_t& at, float v, int32_t k) {
  const bool w = !(v >= best) && best == best;
  best = w ? v : best;
  at = w ? k : at;
}

// one column's running state: 7 registers
struct Col {
  float mn, mx, K, s1, s2;
  int32_t kmn, kmx;
  __device__ __forceinline__ void first(float v, int32_t k) {
    mn = mx = K = v;
    kmn = kmx = k;
    s1 = s2 = 0.f;
  }
  __device__ __forceinline__ void next(float v, int32_t k) {
    take_min(mn, kmn, v, k);
    take_max(mx, kmx, v, k);
    const float dv = v - K;  // shifted: a column like 1000 + noise keeps its digits (E[x^2] - E[x]^2 would lose them all)
    s1 += dv;
    s2 = fmaf(dv, dv, s2);
  }
};

__device__ __forceinline__ float scaler(int kind, float logd, float delta) {
  return kind == 0 ? 1.f : kind == 1 ? logd / delta : delta / logd;
}

__device__ __forceinline__ f4 times(f4 a, float s) { return {a.x * s, a.y * s, a.z * s, a.w * s}; }
__device__ __forceinline__ f4 plus(f4 a, f4 b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

// LPR lanes share a target row; a lane takes 4 columns and loops c += 4 * LPR.  Entries in CSR order from the first, two
// rows in flight, a one-entry tail.  Tout = bf16 rounds each stored element once.
template <typename Tin, typename Tout>
__global__ __launch_bounds__(kNT) void k_agg_stats_fwd(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                       int64_t T, const Tin* __restrict__ x, int64_t x_stride, int64_t F,
                                                       int lpr_log2, Tout* __restrict__ out, int64_t out_stride,
                                                       StatsArgs a) {
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  const float inv = 1.f / (float)(e - b), logd = logf((float)(e - b) + 1.f);
  Tout* o = out + t * out_stride;
  for (int64_t c = (int64_t)lane * 4; c < F; c += (int64_t)lpr * 4) {
    if (b >= e) {  // an empty row: zeros everywhere, no position
      const f4 z = {0.f, 0.f, 0.f, 0.f};
      for (int64_t w = 0; w < 4 * a.n_scalers; ++w) store4(o + w * F + c, z);
      if (a.stats) {
        store4(a.stats + t * 2 * F + c, z);
        store4(a.stats + t * 2 * F + F + c, z);
        const int4 none = make_int4(-1, -1, -1, -1);
        *reinterpret_cast<int4*>(a.pos + t * 2 * F + c) = none;
        *reinterpret_cast<int4*>(a.pos + t * 2 * F + F + c) = none;
      }
      continue;
    }
    Col q0, q1, q2, q3;
    {
      const f4 v = load4(x + col[b] * x_stride + c);
      q0.first(v.x, (int32_t)b), q1.first(v.y, (int32_t)b), q2.first(v.z, (int32_t)b), q3.first(v.w, (int32_t)b);
    }
    int64_t k = b + 1;
    for (; k + 1 < e; k += 2) {  // two independent rows in flight
      const int64_t j0 = col[k], j1 = col[k + 1];
      const f4 v0 = load4(x + j0 * x_stride + c), v1 = load4(x + j1 * x_stride + c);
      q0.next(v0.x, (int32_t)k), q1.next(v0.y, (int32_t)k), q2.next(v0.z, (int32_t)k), q3.next(v0.w, (int32_t)k);
      q0.next(v1.x, (int32_t)k + 1), q1.next(v1.y, (int32_t)k + 1), q2.next(v1.z, (int32_t)k + 1), q3.next(v1.w, (int32_t)k + 1);
    }
    if (k < e) {
      const f4 v = load4(x + col[k] * x_stride + c);
      q0.next(v.x, (int32_t)k), q1.next(v.y, (int32_t)k), q2.next(v.z, (int32_t)k), q3.next(v.w, (int32_t)k);
    }
    const f4 m1 = {q0.s1 * inv, q1.s1 * inv, q2.s1 * inv, q3.s1 * inv};
    f4 mean = {q0.K + m1.x, q1.K + m1.y, q2.K + m1.z, q3.K + m1.w};
    const f4 sd = {sqrtf(fmaxf(q0.s2 * inv - m1.x * m1.x, 0.f) + a.eps), sqrtf(fmaxf(q1.s2 * inv - m1.y * m1.y, 0.f) + a.eps),
                   sqrtf(fmaxf(q2.s2 * inv - m1.z * m1.z, 0.f) + a.eps), sqrtf(fmaxf(q3.s2 * inv - m1.w * m1.w, 0.f) + a.eps)};
    f4 mn = {q0.mn, q1.mn, q2.mn, q3.mn}, mx = {q0.mx, q1.mx, q2.mx, q3.mx};
    if (a.stats) {
      store4(a.stats + t * 2 * F + c, mean);
      store4(a.stats + t * 2 * F + F + c, sd);
      *reinterpret_cast<int4*>(a.pos + t * 2 * F + c) = make_int4(q0.kmn, q1.kmn, q2.kmn, q3.kmn);
      *reinterpret_cast<int4*>(a.pos + t * 2 * F + F + c) = make_int4(q0.kmx, q1.kmx, q2.kmx, q3.kmx);
    }
    if (a.add) {  // the target's own half of the message: mean, min and max move with it, the spread does not
      const f4 ad = load4(a.add + t * F + c);
      mean = plus(mean, ad), mn = plus(mn, ad), mx = plus(mx, ad);
    }
    for (int s = 0; s < a.n_scalers; ++s) {
      const float sc = scaler(a.kind[s], logd, a.delta);
      Tout* os = o + (int64_t)s * 4 * F + c;
      store4(os, times(mean, sc));
      store4(os + F, times(mn, sc));
      store4(os + 2 * F, times(mx, sc));
      store4(os + 3 * F, times(sd, sc));
    }
  }
}

// grad_x[col[k], c] += G_mean / d + G_std (v - mean_b) / (d std) + [k == kmin] G_min + [k == kmax] G_max, one atomic per
// (entry, column); G_a = sum_s scale_s(t) g[t, s, a, c].  grad_add[t, c] = G_mean + G_min + G_max, a plain store.
template <typename Tin, typename Tg>
__global__ __launch_bounds__(kNT) void k_agg_stats_bwd(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                       int64_t T, const Tin* __restrict__ x, int64_t x_stride, int64_t F,
                                                       int lpr_log2, const Tg* __restrict__ g, int64_t g_stride,
                                                       StatsArgs a, int64_t S, float* __restrict__ grad_x,
                                                       float* __restrict__ grad_add) {
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  const float inv = 1.f / (float)(e - b), logd = logf((float)(e - b) + 1.f);
  const Tg* gt = g + t * g_stride;
  for (int64_t c = (int64_t)lane * 4; c < F; c += (int64_t)lpr * 4) {
    if (b >= e) {
      if (grad_add) store4(grad_add + t * F + c, f4{0.f, 0.f, 0.f, 0.f});
      continue;
    }
    f4 Gm = {0.f, 0.f, 0.f, 0.f}, Gn = Gm, Gx = Gm, Gs = Gm;
    for (int s = 0; s < a.n_scalers; ++s) {
      const float sc = scaler(a.kind[s], logd, a.delta);
      const Tg* gs = gt + (int64_t)s * 4 * F + c;
      Gm = Piece<true>::fma(sc, load4(gs), Gm);
      Gn = Piece<true>::fma(sc, load4(gs + F), Gn);
      Gx = Piece<true>::fma(sc, load4(gs + 2 * F), Gx);
      Gs = Piece<true>::fma(sc, load4(gs + 3 * F), Gs);
    }
    if (grad_add) store4(grad_add + t * F + c, plus(plus(Gm, Gn), Gx));
    const f4 mean = load4(a.stats + t * 2 * F + c), sd = load4(a.stats + t * 2 * F + F + c);
    const int4 kmn = *reinterpret_cast<const int4*>(a.pos + t * 2 * F + c);
    const int4 kmx = *reinterpret_cast<const int4*>(a.pos + t * 2 * F + F + c);
    const f4 cm = times(Gm, inv);
    const f4 cs = {Gs.x * inv / sd.x, Gs.y * inv / sd.y, Gs.z * inv / sd.z, Gs.w * inv / sd.w};
    auto send = [&](int64_t j, f4 v, int32_t k) {
      if ((uint64_t)j >= (uint64_t)S) return;  // (a col entry outside the sources: skipped, as spp_agg_max_backward does)
      float* dst = grad_x + j * F + c;
      unsafeAtomicAdd(dst + 0, fmaf(cs.x, v.x - mean.x, cm.x) + (k == kmn.x ? Gn.x : 0.f) + (k == kmx.x ? Gx.x : 0.f));
      unsafeAtomicAdd(dst + 1, fmaf(cs.y, v.y - mean.y, cm.y) + (k == kmn.y ? Gn.y : 0.f) + (k == kmx.y ? Gx.y : 0.f));
      unsafeAtomicAdd(dst + 2, fmaf(cs.z, v.z - mean.z, cm.z) + (k == kmn.z ? Gn.z : 0.f) + (k == kmx.z ? Gx.z : 0.f));
      unsafeAtomicAdd(dst + 3, fmaf(cs.w, v.w - mean.w, cm.w) + (k == kmn.w ? Gn.w : 0.f) + (k == kmx.w ? Gx.w : 0.f));
    };
    int64_t k = b;
    for (; k + 1 < e; k += 2) {  // two independent rows in flight
      const int64_t j0 = col[k], j1 = col[k + 1];
      const f4 v0 = load4(x + j0 * x_stride + c), v1 = load4(x + j1 * x_stride + c);
      send(j0, v0, (int32_t)k);
      send(j1, v1, (int32_t)k + 1);
    }
    if (k < e) {
      const int64_t j0 = col[k];
      send(j0, load4(x + j0 * x_stride + c), (int32_t)k);
    }
  }
}

constexpr int64_t kMaxElems = (int64_t)1 << 62;

// the checks both entries share, in the order the header states; fills the launch record
static spp_status common(const char* who, const spp_agg_stats_desc& d, bool backward, StatsArgs* a, int64_t* width) {
  SPP_REQUIRE(elem_ok(d.x_elem) && f32_bf16_ok(backward ? d.grad_elem : d.out_elem),
              "%s: unknown or unsupported element code (x %d, %s %d; rows fp32 / fp16 / bf16, the %s fp32 or bf16)", who,
              (int)d.x_elem, backward ? "grad" : "out", (int)(backward ? d.grad_elem : d.out_elem),
              backward ? "gradient" : "output");
  SPP_REQUIRE(d.scalers >= 1 && d.scalers <= 7, "%s: scalers must be a non-empty mask of identity 1, amplification 2, "
              "attenuation 4 (got %d)", who, (int)d.scalers);
  SPP_REQUIRE(d.delta > 0.f && d.delta <= 3.0e38f && d.eps >= 0.f && d.eps <= 3.0e38f,
              "%s: delta must be positive and eps non-negative, both finite", who);
  const int64_t T = d.num_targets, S = d.num_sources, E = d.num_edges, F = d.F;
  SPP_REQUIRE(T >= 0 && S >= 0 && E >= 0 && F >= 0, "%s: negative size (T %lld, S %lld, E %lld, F %lld)", who, (long long)T,
              (long long)S, (long long)E, (long long)F);
  SPP_REQUIRE(E < ((int64_t)1 << 31), "%s: E beyond 2^31 (positions are int32)", who);
  SPP_REQUIRE(F % 4 == 0, "%s: F %% 4 != 0 (F = %lld): four columns per lane only", who, (long long)F);
  SPP_REQUIRE(F == 0 || (T < kMaxElems / (12 * F) && S < kMaxElems / F), "%s: T * F or S * F out of range", who);
  a->n_scalers = 0;
  for (int s = 0; s < kMaxScalers; ++s)
    if (d.scalers >> s & 1) a->kind[a->n_scalers++] = s;
  *width = (int64_t)a->n_scalers * 4 * F;
  a->delta = d.delta, a->eps = d.eps, a->add = d.add_dev, a->stats = d.stats_dev, a->pos = d.pos_dev;
  return SPP_OK;
}

}  // namespace agg_stats
}  // namespace spp

using namespace spp;
using namespace spp::agg_stats;

extern "C" spp_status spp_agg_stats_forward(const spp_agg_stats_desc* desc, void* stream) {
  const char* who = "spp_agg_stats_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_agg_stats_desc& d = *desc;
  StatsArgs a;
  int64_t width;
  SPP_TRY(common(who, d, false, &a, &width));
  const int64_t T = d.num_targets, F = d.F;
  SPP_REQUIRE(d.out_stride_elems >= 0 && (d.out_stride_elems == 0 || d.out_stride_elems >= width),
              "%s: output stride smaller than the output row", who);
  const int64_t out_stride = d.out_stride_elems > 0 ? d.out_stride_elems : width;
  if (T == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr_dev && d.out_dev && (d.num_edges == 0 || (d.col_dev && d.x_dev)), "%s: NULL buffer", who);
  SPP_REQUIRE((d.stats_dev != nullptr) == (d.pos_dev != nullptr), "%s: stats and pos come together or not at all", who);
  SPP_REQUIRE(d.x_stride_elems >= F, "%s: row stride smaller than the row", who);
  SPP_REQUIRE(d.x_stride_elems % 4 == 0 && out_stride % 4 == 0 && aligned_to(d.x_dev, 4 * elem_bytes(d.x_elem)) &&
                  aligned_to(d.out_dev, 4 * elem_bytes(d.out_elem)) && aligned_to(d.add_dev, 16) &&
                  aligned_to(d.stats_dev, 16) && aligned_to(d.pos_dev, 16),
              "%s: misaligned buffer (rows, out, add, stats and pos are aligned to 4 elements)", who);
  const int lpr_log2 = lanes_log2(F / 4);
  const unsigned grid = (unsigned)ceil_div(T << lpr_log2, kNT);
  with_elem(d.x_elem, [&](auto tin) {
    with_f32_bf16(d.out_elem, [&](auto tout) {
      using Tin = typename decltype(tin)::type;
      using Tout = typename decltype(tout)::type;
      hipLaunchKernelGGL((k_agg_stats_fwd<Tin, Tout>), dim3(grid), dim3(kNT), 0, as_stream(stream), d.rowptr_dev, d.col_dev,
                         T, static_cast<const Tin*>(d.x_dev), d.x_stride_elems, F, lpr_log2, static_cast<Tout*>(d.out_dev),
                         out_stride, a);
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_agg_stats_backward(const spp_agg_stats_desc* desc, void* stream) {
  const char* who = "spp_agg_stats_backward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_agg_stats_desc& d = *desc;
  StatsArgs a;
  int64_t width;
  SPP_TRY(common(who, d, true, &a, &width));
  const int64_t T = d.num_targets, F = d.F;
  SPP_REQUIRE(d.grad_out_stride_elems >= 0 && (d.grad_out_stride_elems == 0 || d.grad_out_stride_elems >= width),
              "%s: gradient stride smaller than the row", who);
  const int64_t gs = d.grad_out_stride_elems > 0 ? d.grad_out_stride_elems : width;
  if (T == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr_dev && d.grad_out_dev && d.stats_dev && d.pos_dev &&
                  (d.num_edges == 0 || (d.col_dev && d.x_dev && d.grad_x_dev)),
              "%s: NULL buffer", who);
  SPP_REQUIRE(d.x_stride_elems >= F, "%s: row stride smaller than the row", who);
  SPP_REQUIRE(d.x_stride_elems % 4 == 0 && gs % 4 == 0 && aligned_to(d.x_dev, 4 * elem_bytes(d.x_elem)) &&
                  aligned_to(d.grad_out_dev, 4 * elem_bytes(d.grad_elem)) && aligned_to(d.grad_x_dev, 16) &&
                  aligned_to(d.grad_add_dev, 16) && aligned_to(d.stats_dev, 16) && aligned_to(d.pos_dev, 16),
              "%s: misaligned buffer (rows, grad_out, grad_x, grad_add, stats and pos are aligned to 4 elements)", who);
  const int lpr_log2 = lanes_log2(F / 4);
  const unsigned grid = (unsigned)ceil_div(T << lpr_log2, kNT);
  with_elem(d.x_elem, [&](auto tin) {
    with_f32_bf16(d.grad_elem, [&](auto tg) {
      using Tin = typename decltype(tin)::type;
      using Tg = typename decltype(tg)::type;
      hipLaunchKernelGGL((k_agg_stats_bwd<Tin, Tg>), dim3(grid), dim3(kNT), 0, as_stream(stream), d.rowptr_dev, d.col_dev, T,
                         static_cast<const Tin*>(d.x_dev), d.x_stride_elems, F, lpr_log2,
                         static_cast<const Tg*>(d.grad_out_dev), gs, a, d.num_sources, d.grad_x_dev, d.grad_add_dev);
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
