// f3p: the training form of the layer tail behind a GEMM in GIN and SAGEResInception,
//     y = dropout(act(BatchNorm(z))) [+ r]      on batch statistics, forward and backward
// (include/spp.h, spp_bn_act_forward / spp_bn_act_backward, states the contract; resinc_epilogue.hip is the eval-only,
// forward-only relative).  As torch ops the tail is four to six passes over a [n, C] matrix in each direction and keeps
// the BatchNorm output and the dropout mask alive; here the forward reads z twice (statistics, then the tail) and the
// backward reads g and z twice (column sums, then dz), and what is saved for backward is z, mean and invstd.
//
// Shape, every kernel: lpr lanes (a power of two, at most 64) own one row of `pieces` pieces (W = 4 columns in the
// vector form, 1 otherwise), a workgroup's 256 / lpr lane groups take different rows, columns beyond lpr pieces are
// walked in chunks.  At C = 256 one wave covers a row with 16-byte loads and the four waves take different rows.
//   k_bn_stats / k_bn_bwd_sums   one workgroup per slab of kSlab rows: a thread folds its rows (loads of kUnroll rows
//                                issued back to back), the lane groups meet in LDS once per slab and column chunk, in
//                                a fixed order; the slab's per-column record goes to the workspace
//   k_bn_finalize                4 columns x 64 slab lanes per workgroup: lane j folds slabs j, j + 64, ... in that
//                                order, the 64 lanes meet in LDS in lane order; fp64; writes the [C] results
//   k_bn_act_fwd / k_bn_act_bwd  row tiles of (256 / lpr) * kUnroll rows, element-wise
// No atomics, no scratch, every offset 64-bit; vector or scalar form is a launch-time (workgroup-uniform) choice.
#include "act_keep.hip.h"
#include "elem_io.hip.h"

#include <algorithm>

namespace spp {
namespace bnact {

constexpr int kNT = 256;
constexpr int kUnroll = 4;                  // rows in flight per lane group
constexpr int kSlab = SPP_BN_ACT_SLAB_ROWS; // rows per statistics slab
constexpr int kFinCols = 4, kFinLanes = 64;  // many slabs, few columns: the slab walk is the long axis

struct NoRes {};  // the residual's element type when there is none

struct Args {
  const float* gamma;
  const float* beta;
  float* mean;
  float* invstd;
  float* running_mean;
  float* running_var;
  const int64_t* nbt;
  float* out0;  // finalize (backward): dbeta
  float* out1;  // finalize (backward): dgamma
  float* ws;    // [nslabs, C, 3] (statistics) or [nslabs, C, 2] (backward sums)
  int64_t n, C, nslabs;
  double momentum, eps;
  float slope;
  int32_t act, training;
  int lpr_log2;
  ActArgs drop;  // drop.training: dropout is applied (training and p > 0)
};

template <bool VEC, typename T>
__device__ __forceinline__ void ld(const T* p, float* v) {
  if constexpr (VEC) {
    const f4 q = load4(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = load1(p);
  }
}
template <bool VEC>
__device__ __forceinline__ void ld(const NoRes*, float*) {}
template <bool VEC, typename T>
__device__ __forceinline__ void st(T* p, const float* v) {
  if constexpr (VEC) store4(p, f4{v[0], v[1], v[2], v[3]});
  else store1(p, v[0]);
}

// the contract's expressions, shared by forward and backward so that the sign of u is the same in both
__device__ __forceinline__ float xhat(float z, float mean, float invstd) { return __fmul_rn(__fsub_rn(z, mean), invstd); }
// u = gamma * (z - mean) * invstd + beta of the fp32 operands, rounded ONCE (to within the second-order terms dropped
// below) instead of three times: every fp32 operation's rounding error is recovered exactly (the two-sum of z - mean and
// of t + beta, the fma residuals of the two products) and added back before the last rounding.  fp32 arithmetic only;
// the intrinsics keep the compiler from contracting the error terms away.
__device__ __forceinline__ float pre_act(float z, float mean, float invstd, float gamma, float beta) {
  const float pa = __fmul_rn(gamma, invstd), ea = fmaf(gamma, invstd, -pa);  // gamma * invstd = pa + ea (per column)
  const float dh = __fsub_rn(z, mean), bd = __fsub_rn(dh, z);
  const float dl = __fadd_rn(__fsub_rn(z, __fsub_rn(dh, bd)), __fsub_rn(-mean, bd));  // z - mean = dh + dl
  const float t = __fmul_rn(dh, pa), et = fmaf(dh, pa, -t);                             // dh * pa = t + et
  const float corr = __fadd_rn(et, fmaf(dh, ea, __fmul_rn(dl, pa)));
  const float sh = __fadd_rn(t, beta), bs = __fsub_rn(sh, t);
  const float sl = __fadd_rn(__fsub_rn(t, __fsub_rn(sh, bs)), __fsub_rn(beta, bs));      // t + beta = sh + sl
  return __fadd_rn(sh, __fadd_rn(sl, corr));
}

// keep / drop of the W elements at flat index e of the dense [n, C] array
template <bool VEC>
__device__ __forceinline__ void keep_of(int64_t e, int64_t total, const ActArgs& d, bool* k) {
  if constexpr (VEC) {
    const Keep4 q = keep4(e >> 2, d);
    k[0] = q.x, k[1] = q.y, k[2] = q.z, k[3] = q.w;
  } else {
    k[0] = keep1(e, total, d);
  }
}

// where this thread works: its lane group's first row offset, its lane in the row
struct Where {
  int lpr, gpb, g, l;
  int64_t pieces;
};
template <int W>
__device__ __forceinline__ Where where(const Args& a) {
  Where w;
  w.lpr = 1 << a.lpr_log2, w.gpb = kNT >> a.lpr_log2;
  w.g = threadIdx.x >> a.lpr_log2, w.l = threadIdx.x & (w.lpr - 1);
  w.pieces = a.C / W;
  return w;
}

// ---- forward statistics: per slab, per column (mean, M2) ----
template <typename Tz, bool VEC>
__global__ __launch_bounds__(kNT) void k_bn_stats(const Tz* __restrict__ z, Args a) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ float s_m[kNT * W], s_q[kNT * W];
  const Where t = where<W>(a);
  const int64_t row0 = (int64_t)blockIdx.x * kSlab;
  const int rows = (int)std::min<int64_t>(kSlab, a.n - row0);  // >= 1: the grid is the slab count
  for (int64_t p0 = 0; p0 < t.pieces; p0 += t.lpr) {             // (workgroup-uniform bounds)
    const int64_t p = p0 + t.l;
    const bool on = p < t.pieces;
    const int64_t c = (on ? p : 0) * W;
    float m[W], q[W];
#pragma unroll
    for (int w = 0; w < W; ++w) m[w] = 0.f, q[w] = 0.f;
    for (int k0 = 0; k0 * t.gpb < rows; k0 += kUnroll) {
      float v[kUnroll][W];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int il = t.g + (k0 + u) * t.gpb;
        ld<VEC>(z + (row0 + (il < rows ? il : rows - 1)) * a.C + c, v[u]);  // (clamped: loaded, not folded)
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (t.g + (k0 + u) * t.gpb < rows) {  // a thread's valid rows are a prefix: row k is its (k + 1)-th value
          const float inv = 1.f / (float)(k0 + u + 1);
#pragma unroll
          for (int w = 0; w < W; ++w) {
            const float d = v[u][w] - m[w];
            m[w] += d * inv;
            q[w] += d * (v[u][w] - m[w]);
          }
        }
      }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) s_m[threadIdx.x * W + w] = m[w], s_q[threadIdx.x * W + w] = q[w];
    __syncthreads();
    if (t.g == 0 && on) {
      const int groups = rows < t.gpb ? rows : t.gpb;  // lane group g holds ceil((rows - g) / gpb) rows
#pragma unroll
      for (int w = 0; w < W; ++w) {
        double cn = 0., cm = 0., cq = 0.;
        for (int g = 0; g < groups; ++g) {
          const double bn = (double)((rows - g + t.gpb - 1) / t.gpb);
          const double bm = s_m[(g * t.lpr + t.l) * W + w], bq = s_q[(g * t.lpr + t.l) * W + w];
          const double tot = cn + bn, d = bm - cm;
          cm += d * (bn / tot);
          cq += bq + d * d * (cn * bn / tot);
          cn = tot;
        }
        // the slab's mean as an fp32 pair (hi + lo), so that the final mean is rounded once, not once per slab
        float* o = a.ws + ((int64_t)blockIdx.x * a.C + c + w) * 3;
        const float hi = (float)cm;
        o[0] = hi, o[1] = (float)(cm - (double)hi), o[2] = (float)cq;
      }
    }
    __syncthreads();
  }
}

// ---- the slabs' records to the [C] results, in a fixed order, fp64 ----
// kStats: records are (mean hi, mean lo, M2) of min(kSlab, n - s * kSlab) rows, folded by Chan's update; writes mean,
// invstd and the running buffers.  !kStats: records are two partial sums, added; writes out0 (dbeta) and out1 (dgamma).
template <bool kStats>
__global__ __launch_bounds__(kFinCols* kFinLanes) void k_bn_finalize(Args a) {
  __shared__ double s_n[kFinCols * kFinLanes], s_a[kFinCols * kFinLanes], s_b[kFinCols * kFinLanes];
  const int cl = threadIdx.x % kFinCols, j = threadIdx.x / kFinCols;
  const int64_t col = (int64_t)blockIdx.x * kFinCols + cl;
  const bool on = col < a.C;
  double cn = 0., ca = 0., cb = 0.;
  if (on) {
    for (int64_t s = j; s < a.nslabs; s += kFinLanes) {
      if constexpr (kStats) {
        const float* pr = a.ws + (s * a.C + col) * 3;
        const double bn = (double)std::min<int64_t>(kSlab, a.n - s * kSlab);
        const double tot = cn + bn, d = ((double)pr[0] + (double)pr[1]) - ca;
        ca += d * (bn / tot);
        cb += (double)pr[2] + d * d * (cn * bn / tot);
        cn = tot;
      } else {
        const float2 pr = *reinterpret_cast<const float2*>(a.ws + (s * a.C + col) * 2);
        ca += (double)pr.x, cb += (double)pr.y;
      }
    }
  }
  s_n[threadIdx.x] = cn, s_a[threadIdx.x] = ca, s_b[threadIdx.x] = cb;
  __syncthreads();
  if (j != 0 || !on) return;
  for (int k = 1; k < kFinLanes; ++k) {
    const double bn = s_n[k * kFinCols + cl], ba = s_a[k * kFinCols + cl], bb = s_b[k * kFinCols + cl];
    if constexpr (kStats) {
      if (bn > 0.) {
        const double tot = cn + bn, d = ba - ca;
        ca += d * (bn / tot);
        cb += bb + d * d * (cn * bn / tot);
        cn = tot;
      }
    } else {
      ca += ba, cb += bb;
    }
  }
  if constexpr (kStats) {
    const double var = cb / (double)a.n;
    a.mean[col] = (float)ca;
    a.invstd[col] = (float)(1.0 / sqrt(var + a.eps));
    if (a.running_mean) {
      const double f = a.momentum < 0. ? 1.0 / (double)*a.nbt : a.momentum;
      a.running_mean[col] = (float)((1.0 - f) * (double)a.running_mean[col] + f * ca);
      a.running_var[col] = (float)((1.0 - f) * (double)a.running_var[col] + f * (cb / (double)(a.n - 1)));
    }
  } else {
    a.out0[col] = (float)ca;
    a.out1[col] = (float)cb;
  }
}

// eval: mean = running_mean, invstd = 1 / sqrt(running_var + eps)
__global__ __launch_bounds__(kNT) void k_bn_eval_stats(Args a) {
  const int64_t c = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (c < a.C) {
    a.mean[c] = a.running_mean[c];
    a.invstd[c] = (float)(1.0 / sqrt((double)a.running_var[c] + a.eps));
  }
}

__device__ __forceinline__ float act_of(float u, int act, float slope) {
  return (u > 0.f || act == SPP_BN_ACT_NONE) ? u : act == SPP_BN_ACT_RELU ? 0.f : __fmul_rn(slope, u);
}
// g * act'(u)
__device__ __forceinline__ float act_grad(float g, float u, int act, float slope) {
  return (u > 0.f || act == SPP_BN_ACT_NONE) ? g : act == SPP_BN_ACT_RELU ? 0.f : __fmul_rn(slope, g);
}

// ---- forward tail ----
template <typename Tz, typename Tr, typename Ty, bool VEC>
__global__ __launch_bounds__(kNT) void k_bn_act_fwd(const Tz* __restrict__ z, const Tr* __restrict__ r,
                                                    Ty* __restrict__ y, Args a) {
  constexpr int W = VEC ? 4 : 1;
  constexpr bool kRes = !std::is_same<Tr, NoRes>::value;
  const Where t = where<W>(a);
  const int64_t base = (int64_t)blockIdx.x * t.gpb * kUnroll, total = a.n * a.C;
  int64_t i[kUnroll];
  bool ok[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int64_t iu = base + (int64_t)u * t.gpb + t.g;
    ok[u] = iu < a.n;
    i[u] = ok[u] ? iu : a.n - 1;  // (clamped: loaded, never stored)
  }
  for (int64_t p0 = 0; p0 < t.pieces; p0 += t.lpr) {  // (workgroup-uniform bounds)
    const int64_t p = p0 + t.l;
    const bool on = p < t.pieces;
    const int64_t c = (on ? p : 0) * W;
    float mean[W], invstd[W], gamma[W], beta[W];
#pragma unroll
    for (int w = 0; w < W; ++w) mean[w] = a.mean[c + w], invstd[w] = a.invstd[c + w], gamma[w] = a.gamma[c + w], beta[w] = a.beta[c + w];
    float zv[kUnroll][W], rv[kUnroll][W];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) ld<VEC>(z + i[u] * a.C + c, zv[u]);
    if constexpr (kRes) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) ld<VEC>(r + i[u] * a.C + c, rv[u]);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      bool keep[W];
      if (a.drop.training) keep_of<VEC>(i[u] * a.C + c, total, a.drop, keep);  // (a kernel argument: a scalar branch)
      float o[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const float uu = pre_act(zv[u][w], mean[w], invstd[w], gamma[w], beta[w]);
        float v = act_of(uu, a.act, a.slope);
        if (a.drop.training) v = keep[w] ? __fmul_rn(v, a.drop.scale) : 0.f;
        o[w] = kRes ? __fadd_rn(v, rv[u][w]) : v;
      }
      if (ok[u] && on) st<VEC>(y + i[u] * a.C + c, o);
    }
  }
}

// ---- backward: per slab, per column (sum g_a, sum g_a * xh) ----
template <typename Tg, typename Tz, bool VEC>
__global__ __launch_bounds__(kNT) void k_bn_bwd_sums(const Tg* __restrict__ g, const Tz* __restrict__ z, Args a) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ float s_b[kNT * W], s_g[kNT * W];
  const Where t = where<W>(a);
  const int64_t row0 = (int64_t)blockIdx.x * kSlab, total = a.n * a.C;
  const int rows = (int)std::min<int64_t>(kSlab, a.n - row0);
  for (int64_t p0 = 0; p0 < t.pieces; p0 += t.lpr) {
    const int64_t p = p0 + t.l;
    const bool on = p < t.pieces;
    const int64_t c = (on ? p : 0) * W;
    float mean[W], invstd[W], gamma[W], beta[W], sb[W], sg[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      mean[w] = a.mean[c + w], invstd[w] = a.invstd[c + w], gamma[w] = a.gamma[c + w], beta[w] = a.beta[c + w];
      sb[w] = 0.f, sg[w] = 0.f;
    }
    for (int k0 = 0; k0 * t.gpb < rows; k0 += kUnroll) {
      float zv[kUnroll][W], gv[kUnroll][W];
      int64_t i[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int il = t.g + (k0 + u) * t.gpb;
        i[u] = row0 + (il < rows ? il : rows - 1);
        ld<VEC>(z + i[u] * a.C + c, zv[u]);
        ld<VEC>(g + i[u] * a.C + c, gv[u]);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (t.g + (k0 + u) * t.gpb < rows) {
          bool keep[W];
          if (a.drop.training) keep_of<VEC>(i[u] * a.C + c, total, a.drop, keep);
#pragma unroll
          for (int w = 0; w < W; ++w) {
            const float xh = xhat(zv[u][w], mean[w], invstd[w]);
            float gg = gv[u][w];
            if (a.drop.training) gg = keep[w] ? __fmul_rn(gg, a.drop.scale) : 0.f;
            const float ga = act_grad(gg, pre_act(zv[u][w], mean[w], invstd[w], gamma[w], beta[w]), a.act, a.slope);
            sb[w] += ga;
            sg[w] = fmaf(ga, xh, sg[w]);
          }
        }
      }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) s_b[threadIdx.x * W + w] = sb[w], s_g[threadIdx.x * W + w] = sg[w];
    __syncthreads();
    if (t.g == 0 && on) {
      const int groups = rows < t.gpb ? rows : t.gpb;  // the other lane groups hold zeros
#pragma unroll
      for (int w = 0; w < W; ++w) {
        double cb = 0., cg = 0.;
        for (int gi = 0; gi < groups; ++gi) cb += (double)s_b[(gi * t.lpr + t.l) * W + w], cg += (double)s_g[(gi * t.lpr + t.l) * W + w];
        float* o = a.ws + ((int64_t)blockIdx.x * a.C + c + w) * 2;
        o[0] = (float)cb, o[1] = (float)cg;
      }
    }
    __syncthreads();
  }
}

// ---- backward: dz ----
template <typename Tg, typename Tz, bool VEC>
__global__ __launch_bounds__(kNT) void k_bn_act_bwd(const Tg* __restrict__ g, const Tz* __restrict__ z,
                                                    Tz* __restrict__ dz, Args a) {
  constexpr int W = VEC ? 4 : 1;
  const Where t = where<W>(a);
  const int64_t base = (int64_t)blockIdx.x * t.gpb * kUnroll, total = a.n * a.C;
  const float inv_n = 1.f / (float)a.n;
  int64_t i[kUnroll];
  bool ok[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int64_t iu = base + (int64_t)u * t.gpb + t.g;
    ok[u] = iu < a.n;
    i[u] = ok[u] ? iu : a.n - 1;
  }
  for (int64_t p0 = 0; p0 < t.pieces; p0 += t.lpr) {
    const int64_t p = p0 + t.l;
    const bool on = p < t.pieces;
    const int64_t c = (on ? p : 0) * W;
    float mean[W], invstd[W], gamma[W], beta[W], k1[W], k2[W], s[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      mean[w] = a.mean[c + w], invstd[w] = a.invstd[c + w], gamma[w] = a.gamma[c + w], beta[w] = a.beta[c + w];
      k1[w] = a.training ? a.out0[c + w] * inv_n : 0.f;  // dbeta / n
      k2[w] = a.training ? a.out1[c + w] * inv_n : 0.f;  // dgamma / n
      s[w] = gamma[w] * invstd[w];
    }
    float zv[kUnroll][W], gv[kUnroll][W];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) ld<VEC>(z + i[u] * a.C + c, zv[u]), ld<VEC>(g + i[u] * a.C + c, gv[u]);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      bool keep[W];
      if (a.drop.training) keep_of<VEC>(i[u] * a.C + c, total, a.drop, keep);
      float o[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const float xh = xhat(zv[u][w], mean[w], invstd[w]);
        float gg = gv[u][w];
        if (a.drop.training) gg = keep[w] ? __fmul_rn(gg, a.drop.scale) : 0.f;
        const float ga = act_grad(gg, pre_act(zv[u][w], mean[w], invstd[w], gamma[w], beta[w]), a.act, a.slope);
        o[w] = s[w] * (ga - k1[w] - xh * k2[w]);
      }
      if (ok[u] && on) st<VEC>(dz + i[u] * a.C + c, o);
    }
  }
}

}  // namespace bnact
}  // namespace spp

using namespace spp;
using namespace spp::bnact;

static int64_t slab_count(int64_t n) { return ceil_div(n, (int64_t)kSlab); }

extern "C" int64_t spp_bn_act_slab_rows(void) { return kSlab; }

extern "C" int64_t spp_bn_act_workspace_bytes(int64_t n, int64_t C) {
  if (n < 0 || C < 1) return 16;
  return std::max<int64_t>(16, slab_count(n) * C * 3 * (int64_t)sizeof(float));
}

// what both entries check; fills the kernels' arguments
static spp_status bn_act_common(const char* who, const spp_bn_act_desc* desc, bool backward, Args& a, bool& vec) {
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_bn_act_desc& d = *desc;
  const bool training = d.training != 0;
  SPP_REQUIRE(d.n >= 0, "%s: negative n (%lld)", who, (long long)d.n);
  SPP_REQUIRE(!training || d.n >= 2, "%s: expected more than 1 value per channel when training (n = %lld)", who,
              (long long)d.n);
  SPP_REQUIRE(d.C >= 1 && d.C < (1ll << 31), "%s: C = %lld must be in [1, 2^31)", who, (long long)d.C);
  SPP_REQUIRE(d.p >= 0.f && d.p < 1.f, "%s: the dropout probability p = %g must be in [0, 1)", who, (double)d.p);
  SPP_REQUIRE(d.act == SPP_BN_ACT_NONE || d.act == SPP_BN_ACT_RELU || d.act == SPP_BN_ACT_LEAKY_RELU,
              "%s: unknown activation code %d", who, (int)d.act);
  SPP_REQUIRE(f32_bf16_ok(d.z_elem), "%s: unknown or unsupported element code (z_elem %d)", who, (int)d.z_elem);
  if (backward)
    SPP_REQUIRE(f32_bf16_ok(d.g_elem), "%s: unknown or unsupported element code (g_elem %d)", who, (int)d.g_elem);
  else
    SPP_REQUIRE(f32_bf16_ok(d.y_elem) && (!d.r_dev || f32_bf16_ok(d.r_elem)),
                "%s: unknown or unsupported element code (r_elem %d, y_elem %d)", who, (int)d.r_elem, (int)d.y_elem);
  SPP_REQUIRE(d.z_dev && d.gamma_dev && d.beta_dev && d.mean_dev && d.invstd_dev,
              "%s: NULL buffer (z_dev, gamma_dev, beta_dev, mean_dev or invstd_dev)", who);
  if (backward) {
    SPP_REQUIRE(d.g_dev && d.dz_dev && d.dgamma_dev && d.dbeta_dev, "%s: NULL buffer (g_dev, dz_dev, dgamma_dev or dbeta_dev)",
                who);
  } else {
    SPP_REQUIRE(d.y_dev, "%s: NULL buffer (y_dev)", who);
    SPP_REQUIRE((d.running_mean_dev == nullptr) == (d.running_var_dev == nullptr),
                "%s: running_mean_dev and running_var_dev come together", who);
    SPP_REQUIRE(training || d.running_mean_dev, "%s: NULL buffer (the running statistics, which eval reads)", who);
    SPP_REQUIRE(!(training && d.running_mean_dev && d.momentum < 0.) || d.num_batches_tracked_dev,
                "%s: NULL buffer (num_batches_tracked_dev, which the cumulative average, momentum < 0, reads)", who);
  }
  const bool needs_ws = backward || training;
  if (needs_ws && d.n > 0) {
    const int64_t need = spp_bn_act_workspace_bytes(d.n, d.C);
    SPP_REQUIRE(d.workspace_dev && aligned_to(d.workspace_dev, 16) && d.workspace_bytes >= need,
                "%s: a missing, misaligned or too small workspace (%lld bytes given, %lld needed, 16-byte aligned)", who,
                (long long)d.workspace_bytes, (long long)need);
  }
  SPP_REQUIRE(slab_count(d.n) < (1ll << 31), "%s: too many rows for one launch (n %lld)", who, (long long)d.n);
  const int64_t zb = 4 * elem_bytes(d.z_elem);
  vec = d.C % 4 == 0 && aligned_to(d.z_dev, zb);
  if (backward)
    vec = vec && aligned_to(d.g_dev, 4 * elem_bytes(d.g_elem)) && aligned_to(d.dz_dev, zb);
  else
    vec = vec && aligned_to(d.y_dev, 4 * elem_bytes(d.y_elem)) && (!d.r_dev || aligned_to(d.r_dev, 4 * elem_bytes(d.r_elem)));
  a = Args{};
  a.gamma = d.gamma_dev, a.beta = d.beta_dev, a.mean = d.mean_dev, a.invstd = d.invstd_dev;
  a.running_mean = d.running_mean_dev, a.running_var = d.running_var_dev, a.nbt = d.num_batches_tracked_dev;
  a.out0 = d.dbeta_dev, a.out1 = d.dgamma_dev, a.ws = static_cast<float*>(d.workspace_dev);
  a.n = d.n, a.C = d.C, a.nslabs = slab_count(d.n);
  a.momentum = d.momentum, a.eps = (double)d.eps;
  a.slope = d.negative_slope, a.act = d.act, a.training = training ? 1 : 0;
  a.lpr_log2 = lanes_log2(vec ? d.C / 4 : d.C);
  // p == 0 keeps every element: no generator (its threshold would still drop one element in 2^32)
  a.drop = act_args(d.p, training && d.p > 0.f, d.seed);
  return SPP_OK;
}

static unsigned tile_grid(const Args& a) { return (unsigned)ceil_div(a.n, (int64_t)(kNT >> a.lpr_log2) * kUnroll); }

extern "C" spp_status spp_bn_act_forward(const spp_bn_act_desc* desc, void* stream) {
  const char* who = "spp_bn_act_forward";
  Args a;
  bool vec;
  SPP_TRY(bn_act_common(who, desc, false, a, vec));
  const spp_bn_act_desc& d = *desc;
  if (d.n == 0) return SPP_OK;  // (eval: training refused n < 2)
  hipStream_t st = as_stream(stream);
  if (a.training) {
    with_f32_bf16(d.z_elem, [&](auto tz) {
      using Tz = typename decltype(tz)::type;
      const Tz* z = static_cast<const Tz*>(d.z_dev);
      if (vec) hipLaunchKernelGGL((k_bn_stats<Tz, true>), dim3((unsigned)a.nslabs), dim3(kNT), 0, st, z, a);
      else hipLaunchKernelGGL((k_bn_stats<Tz, false>), dim3((unsigned)a.nslabs), dim3(kNT), 0, st, z, a);
    });
    hipLaunchKernelGGL(k_bn_finalize<true>, dim3((unsigned)ceil_div(a.C, kFinCols)), dim3(kFinCols * kFinLanes), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_bn_eval_stats, dim3((unsigned)ceil_div(a.C, kNT)), dim3(kNT), 0, st, a);
  }
  auto launch = [&](auto tz, auto tr, auto ty, auto v) {
    using Tz = typename decltype(tz)::type;
    using Tr = typename decltype(tr)::type;
    using Ty = typename decltype(ty)::type;
    hipLaunchKernelGGL((k_bn_act_fwd<Tz, Tr, Ty, decltype(v)::value>), dim3(tile_grid(a)), dim3(kNT), 0, st,
                       static_cast<const Tz*>(d.z_dev), static_cast<const Tr*>(d.r_dev), static_cast<Ty*>(d.y_dev), a);
  };
  auto by_vec = [&](auto tz, auto tr, auto ty) {
    vec ? launch(tz, tr, ty, std::true_type{}) : launch(tz, tr, ty, std::false_type{});
  };
  with_f32_bf16(d.z_elem, [&](auto tz) {
    with_f32_bf16(d.y_elem, [&](auto ty) {
      if (!d.r_dev) by_vec(tz, Type<NoRes>{}, ty);
      else with_f32_bf16(d.r_elem, [&](auto tr) { by_vec(tz, tr, ty); });
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_bn_act_backward(const spp_bn_act_desc* desc, void* stream) {
  const char* who = "spp_bn_act_backward";
  Args a;
  bool vec;
  SPP_TRY(bn_act_common(who, desc, true, a, vec));
  const spp_bn_act_desc& d = *desc;
  if (d.n == 0) return SPP_OK;
  hipStream_t st = as_stream(stream);
  auto launch = [&](auto tg, auto tz, auto v) {
    using Tg = typename decltype(tg)::type;
    using Tz = typename decltype(tz)::type;
    constexpr bool V = decltype(v)::value;
    const Tg* g = static_cast<const Tg*>(d.g_dev);
    const Tz* z = static_cast<const Tz*>(d.z_dev);
    hipLaunchKernelGGL((k_bn_bwd_sums<Tg, Tz, V>), dim3((unsigned)a.nslabs), dim3(kNT), 0, st, g, z, a);
    hipLaunchKernelGGL(k_bn_finalize<false>, dim3((unsigned)ceil_div(a.C, kFinCols)), dim3(kFinCols * kFinLanes), 0, st, a);
    hipLaunchKernelGGL((k_bn_act_bwd<Tg, Tz, V>), dim3(tile_grid(a)), dim3(kNT), 0, st, g, z, static_cast<Tz*>(d.dz_dev), a);
  };
  with_f32_bf16(d.g_elem, [&](auto tg) {
    with_f32_bf16(d.z_elem, [&](auto tz) { vec ? launch(tg, tz, std::true_type{}) : launch(tg, tz, std::false_type{}); });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
