// f4f: the LayerNorm tail between the layers of the attention models (GAT, GATv2, GraphTransformer with norm="layer"),
//     y = dropout(act(LayerNorm(z))) [+ r]      per-row statistics, forward and backward
// (include/spp.h, spp_ln_act_forward / spp_ln_act_backward, states the contract; bn_act.hip is the BatchNorm relative,
// whose statistics run down the columns and therefore need kernels of another shape).
//
// Shape, both kernels: lpr = min(64, pow2ceil(C / 4)) lanes own one row, each lane holds NP in {1, 2, 4} pieces of four
// columns (piece k of lane l is piece k * lpr + l of the row: neighbouring lanes read neighbouring 16 bytes), pieces past
// C / 4 hold zeros and are masked out; a workgroup's 256 / lpr lane groups take different rows.  At C = 256 one wave holds
// a row in one piece a lane; at C = 1024 one wave holds a row in four.  Row sums go through an xor butterfly over the
// lane group (every lane ends with the same bits, in an order that depends on C alone).
//   k_ln_act_fwd       one row per lane group: z is read ONCE and stays in registers; the mean is the butterfly's sum
//                      over C plus the (tiny) mean of the residuals z - mean0, the variance the sum of the squared
//                      residuals about that mean -- a two-pass variance at the cost of one read; then the tail from the
//                      registers and the stores of y, mean, rstd.  No LDS, no atomics: a row's result depends on the row
//                      and C only
//   k_ln_act_bwd       one workgroup per slab of kSlab rows, a lane group walks rows g, g + gpb, ... of its slab: per
//                      row two sums (gh, gh * xh) through the butterfly, dz written; every lane keeps its own columns'
//                      sums of g_a and g_a * xh in registers across its rows, in fp64; at the end of the slab the lane
//                      groups meet in LDS once, in lane-group order, and the slab's [2, C] fp32 record (each sum rounded
//                      once) goes to the workspace
//   k_ln_act_finalize  4 columns x 64 slab lanes per workgroup: lane j folds slabs j, j + 64, ... in that order, the 64
//                      lanes meet in LDS in lane order; fp64; writes dgamma and dbeta
// No atomics, no scratch, every offset 64-bit.  There is no scalar form: C % 4 == 0, 4 <= C <= 1024.
#include "act_keep.hip.h"
#include "elem_io.hip.h"

#include <algorithm>

namespace spp {
namespace lnact {

constexpr int kNT = 256;
constexpr int kSlab = SPP_LN_ACT_SLAB_ROWS;  // rows per backward slab
constexpr int kFinCols = 4, kFinLanes = 64;  // many slabs, few columns: the slab walk is the long axis
constexpr int kMaxC = 1024;

struct NoRes {};  // the residual's element type when there is none

struct Args {
  const float* gamma;
  const float* beta;
  float* mean;
  float* rstd;
  float* dgamma;
  float* dbeta;
  float* ws;  // [nslabs, 2, C]: per slab the column sums of g_a (dbeta), then of g_a * xh (dgamma)
  int64_t n, C, nslabs;
  float eps, slope;
  int32_t act;
  int lpr_log2;
  ActArgs drop;  // drop.training: dropout is applied (training and p > 0)
};

// the contract's expressions, shared by forward and backward so that the sign of u is the same in both
__device__ __forceinline__ float xhat(float z, float mean, float rstd) { return __fmul_rn(__fsub_rn(z, mean), rstd); }
// u = gamma * (z - mean) * rstd + beta of the fp32 operands, rounded ONCE (to within the second-order terms dropped
// below) instead of three times: every fp32 operation's rounding error is recovered exactly (the two-sum of z - mean and
// of t + beta, the fma residuals of the two products) and added back before the last rounding.  fp32 arithmetic only;
// the intrinsics keep the compiler from contracting the error terms away.  (bn_act.hip's pre_act, with rstd per row.)
__device__ __forceinline__ float pre_act(float z, float mean, float rstd, float gamma, float beta) {
  const float pa = __fmul_rn(gamma, rstd), ea = fmaf(gamma, rstd, -pa);  // gamma * rstd = pa + ea
  const float dh = __fsub_rn(z, mean), bd = __fsub_rn(dh, z);
  const float dl = __fadd_rn(__fsub_rn(z, __fsub_rn(dh, bd)), __fsub_rn(-mean, bd));  // z - mean = dh + dl
  const float t = __fmul_rn(dh, pa), et = fmaf(dh, pa, -t);                             // dh * pa = t + et
  const float corr = __fadd_rn(et, fmaf(dh, ea, __fmul_rn(dl, pa)));
  const float sh = __fadd_rn(t, beta), bs = __fsub_rn(sh, t);
  const float sl = __fadd_rn(__fsub_rn(t, __fsub_rn(sh, bs)), __fsub_rn(beta, bs));      // t + beta = sh + sl
  return __fadd_rn(sh, __fadd_rn(sl, corr));
}
__device__ __forceinline__ float act_of(float u, int act, float slope) {
  return (u > 0.f || act == SPP_LN_ACT_NONE) ? u : act == SPP_LN_ACT_RELU ? 0.f : __fmul_rn(slope, u);
}
// g * act'(u)
__device__ __forceinline__ float act_grad(float g, float u, int act, float slope) {
  return (u > 0.f || act == SPP_LN_ACT_NONE) ? g : act == SPP_LN_ACT_RELU ? 0.f : __fmul_rn(slope, g);
}

// the sum of v over the lpr lanes of a lane group, the same bits in every lane: partner distances lpr / 2, ..., 1
__device__ __forceinline__ float group_sum(float v, int lpr) {
  for (int m = lpr >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// where this thread works: its lane group, its lane in the row, which of its pieces lie inside the row
template <int NP>
struct Where {
  int lpr, gpb, g, l;
  bool on[NP];
  int64_t c[NP];  // first column of piece k (0 for a masked piece: never dereferenced)
};
template <int NP>
__device__ __forceinline__ Where<NP> where(const Args& a) {
  Where<NP> w;
  w.lpr = 1 << a.lpr_log2, w.gpb = kNT >> a.lpr_log2;
  w.g = threadIdx.x >> a.lpr_log2, w.l = threadIdx.x & (w.lpr - 1);
  const int pieces = (int)(a.C >> 2);
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int p = k * w.lpr + w.l;
    w.on[k] = p < pieces;
    w.c[k] = w.on[k] ? (int64_t)p * 4 : 0;
  }
  return w;
}

template <int NP, typename T>
__device__ __forceinline__ void load_row(const T* row, const Where<NP>& t, f4* v) {
#pragma unroll
  for (int k = 0; k < NP; ++k) v[k] = t.on[k] ? load4(row + t.c[k]) : f4{0.f, 0.f, 0.f, 0.f};
}
template <int NP>
__device__ __forceinline__ void load_row(const NoRes*, const Where<NP>&, f4*) {}

// ---- forward: one row per lane group ----
template <typename Tz, typename Tr, typename Ty, int NP>
__global__ __launch_bounds__(kNT) void k_ln_act_fwd(const Tz* __restrict__ z, const Tr* __restrict__ r,
                                                    Ty* __restrict__ y, Args a) {
  constexpr bool kRes = !std::is_same<Tr, NoRes>::value;
  const Where<NP> t = where<NP>(a);
  const int64_t iu = (int64_t)blockIdx.x * t.gpb + t.g;
  const bool ok = iu < a.n;
  const int64_t i = ok ? iu : a.n - 1;  // (clamped: loaded, never stored; the butterfly needs every lane)
  f4 zv[NP], rv[NP], ga[NP], be[NP];
  load_row<NP>(z + i * a.C, t, zv);
  if constexpr (kRes) load_row<NP>(r + i * a.C, t, rv);
  load_row<NP>(a.gamma, t, ga);
  load_row<NP>(a.beta, t, be);
  const float fC = (float)a.C;
  // mean0: the plain sum; masked pieces add zeros
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NP; ++k) s += (zv[k].x + zv[k].y) + (zv[k].z + zv[k].w);
  const float mean0 = group_sum(s, t.lpr) / fC;
  // residuals about mean0: their sum corrects the mean's rounding, their squares give the variance (shifted exactly:
  // sum (z - mean)^2 = sum d^2 - (sum d)^2 / C for d = z - mean0)
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    if (t.on[k]) {
      const float d0 = zv[k].x - mean0, d1 = zv[k].y - mean0, d2 = zv[k].z - mean0, d3 = zv[k].w - mean0;
      s1 += (d0 + d1) + (d2 + d3);
      s2 += fmaf(d0, d0, d1 * d1) + fmaf(d2, d2, d3 * d3);
    }
  }
  s1 = group_sum(s1, t.lpr), s2 = group_sum(s2, t.lpr);
  const float dm = s1 / fC;
  const float mean = mean0 + dm;
  const float var = fmaxf(fmaf(-s1, dm, s2), 0.f) / fC;
  // rstd = 1 / sqrt(var + eps): correctly rounded sqrt and divide, then one Newton step on the residual 1 - v * r0^2,
  // which is formed without a rounding of its own (v * r0 = h + eh exactly)
  const float v = var + a.eps;
  const float r0 = 1.f / sqrtf(v);
  const float h = __fmul_rn(v, r0), eh = fmaf(v, r0, -h);
  const float rstd = fmaf(0.5f * r0, fmaf(-eh, r0, fmaf(-h, r0, 1.f)), r0);
  const int64_t e0 = i * a.C;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    if (!t.on[k]) continue;
    Keep4 kp{true, true, true, true};
    if (a.drop.training) kp = keep4((e0 + t.c[k]) >> 2, a.drop);  // (a kernel argument: a scalar branch)
    const float zz[4] = {zv[k].x, zv[k].y, zv[k].z, zv[k].w};
    const float gg[4] = {ga[k].x, ga[k].y, ga[k].z, ga[k].w};
    const float bb[4] = {be[k].x, be[k].y, be[k].z, be[k].w};
    const bool kk[4] = {kp.x, kp.y, kp.z, kp.w};
    float o[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float vv = act_of(pre_act(zz[w], mean, rstd, gg[w], bb[w]), a.act, a.slope);
      if (a.drop.training) vv = kk[w] ? __fmul_rn(vv, a.drop.scale) : 0.f;
      o[w] = vv;
    }
    if constexpr (kRes) {
      o[0] = __fadd_rn(o[0], rv[k].x), o[1] = __fadd_rn(o[1], rv[k].y);
      o[2] = __fadd_rn(o[2], rv[k].z), o[3] = __fadd_rn(o[3], rv[k].w);
    }
    if (ok) store4(y + e0 + t.c[k], f4{o[0], o[1], o[2], o[3]});
  }
  if (ok && t.l == 0) a.mean[i] = mean, a.rstd[i] = rstd;
}

// ---- backward: dz per row, and per slab the column sums of g_a and g_a * xh ----
template <typename Tg, typename Tz, int NP>
__global__ __launch_bounds__(kNT) void k_ln_act_bwd(const Tg* __restrict__ g, const Tz* __restrict__ z,
                                                    Tz* __restrict__ dz, Args a) {
  __shared__ double s_b[NP][kNT * 4], s_g[NP][kNT * 4];
  const Where<NP> t = where<NP>(a);
  const int64_t row0 = (int64_t)blockIdx.x * kSlab;
  const int rows = (int)std::min<int64_t>(kSlab, a.n - row0);  // >= 1: the grid is the slab count
  const float inv_C = 1.f / (float)a.C;
  f4 ga[NP], be[NP];
  load_row<NP>(a.gamma, t, ga);
  load_row<NP>(a.beta, t, be);
  double sb[NP][4], sg[NP][4];  // fp64: a column's sum is rounded to fp32 once per slab, in its record
#pragma unroll
  for (int k = 0; k < NP; ++k)
#pragma unroll
    for (int w = 0; w < 4; ++w) sb[k][w] = 0., sg[k][w] = 0.;
  // (workgroup-uniform trip count; a lane group past its last row works on a clamped row and neither stores nor adds)
  for (int il0 = 0; il0 < rows; il0 += t.gpb) {
    const int il = il0 + t.g;
    const bool ok = il < rows;
    const int64_t i = row0 + (ok ? il : rows - 1);
    f4 zv[NP], gv[NP];
    load_row<NP>(z + i * a.C, t, zv);
    load_row<NP>(g + i * a.C, t, gv);
    const float mean = a.mean[i], rstd = a.rstd[i];
    const int64_t e0 = i * a.C;
    float gh[NP][4], xh[NP][4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      Keep4 kp{true, true, true, true};
      if (a.drop.training) kp = keep4((e0 + t.c[k]) >> 2, a.drop);
      const float zz[4] = {zv[k].x, zv[k].y, zv[k].z, zv[k].w};
      const float gi[4] = {gv[k].x, gv[k].y, gv[k].z, gv[k].w};
      const float gm[4] = {ga[k].x, ga[k].y, ga[k].z, ga[k].w};
      const float bb[4] = {be[k].x, be[k].y, be[k].z, be[k].w};
      const bool kk[4] = {kp.x, kp.y, kp.z, kp.w};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        xh[k][w] = xhat(zz[w], mean, rstd);
        float gg = gi[w];
        if (a.drop.training) gg = kk[w] ? __fmul_rn(gg, a.drop.scale) : 0.f;
        float gact = act_grad(gg, pre_act(zz[w], mean, rstd, gm[w], bb[w]), a.act, a.slope);
        if (!t.on[k]) gact = 0.f, xh[k][w] = 0.f;  // masked pieces: z = g = gamma = 0, and mean must not leak in
        gh[k][w] = gact * gm[w];
        s1 += gh[k][w];
        s2 = fmaf(gh[k][w], xh[k][w], s2);
        if (ok) {
          sb[k][w] += (double)gact;
          sg[k][w] = fma((double)gact, (double)xh[k][w], sg[k][w]);
        }
      }
    }
    s1 = group_sum(s1, t.lpr) * inv_C, s2 = group_sum(s2, t.lpr) * inv_C;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      float o[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) o[w] = rstd * ((gh[k][w] - s1) - xh[k][w] * s2);
      if (ok && t.on[k]) store4(dz + e0 + t.c[k], f4{o[0], o[1], o[2], o[3]});
    }
  }
  // the lane groups meet once: lane group 0 adds the groups' partial sums of its columns in lane-group order
#pragma unroll
  for (int k = 0; k < NP; ++k)
#pragma unroll
    for (int w = 0; w < 4; ++w) s_b[k][threadIdx.x * 4 + w] = sb[k][w], s_g[k][threadIdx.x * 4 + w] = sg[k][w];
  __syncthreads();
  if (t.g != 0) return;
  const int groups = rows < t.gpb ? rows : t.gpb;  // the other lane groups hold zeros
  float* rec = a.ws + (int64_t)blockIdx.x * 2 * a.C;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    if (!t.on[k]) continue;
    double cb[4] = {0., 0., 0., 0.}, cg[4] = {0., 0., 0., 0.};
    for (int gi = 0; gi < groups; ++gi) {
#pragma unroll
      for (int w = 0; w < 4; ++w) cb[w] += s_b[k][(gi * t.lpr + t.l) * 4 + w], cg[w] += s_g[k][(gi * t.lpr + t.l) * 4 + w];
    }
    store4(rec + t.c[k], f4{(float)cb[0], (float)cb[1], (float)cb[2], (float)cb[3]});
    store4(rec + a.C + t.c[k], f4{(float)cg[0], (float)cg[1], (float)cg[2], (float)cg[3]});
  }
}

// ---- the slabs' [2, C] records to dbeta and dgamma, in a fixed order, fp64 ----
__global__ __launch_bounds__(kFinCols* kFinLanes) void k_ln_act_finalize(Args a) {
  __shared__ double s_a[kFinCols * kFinLanes], s_b[kFinCols * kFinLanes];
  const int cl = threadIdx.x % kFinCols, j = threadIdx.x / kFinCols;
  const int64_t col = (int64_t)blockIdx.x * kFinCols + cl;  // C % 4 == 0: always inside
  double ca = 0., cb = 0.;
  for (int64_t s = j; s < a.nslabs; s += kFinLanes) {
    const float* rec = a.ws + s * 2 * a.C;
    ca += (double)rec[col], cb += (double)rec[a.C + col];
  }
  s_a[threadIdx.x] = ca, s_b[threadIdx.x] = cb;
  __syncthreads();
  if (j != 0) return;
  for (int k = 1; k < kFinLanes; ++k) ca += s_a[k * kFinCols + cl], cb += s_b[k * kFinCols + cl];
  a.dbeta[col] = (float)ca;
  a.dgamma[col] = (float)cb;
}

}  // namespace lnact
}  // namespace spp

using namespace spp;
using namespace spp::lnact;

static int64_t slab_count(int64_t n) { return ceil_div(n, (int64_t)kSlab); }

extern "C" int64_t spp_ln_act_slab_rows(void) { return kSlab; }

extern "C" int64_t spp_ln_act_workspace_bytes(int64_t n, int64_t C) {
  if (n < 0 || C < 1) return 16;
  return std::max<int64_t>(16, slab_count(n) * C * 2 * (int64_t)sizeof(float));
}

// what both entries check; fills the kernels' arguments
static spp_status ln_act_common(const char* who, const spp_ln_act_desc* desc, bool backward, Args& a) {
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_ln_act_desc& d = *desc;
  SPP_REQUIRE(d.n >= 0, "%s: negative n (%lld)", who, (long long)d.n);
  SPP_REQUIRE(f32_bf16_ok(d.z_elem), "%s: unknown or unsupported element code (z_elem %d)", who, (int)d.z_elem);
  if (backward)
    SPP_REQUIRE(f32_bf16_ok(d.g_elem), "%s: unknown or unsupported element code (g_elem %d)", who, (int)d.g_elem);
  else
    SPP_REQUIRE(f32_bf16_ok(d.y_elem) && (!d.r_dev || f32_bf16_ok(d.r_elem)),
                "%s: unknown or unsupported element code (r_elem %d, y_elem %d)", who, (int)d.r_elem, (int)d.y_elem);
  SPP_REQUIRE(d.act == SPP_LN_ACT_NONE || d.act == SPP_LN_ACT_RELU || d.act == SPP_LN_ACT_LEAKY_RELU,
              "%s: unknown activation code %d", who, (int)d.act);
  SPP_REQUIRE(d.C >= 4 && d.C <= kMaxC && d.C % 4 == 0,
              "%s: C = %lld must be a multiple of 4 in [4, %d] (four columns per lane, no scalar form)", who,
              (long long)d.C, kMaxC);
  if (d.n == 0) {  // nothing to do: no buffer is looked at (an empty tensor has no address)
    a = Args{};
    return SPP_OK;
  }
  const int64_t zb = 4 * elem_bytes(d.z_elem);
  bool al = aligned_to(d.z_dev, zb) && aligned_to(d.gamma_dev, 16) && aligned_to(d.beta_dev, 16);
  if (backward)
    al = al && aligned_to(d.g_dev, 4 * elem_bytes(d.g_elem)) && aligned_to(d.dz_dev, zb) &&
         aligned_to(d.dgamma_dev, 4) && aligned_to(d.dbeta_dev, 4);
  else
    al = al && aligned_to(d.y_dev, 4 * elem_bytes(d.y_elem)) && (!d.r_dev || aligned_to(d.r_dev, 4 * elem_bytes(d.r_elem)));
  SPP_REQUIRE(al, "%s: a misaligned buffer (every matrix base to 4 of its elements, gamma_dev and beta_dev to 16 bytes)", who);
  SPP_REQUIRE(d.z_dev && d.gamma_dev && d.beta_dev && d.mean_dev && d.rstd_dev,
              "%s: NULL buffer (z_dev, gamma_dev, beta_dev, mean_dev or rstd_dev)", who);
  if (backward)
    SPP_REQUIRE(d.g_dev && d.dz_dev && d.dgamma_dev && d.dbeta_dev, "%s: NULL buffer (g_dev, dz_dev, dgamma_dev or dbeta_dev)",
                who);
  else
    SPP_REQUIRE(d.y_dev, "%s: NULL buffer (y_dev)", who);
  SPP_REQUIRE(d.p >= 0.f && d.p < 1.f, "%s: the dropout probability p = %g must be in [0, 1)", who, (double)d.p);
  const bool drop = d.training != 0 && d.p > 0.f;  // eval or p == 0: no generator, the kernels read neither p nor the seed
  if (backward) {
    const int64_t need = spp_ln_act_workspace_bytes(d.n, d.C);
    SPP_REQUIRE(d.workspace_dev && aligned_to(d.workspace_dev, 16) && d.workspace_bytes >= need,
                "%s: a missing, misaligned or too small workspace (%lld bytes given, %lld needed, 16-byte aligned)", who,
                (long long)d.workspace_bytes, (long long)need);
  }
  a = Args{};
  a.lpr_log2 = lanes_log2(d.C / 4);
  SPP_REQUIRE(ceil_div(d.n, (int64_t)(kNT >> a.lpr_log2)) < (1ll << 31), "%s: too many rows for one launch (n %lld)", who,
              (long long)d.n);
  a.gamma = d.gamma_dev, a.beta = d.beta_dev, a.mean = d.mean_dev, a.rstd = d.rstd_dev;
  a.dgamma = d.dgamma_dev, a.dbeta = d.dbeta_dev, a.ws = static_cast<float*>(d.workspace_dev);
  a.n = d.n, a.C = d.C, a.nslabs = slab_count(d.n);
  a.eps = d.eps, a.slope = d.negative_slope, a.act = d.act;
  a.drop = act_args(drop ? d.p : 0.f, drop, drop ? d.seed : 0);
  return SPP_OK;
}

// fn(std::integral_constant<int, NP>{}): the pieces a lane holds, 1, 2 or 4 (three pieces run the four-piece kernel)
template <class Fn>
static void with_pieces(const Args& a, Fn&& fn) {
  const int64_t np = ceil_div(a.C / 4, (int64_t)1 << a.lpr_log2);
  np == 1 ? fn(std::integral_constant<int, 1>{}) : np == 2 ? fn(std::integral_constant<int, 2>{})
                                                            : fn(std::integral_constant<int, 4>{});
}

extern "C" spp_status spp_ln_act_forward(const spp_ln_act_desc* desc, void* stream) {
  const char* who = "spp_ln_act_forward";
  Args a;
  SPP_TRY(ln_act_common(who, desc, false, a));
  const spp_ln_act_desc& d = *desc;
  if (d.n == 0) return SPP_OK;
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)ceil_div(a.n, (int64_t)(kNT >> a.lpr_log2));
  auto launch = [&](auto tz, auto tr, auto ty) {
    using Tz = typename decltype(tz)::type;
    using Tr = typename decltype(tr)::type;
    using Ty = typename decltype(ty)::type;
    with_pieces(a, [&](auto np) {
      hipLaunchKernelGGL((k_ln_act_fwd<Tz, Tr, Ty, decltype(np)::value>), dim3(grid), dim3(kNT), 0, st,
                         static_cast<const Tz*>(d.z_dev), static_cast<const Tr*>(d.r_dev), static_cast<Ty*>(d.y_dev), a);
    });
  };
  with_f32_bf16(d.z_elem, [&](auto tz) {
    with_f32_bf16(d.y_elem, [&](auto ty) {
      if (!d.r_dev) launch(tz, Type<NoRes>{}, ty);
      else with_f32_bf16(d.r_elem, [&](auto tr) { launch(tz, tr, ty); });
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_ln_act_backward(const spp_ln_act_desc* desc, void* stream) {
  const char* who = "spp_ln_act_backward";
  Args a;
  SPP_TRY(ln_act_common(who, desc, true, a));
  const spp_ln_act_desc& d = *desc;
  if (d.n == 0) return SPP_OK;
  hipStream_t st = as_stream(stream);
  with_f32_bf16(d.g_elem, [&](auto tg) {
    with_f32_bf16(d.z_elem, [&](auto tz) {
      using Tg = typename decltype(tg)::type;
      using Tz = typename decltype(tz)::type;
      with_pieces(a, [&](auto np) {
        hipLaunchKernelGGL((k_ln_act_bwd<Tg, Tz, decltype(np)::value>), dim3((unsigned)a.nslabs), dim3(kNT), 0, st,
                           static_cast<const Tg*>(d.g_dev), static_cast<const Tz*>(d.z_dev), static_cast<Tz*>(d.dz_dev), a);
      });
    });
  });
  hipLaunchKernelGGL(k_ln_act_finalize, dim3((unsigned)(a.C / kFinCols)), dim3(kFinCols * kFinLanes), 0, st, a);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
