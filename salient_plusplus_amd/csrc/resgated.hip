// f4g: the residual gated graph convolution (Bresson & Laurent; PyG's ResGatedGraphConv) over an MFG hop, on rows the
// caller has projected: k [T, D] = lin_key(x_target), q [S, D] = lin_query(x), v [S, D] = lin_value(x),
//     out[i,c]    = sum_{j in row i} s_ij * v[j,c]                  s_ij = sigmoid(k[i,c] + q[j,c])          forward
//     grad_k[i,c] = sum_{j in row i} g[i,c] * v[j,c] * s_ij (1 - s_ij)                                       target side
//     grad_v[j,c] = sum_{i names j}  g[i,c] * s_ij                                                           source side
//     grad_q[j,c] = sum_{i names j}  g[i,c] * v[j,c] * s_ij (1 - s_ij)
// (include/spp.h, spp_resgated_forward / spp_resgated_backward, states the contract.)  Every column stands alone: no
// softmax, no head, no reduction across lanes.  So all three kernels have one shape, ln_act.hip's row mapping: lpr =
// min(64, pow2ceil(D / 4)) lanes own one row, a lane holds NP in {1, 2, 4} pieces of four columns (piece p of lane l is
// piece p * lpr + l of the row: neighbouring lanes read neighbouring 16 bytes), pieces past D / 4 are masked.  The row a
// lane group owns -- k_i (and g_i) of a target, q_j and v_j of a source -- stays in registers while the group walks the
// row's entries, NB of them in flight per round: the index loads first, then the 2 NB NP piece loads back to back, then
// the arithmetic, entry by entry in the walk's order, into fp64 accumulators that are rounded once.  The source side walks the transposed hop (transpose_hop.hip.h),
// whose segments are in ascending CSR position.  Every sum therefore has ONE sequential order that depends on the row
// alone: no atomics, no LDS, no shuffles, no scratch, and the same bits from run to run, whatever the grid and T are.
// The gate is recomputed wherever it is needed: no [E, D] array exists.
#include "elem_io.hip.h"
#include "transpose_hop.hip.h"

#include <algorithm>

namespace spp {
namespace resgated {

constexpr int kNT = 256;
constexpr int kMaxD = 1024;
constexpr int64_t kMaxIndex = (int64_t)1 << 31;

struct Args {
  const int64_t* rowptr;
  const int64_t* col;
  const int32_t* start;  // the transposed hop: source s's targets are tcol[start[s] .. start[s + 1])
  const int32_t* tcol;
  int64_t T, S, E, D;
  int64_t k_stride, q_stride, v_stride;
  int lpr_log2;
  float* out;
  const float* g;
  float* grad_k;
  float* grad_q;
  float* grad_v;
};

// The accumulators are fp64 and are rounded to fp32 once, at the store: a row of 130 entries summed in fp32 in sequence
// stood 10 ulps from the float64 value in one column (1.0e-5 at 8.2, reproduced bit for bit on the host) where torch's
// fp32 index_add_ stood at 3, outside the tests' margin; the fp64 fma costs little beside the gate's expf and division.
struct d4 {
  double x, y, z, w;
};

// expf, not __expf; the forward and both backward kernels call this one function
__device__ __forceinline__ float gate(float k, float q) { return 1.f / (1.f + expf(-(k + q))); }
// acc += s * v
__device__ __forceinline__ void gate_fma(f4 k, f4 q, f4 v, d4& acc) {
  acc.x = fma((double)gate(k.x, q.x), (double)v.x, acc.x), acc.y = fma((double)gate(k.y, q.y), (double)v.y, acc.y);
  acc.z = fma((double)gate(k.z, q.z), (double)v.z, acc.z), acc.w = fma((double)gate(k.w, q.w), (double)v.w, acc.w);
}
// acc += (g * v) * (s * (1 - s)): the gradient of either argument of the gate; the two factors are rounded fp32 products
__device__ __forceinline__ double dgate1(float k, float q, float g, float v, double acc) {
  const float s = gate(k, q);
  return fma((double)__fmul_rn(g, v), (double)__fmul_rn(s, __fsub_rn(1.f, s)), acc);
}
__device__ __forceinline__ void dgate_fma(f4 k, f4 q, f4 g, f4 v, d4& acc) {
  acc.x = dgate1(k.x, q.x, g.x, v.x, acc.x), acc.y = dgate1(k.y, q.y, g.y, v.y, acc.y);
  acc.z = dgate1(k.z, q.z, g.z, v.z, acc.z), acc.w = dgate1(k.w, q.w, g.w, v.w, acc.w);
}

// where this thread works: its row, and which of its pieces lie inside the row (ln_act.hip's Where, one row per group)
template <int NP>
struct Where {
  int64_t row;
  bool on[NP];
  int64_t c[NP];  // first column of piece p (0 for a masked piece: never dereferenced)
};
template <int NP>
__device__ __forceinline__ Where<NP> where(const Args& a) {
  Where<NP> w;
  const int lpr = 1 << a.lpr_log2, l = threadIdx.x & (lpr - 1);
  w.row = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> a.lpr_log2;
  const int pieces = (int)(a.D >> 2);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int i = p * lpr + l;
    w.on[p] = i < pieces;
    w.c[p] = w.on[p] ? (int64_t)i * 4 : 0;
  }
  return w;
}
template <int NP, typename T>
__device__ __forceinline__ void load_row(const T* row, const Where<NP>& w, f4* v) {
#pragma unroll
  for (int p = 0; p < NP; ++p) v[p] = w.on[p] ? load4(row + w.c[p]) : f4{0.f, 0.f, 0.f, 0.f};
}
template <int NP>
__device__ __forceinline__ void store_row(float* row, const Where<NP>& w, const d4* v) {
#pragma unroll
  for (int p = 0; p < NP; ++p)
    if (w.on[p]) store4(row + w.c[p], f4{(float)v[p].x, (float)v[p].y, (float)v[p].z, (float)v[p].w});
}
template <int NP>
__device__ __forceinline__ void zero_row(d4* v) {
#pragma unroll
  for (int p = 0; p < NP; ++p) v[p] = {0., 0., 0., 0.};
}

// The walk all three kernels share: entries [b, e) of `idx`, NB per round and then one at a time; rows(j, x, y) loads the
// two rows entry j names, each(x, y) folds them into the accumulators.  The order of the each() calls is the entries'.
template <int NP, int NB, typename Index, class Rows, class Each>
__device__ __forceinline__ void walk(const Index* __restrict__ idx, int64_t b, int64_t e, Rows&& rows, Each&& each) {
  int64_t i = b;
  for (; i + NB <= e; i += NB) {
    int64_t j[NB];
    f4 x[NB][NP], y[NB][NP];
#pragma unroll
    for (int u = 0; u < NB; ++u) j[u] = idx[i + u];
#pragma unroll
    for (int u = 0; u < NB; ++u) rows(j[u], x[u], y[u]);
#pragma unroll
    for (int u = 0; u < NB; ++u) each(x[u], y[u]);
  }
  for (; i < e; ++i) {
    f4 x[NP], y[NP];
    rows((int64_t)idx[i], x, y);
    each(x, y);
  }
}

// ---- forward: one lane group per target; k_i in registers, q_j and v_j per entry ----
template <typename Tin, int NP, int NB>
__global__ __launch_bounds__(kNT) void k_resgated_fwd(const Tin* __restrict__ k, const Tin* __restrict__ q,
                                                      const Tin* __restrict__ v, Args a) {
  const Where<NP> w = where<NP>(a);
  const int64_t t = w.row;
  if (t >= a.T) return;
  f4 kk[NP];
  d4 acc[NP];
  load_row<NP>(k + t * a.k_stride, w, kk);
  zero_row<NP>(acc);
  walk<NP, NB>(
      a.col, a.rowptr[t], a.rowptr[t + 1],
      [&](int64_t j, f4* qj, f4* vj) {
        load_row<NP>(q + j * a.q_stride, w, qj);
        load_row<NP>(v + j * a.v_stride, w, vj);
      },
      [&](const f4* qj, const f4* vj) {
#pragma unroll
        for (int p = 0; p < NP; ++p) gate_fma(kk[p], qj[p], vj[p], acc[p]);
      });
  store_row<NP>(a.out + t * a.D, w, acc);
}

// ---- backward, target side: the forward's walk with g_i beside k_i; grad_k written ----
template <typename Tin, int NP, int NB>
__global__ __launch_bounds__(kNT) void k_resgated_bwd_target(const Tin* __restrict__ k, const Tin* __restrict__ q,
                                                             const Tin* __restrict__ v, Args a) {
  const Where<NP> w = where<NP>(a);
  const int64_t t = w.row;
  if (t >= a.T) return;
  f4 kk[NP], gg[NP];
  d4 acc[NP];
  load_row<NP>(k + t * a.k_stride, w, kk);
  load_row<NP>(a.g + t * a.D, w, gg);
  zero_row<NP>(acc);
  walk<NP, NB>(
      a.col, a.rowptr[t], a.rowptr[t + 1],
      [&](int64_t j, f4* qj, f4* vj) {
        load_row<NP>(q + j * a.q_stride, w, qj);
        load_row<NP>(v + j * a.v_stride, w, vj);
      },
      [&](const f4* qj, const f4* vj) {
#pragma unroll
        for (int p = 0; p < NP; ++p) dgate_fma(kk[p], qj[p], gg[p], vj[p], acc[p]);
      });
  store_row<NP>(a.grad_k + t * a.D, w, acc);
}

// ---- backward, source side: one lane group per source over its transposed segment; q_j and v_j in registers, k_i and
// g_i per entry; grad_q and grad_v written, zeros for a source no row names ----
template <typename Tin, int NP, int NB>
__global__ __launch_bounds__(kNT) void k_resgated_bwd_source(const Tin* __restrict__ k, const Tin* __restrict__ q,
                                                             const Tin* __restrict__ v, Args a) {
  const Where<NP> w = where<NP>(a);
  const int64_t s = w.row;
  if (s >= a.S) return;
  f4 qq[NP], vv[NP];
  d4 aq[NP], av[NP];
  load_row<NP>(q + s * a.q_stride, w, qq);
  load_row<NP>(v + s * a.v_stride, w, vv);
  zero_row<NP>(aq);
  zero_row<NP>(av);
  walk<NP, NB>(
      a.tcol, a.start[s], a.start[s + 1],
      [&](int64_t i, f4* ki, f4* gi) {
        load_row<NP>(k + i * a.k_stride, w, ki);
        load_row<NP>(a.g + i * a.D, w, gi);
      },
      [&](const f4* ki, const f4* gi) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          gate_fma(ki[p], qq[p], gi[p], av[p]);
          dgate_fma(ki[p], qq[p], gi[p], vv[p], aq[p]);
        }
      });
  store_row<NP>(a.grad_q + s * a.D, w, aq);
  store_row<NP>(a.grad_v + s * a.D, w, av);
}

// fn(Type<Tin>{}, IC<NP>{}, IC<NB>{}): the element type, the pieces a lane holds (three run the four-piece body) and the
// entries in flight, 4, or 2 at NP = 4
template <class Fn>
static void dispatch(int32_t elem, int64_t D, int lpr_log2, Fn&& fn) {
  const int64_t np = ceil_div(D / 4, (int64_t)1 << lpr_log2);
  with_elem(elem, [&](auto tin) {
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I4 = std::integral_constant<int, 4>;
    np == 1 ? fn(tin, I1{}, I4{}) : np == 2 ? fn(tin, I2{}, I4{}) : fn(tin, I4{}, I2{});
  });
}

// What both entries check, in the order include/spp.h documents; *go is false when there is nothing to do (T == 0)
static spp_status check(const char* who, const spp_resgated_desc* desc, bool backward, Args& a, bool* go) {
  *go = false;
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_resgated_desc& d = *desc;
  const int64_t T = d.num_targets, S = d.num_sources, E = d.num_edges, D = d.D;
  SPP_REQUIRE(elem_ok(d.x_elem), "%s: unknown or unsupported element code %d (fp32, fp16 or bf16 rows)", who, (int)d.x_elem);
  SPP_REQUIRE(D >= 4 && D <= kMaxD && D % 4 == 0,
              "%s: D = %lld must be a multiple of 4 in [4, %d] (four columns per lane, no scalar form)", who, (long long)D,
              kMaxD);
  SPP_REQUIRE(T >= 0 && S >= T && E >= 0, "%s: bad sizes (T %lld, S %lld, E %lld; needs 0 <= T <= S, E >= 0)", who,
              (long long)T, (long long)S, (long long)E);
  SPP_REQUIRE(S < kMaxIndex && E < kMaxIndex, "%s: S or E beyond 2^31 (one launch; the transposed hop has 32-bit indices)",
              who);
  if (T == 0) return SPP_OK;  // nothing to do: no pointer is looked at
  SPP_REQUIRE(d.k_stride_elems >= D && d.q_stride_elems >= D && d.v_stride_elems >= D && d.k_stride_elems % 4 == 0 &&
                  d.q_stride_elems % 4 == 0 && d.v_stride_elems % 4 == 0,
              "%s: a row stride is smaller than D or not a multiple of 4 elements", who);
  SPP_REQUIRE(d.rowptr_dev && (d.col_dev || E == 0) && d.k_dev && d.q_dev && d.v_dev, "%s: NULL buffer (rowptr, col, k, q or v)",
              who);
  const bool sources = d.grad_q_dev != nullptr;
  if (backward) {
    SPP_REQUIRE(d.grad_out_dev && d.grad_k_dev, "%s: NULL buffer (grad_out or grad_k)", who);
    SPP_REQUIRE((d.grad_q_dev == nullptr) == (d.grad_v_dev == nullptr),
                "%s: grad_q and grad_v are wanted together or not at all (one of them is NULL)", who);
    SPP_REQUIRE(!sources || d.workspace_dev, "%s: missing workspace (spp_resgated_workspace_bytes)", who);
  } else {
    SPP_REQUIRE(d.out_dev, "%s: NULL buffer (out)", who);
  }
  const int64_t rb = 4 * elem_bytes(d.x_elem);
  SPP_REQUIRE(aligned_to(d.k_dev, rb) && aligned_to(d.q_dev, rb) && aligned_to(d.v_dev, rb) && aligned_to(d.rowptr_dev, 8) &&
                  aligned_to(d.col_dev, 8),
              "%s: misaligned buffer (rows of k, q, v: 4 elements; rowptr, col: 8 bytes)", who);
  if (backward) {
    SPP_REQUIRE(aligned_to(d.grad_out_dev, 16) && aligned_to(d.grad_k_dev, 16) && aligned_to(d.grad_q_dev, 16) &&
                    aligned_to(d.grad_v_dev, 16),
                "%s: misaligned buffer (grad_out, grad_k, grad_q, grad_v: 16 bytes)", who);
    SPP_REQUIRE(!sources || (aligned_to(d.workspace_dev, 16) && d.workspace_bytes >= transpose_hop_bytes(T, S, E, false)),
                "%s: misaligned or too small workspace (spp_resgated_workspace_bytes, 16-byte aligned)", who);
  } else {
    SPP_REQUIRE(aligned_to(d.out_dev, 16), "%s: misaligned buffer (out: 16 bytes)", who);
  }
  a = Args{};
  a.rowptr = d.rowptr_dev, a.col = d.col_dev;
  a.T = T, a.S = S, a.E = E, a.D = D;
  a.k_stride = d.k_stride_elems, a.q_stride = d.q_stride_elems, a.v_stride = d.v_stride_elems;
  a.lpr_log2 = lanes_log2(D / 4);
  a.out = d.out_dev, a.g = d.grad_out_dev, a.grad_k = d.grad_k_dev, a.grad_q = d.grad_q_dev, a.grad_v = d.grad_v_dev;
  *go = true;
  return SPP_OK;
}

static unsigned grid_of(int64_t rows, int lpr_log2) { return (unsigned)ceil_div(rows << lpr_log2, kNT); }  // < 2^31 * 64 / 256

}  // namespace resgated
}  // namespace spp

using namespace spp;
using namespace spp::resgated;

#define SPP_RESGATED_LAUNCH(kernel, rows)                                                                                \
  dispatch(d.x_elem, a.D, a.lpr_log2, [&](auto tin, auto np, auto nb) {                                                  \
    using Tin = typename decltype(tin)::type;                                                                            \
    hipLaunchKernelGGL((kernel<Tin, decltype(np)::value, decltype(nb)::value>), dim3(grid_of(rows, a.lpr_log2)),         \
                       dim3(kNT), 0, st, static_cast<const Tin*>(d.k_dev), static_cast<const Tin*>(d.q_dev),             \
                       static_cast<const Tin*>(d.v_dev), a);                                                             \
  })

extern "C" int64_t spp_resgated_workspace_bytes(int64_t num_targets, int64_t num_sources, int64_t num_edges) {
  if (num_targets < 0 || num_sources < num_targets || num_edges < 0 || num_sources >= kMaxIndex || num_edges >= kMaxIndex)
    return -1;
  return transpose_hop_bytes(num_targets, num_sources, num_edges, false);
}

extern "C" spp_status spp_resgated_forward(const spp_resgated_desc* desc, void* stream) {
  const char* who = "spp_resgated_forward";
  Args a;
  bool go;
  SPP_TRY(check(who, desc, false, a, &go));
  if (!go) return SPP_OK;
  const spp_resgated_desc& d = *desc;
  hipStream_t st = as_stream(stream);
  SPP_RESGATED_LAUNCH(k_resgated_fwd, a.T);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_resgated_backward(const spp_resgated_desc* desc, void* stream) {
  const char* who = "spp_resgated_backward";
  Args a;
  bool go;
  SPP_TRY(check(who, desc, true, a, &go));
  if (!go) return SPP_OK;
  const spp_resgated_desc& d = *desc;
  hipStream_t st = as_stream(stream);
  SPP_RESGATED_LAUNCH(k_resgated_bwd_target, a.T);
  if (a.grad_q) {
    TransposedHop hop{};
    SPP_TRY(transpose_hop(d.rowptr_dev, d.col_dev, a.T, a.S, a.E, false, d.workspace_dev, d.workspace_bytes, st, &hop));
    a.start = hop.start, a.tcol = hop.tcol;
    SPP_RESGATED_LAUNCH(k_resgated_bwd_source, a.S);
  }
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
