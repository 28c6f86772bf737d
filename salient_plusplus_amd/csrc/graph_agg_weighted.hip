// f3s: EDGE-WEIGHTED sum aggregation over rows of the RESIDENT graph's CSR -- the message passing of exact, layer-wise
// GCN inference, the weighted member of graph_aggregate.hip's family:
//     out[i,:] = sum_{k in [rowptr[t], rowptr[t+1])} c_k * x[col[k],:]  (+ self_c * x[t,:], last),   t = target_row0 + i  or  target_ids[i]
// The weights are explicit (c_k = w[k], or 1 without w; self_c = self_w[t]) or formed here from one fp32 value per NODE,
//     c_k = dinv[t] * (w ? w[k] : 1.f) * dinv[col[k]],   self_c = dinv[t] * fill * dinv[t]
// -- k_gcn_coef's fp32 expressions (aggregate_weighted.hip), token for token: two multiplications left to right, nothing
// for the compiler to contract or reassociate, so the bits of spp_gcn_norm's coefficients without its [E] array.
//
// Summation contract (include/spp.h, spp_graph_agg_weighted_forward): C = kGraphChunk.  A row of d <= C entries is one
// fmaf per entry in CSR order on an accumulator that starts at 0, the self term last: k_agg_w_fwd's arithmetic.  A longer
// row is consecutive chunks of C entries, each such a chain from zero, the chunk sums added in chunk order and the self
// term applied as one fmaf on the total.  Nothing else enters: not the grid, not the slab, not the other rows.
//
// The shape is graph_aggregate.hip's: k_graph_aggw_rows, lpr lanes per target, finishes the rows of d <= C and lists the
// longer ones in the workspace; k_graph_aggw_long, one workgroup per listed row, sums 256 / lpr chunks at a time through
// LDS with the double-buffered barrier scheme.  Four rows are in flight per lane, as in sum_entries; per entry a lane
// group streams 8 bytes of col and 4 of w, or gathers 4 of dinv, next to F * s bytes of row.  Every offset is 64-bit.
#include "graph_rows.hip.h"

namespace spp {
namespace graph_agg_w {

using namespace graph_rows;

struct Args : Targets {
  const float* w;       // one per entry of col, or NULL
  const float* dinv;    // [x_rows] (kDinv kernels)
  const float* self_w;  // [x_rows] by global node id, or NULL (never with dinv)
  float fill;           // kDinv kernels: 0, 1 or 2
  int lpr_log2;
  LongRows long_rows;
};

// row g of the full matrix; an id outside [0, x_rows) reads row 0 (the rule of graph_aggregate.hip's NodeRows)
template <typename Tin>
struct NodeRows {
  const Tin* x;
  int64_t stride, rows;
  __device__ __forceinline__ NodeRows(const Tin* src, const Args& a) : x(src), stride(a.x_stride), rows(a.x_rows) {}
  __device__ __forceinline__ const Tin* operator()(int64_t g) const {
    return x + ((uint64_t)g < (uint64_t)rows ? g : 0) * stride;
  }
};

// the weight of entry k, whose source is node j, in the row of a target whose dinv is dt
template <bool kW, bool kDinv>
struct Coef {
  const float* __restrict__ w;
  const float* __restrict__ dinv;
  int64_t rows;
  float dt;
  __device__ __forceinline__ float operator()(int64_t k, int64_t j) const {
    if constexpr (kDinv) {
      const float ds = dinv[(uint64_t)j < (uint64_t)rows ? j : 0];
      return dt * (kW ? w[k] : 1.f) * ds;  // (k_gcn_coef's expression)
    } else {
      return kW ? w[k] : 1.f;
    }
  }
};

// columns c.. of the entries [b, e): one fmaf per entry in CSR order from zero; four rows are in flight
template <typename Tin, bool VEC4, class Cf>
__device__ __forceinline__ typename Piece<VEC4>::type fma_entries(const NodeRows<Tin>& row, const int64_t* __restrict__ col,
                                                                  const Cf& coef, int64_t b, int64_t e, int64_t c) {
  using P = Piece<VEC4>;
  typename P::type acc = P::zero();
  int64_t k = b;
  for (; k + 3 < e; k += 4) {
    const int64_t j0 = col[k], j1 = col[k + 1], j2 = col[k + 2], j3 = col[k + 3];
    const float c0 = coef(k, j0), c1 = coef(k + 1, j1), c2 = coef(k + 2, j2), c3 = coef(k + 3, j3);
    const auto v0 = P::load(row(j0) + c), v1 = P::load(row(j1) + c), v2 = P::load(row(j2) + c), v3 = P::load(row(j3) + c);
    acc = P::fma(c0, v0, acc);
    acc = P::fma(c1, v1, acc);
    acc = P::fma(c2, v2, acc);
    acc = P::fma(c3, v3, acc);
  }
  for (; k < e; ++k) {
    const int64_t j = col[k];
    acc = P::fma(coef(k, j), P::load(row(j) + c), acc);
  }
  return acc;
}

// the self term, last, and the store: columns c.. of output row o (own: node t's row of x, NULL for a target id outside
// the graph, whose output row is all zeros)
template <typename Tin, typename Tout, bool VEC4, bool kDinv>
__device__ __forceinline__ void finish(const Args& a, typename Piece<VEC4>::type acc, int64_t t, float dt, const Tin* own,
                                       Tout* o, int64_t c) {
  using P = Piece<VEC4>;
  if (own) {
    if constexpr (kDinv) {
      if (a.fill != 0.f) acc = P::fma(dt * a.fill * dt, P::load(own + c), acc);  // (k_gcn_coef's self_coef)
    } else {
      if (a.self_w) acc = P::fma(a.self_w[t], P::load(own + c), acc);
    }
  }
  P::store(o + c, acc);
}

template <typename Tin, typename Tout, bool VEC4, bool kW, bool kDinv>
__global__ __launch_bounds__(kNT) void k_graph_aggw_rows(const Tin* __restrict__ x, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
  const NodeRows<Tin> row(x, a);
  const int lpr = 1 << a.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t i = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> a.lpr_log2;
  if (i >= a.T) return;
  const int64_t t = a.target(i);
  const bool in_graph = (uint64_t)t < (uint64_t)a.x_rows;
  const int64_t b = in_graph ? a.rowptr[t] : 0, e = in_graph ? a.rowptr[t + 1] : 0;
  if (e - b > kGraphChunk) {  // a long row: k_graph_aggw_long's
    if (lane == 0) a.long_rows.append(i);
    return;
  }
  const float dt = kDinv && in_graph ? a.dinv[t] : 0.f;
  const Coef<kW, kDinv> coef{a.w, a.dinv, a.x_rows, dt};
  const Tin* own = in_graph ? row(t) : nullptr;
  Tout* o = out + i * a.out_stride;
  for (int64_t c = (int64_t)lane * P::kWidth; c < a.F; c += (int64_t)lpr * P::kWidth)
    finish<Tin, Tout, VEC4, kDinv>(a, fma_entries<Tin, VEC4>(row, a.col, coef, b, e, c), t, dt, own, o, c);
}

template <typename Tin, typename Tout, bool VEC4, bool kW, bool kDinv>
__global__ __launch_bounds__(kNT) void k_graph_aggw_long(const Tin* __restrict__ x, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
  using piece = typename P::type;
  __shared__ piece part[2][kNT];
  const int lpr = 1 << a.lpr_log2, groups = kNT >> a.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1), grp = threadIdx.x >> a.lpr_log2;
  const NodeRows<Tin> row(x, a);
  const int64_t n = a.long_rows.count();
  unsigned round = 0;  // (workgroup-uniform, as every loop bound below: all 256 threads reach every barrier)
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = a.long_rows.list[r];
    const int64_t t = a.target(i);  // (inside the graph: the row was found long)
    const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
    const int64_t chunks = (e - b + kGraphChunk - 1) / kGraphChunk;
    const float dt = kDinv ? a.dinv[t] : 0.f;
    const Coef<kW, kDinv> coef{a.w, a.dinv, a.x_rows, dt};
    Tout* o = out + i * a.out_stride;
    for (int64_t c0 = 0; c0 < a.F; c0 += (int64_t)lpr * P::kWidth) {
      const int64_t c = c0 + (int64_t)lane * P::kWidth;
      const bool active = c < a.F;
      piece total = P::zero();
      for (int64_t j0 = 0; j0 < chunks; j0 += groups, ++round) {
        // group g sums chunk j0 + g; round k parks its sums in part[k & 1], which is written again in round k + 2,
        // behind the barrier of round k + 1 that group 0 reaches after it has read them
        const int64_t j = j0 + grp;
        piece p = P::zero();
        if (active && j < chunks) {
          const int64_t cb = b + j * kGraphChunk;
          p = fma_entries<Tin, VEC4>(row, a.col, coef, cb, std::min<int64_t>(e, cb + kGraphChunk), c);
        }
        part[round & 1][threadIdx.x] = p;
        __syncthreads();
        if (grp == 0) {
          const int m = (int)std::min<int64_t>(groups, chunks - j0);
          for (int g = 0; g < m; ++g) P::add(total, part[round & 1][(g << a.lpr_log2) + lane]);
        }
      }
      if (grp == 0 && active) finish<Tin, Tout, VEC4, kDinv>(a, total, t, dt, row(t), o, c);
    }
  }
}

}  // namespace graph_agg_w
}  // namespace spp

using namespace spp;
using namespace spp::graph_agg_w;

namespace {

template <typename Tin, typename Tout, bool V, bool kW, bool kDinv>
void launch(const Launch& l, const void* x, void* out, const Args& a, hipStream_t st) {
  hipLaunchKernelGGL((k_graph_aggw_rows<Tin, Tout, V, kW, kDinv>), dim3(l.grid), dim3(kNT), 0, st, static_cast<const Tin*>(x),
                     static_cast<Tout*>(out), a);
  hipLaunchKernelGGL((k_graph_aggw_long<Tin, Tout, V, kW, kDinv>), dim3(l.long_grid), dim3(kNT), 0, st,
                     static_cast<const Tin*>(x), static_cast<Tout*>(out), a);
}

}  // namespace

extern "C" spp_status spp_graph_agg_weighted_forward(const spp_graph_agg_weighted_desc* desc, void* workspace_dev,
                                                     int64_t workspace_bytes, void* stream) {
  const char* who = "spp_graph_agg_weighted_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_agg_weighted_desc& d = *desc;
  SPP_REQUIRE(!(d.dinv_dev && d.self_w_dev),
              "%s: dinv_dev and self_w_dev together (with dinv_dev the self term is dinv[t] * fill * dinv[t])", who);
  SPP_REQUIRE(!d.dinv_dev || (d.fill >= 0 && d.fill <= 2), "%s: unknown fill %d (1, 2 for improved, 0 for no self loops)", who,
              (int)d.fill);
  SPP_REQUIRE(aligned_to(d.w_dev, 4) && aligned_to(d.dinv_dev, 4) && aligned_to(d.self_w_dev, 4),
              "%s: misaligned buffer (w, dinv or self_w is not aligned to its element)", who);
  const Common c{d.x_elem, d.out_elem,    d.rowptr_dev,     d.col_dev,     d.x_stride_elems, d.x_rows,
                 d.F,      d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,        d.out_stride_elems};
  Launch l;
  SPP_TRY(check_common(who, c, d.F, d.F, &d.x_dev, 1, true, workspace_dev, workspace_bytes, &l));
  if (l.empty) return SPP_OK;
  hipStream_t st = as_stream(stream);
  Args a{};
  static_cast<Targets&>(a) = l.targets;
  a.w = d.w_dev, a.dinv = d.dinv_dev, a.self_w = d.self_w_dev, a.fill = (float)d.fill;
  a.lpr_log2 = l.lpr_log2, a.long_rows = l.long_rows;
  SPP_HIP_TRY(hipMemsetAsync(workspace_dev, 0, kWorkspaceHeader, st));
  with_in_out_vec(d.x_elem, d.out_elem, l.vec, [&](auto tin, auto tout, auto v) {
    using Tin = typename decltype(tin)::type;
    using Tout = typename decltype(tout)::type;
    constexpr bool V = decltype(v)::value;
    if (d.dinv_dev)
      d.w_dev ? launch<Tin, Tout, V, true, true>(l, d.x_dev, d.out_dev, a, st)
              : launch<Tin, Tout, V, false, true>(l, d.x_dev, d.out_dev, a, st);
    else
      d.w_dev ? launch<Tin, Tout, V, true, false>(l, d.x_dev, d.out_dev, a, st)
              : launch<Tin, Tout, V, false, false>(l, d.x_dev, d.out_dev, a, st);
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
