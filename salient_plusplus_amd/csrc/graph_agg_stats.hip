// f4e: MEAN / MIN / MAX / STD over rows of the RESIDENT graph's CSR in one pass, times degree scalers -- the message
// passing of exact, layer-wise PNA inference; the member of graph_aggregate.hip's family for aggregate_stats.hip's four
// statistics.  Forward only.  For output row i, t = target_row0 + i or target_ids[i], entries k in [b, e) of t's CSR
// row, d = e - b, v_k = x[col[k]], per column, all in fp32:
//     K = v_b, the row's FIRST entry          s1 = sum (v_k - K)        s2 = sum (v_k - K)^2
//     mean = K + s1 / d      std = sqrt(max(s2 / d - (s1 / d)^2, 0) + eps)      min, max by take_min / take_max
//     out[i] = [scaler][mean + add | min + add | max + add | std][F], scalers 1, log(d + 1) / delta, delta / log(d + 1)
//
// Contract (include/spp.h, spp_graph_agg_stats_forward): C = kGraphChunk.  A row of d <= C entries runs in CSR order one
// entry at a time from its first entry: k_agg_stats_fwd's arithmetic.  A longer row is cut into consecutive chunks of C
// entries; EVERY chunk is shifted by the row's K, not by its own first entry, so s1 and s2 of the chunks are sums of the
// same addends as the row's and combine by plain addition, in chunk order -- no correction term between two shifts.  A
// chunk's min and max start from the chunk's first entry and are combined in chunk order by the same rule (a later value
// wins only if strictly better or a NaN; a NaN held stays).  Nothing else enters a row's result.
//
// Load balance, two launches on the stream and no host wait (graph_aggregate.hip's shape):
//   k_graph_stats_rows  lpr lanes per target, a lane 4 columns at a time with K, mn, mx, s1, s2 in registers (20 for the
//                       piece) and four neighbour rows in flight; finishes every row of d <= C, lists the longer ones.
//   k_graph_stats_long  one workgroup per listed row; each of its 256 / lpr lane groups loads row col[b] once per column
//                       round (the shift: one extra row per 64) and takes one chunk a round; the groups park mn, mx, s1,
//                       s2 in LDS (2 buffers x 4 x 256 f4 = 32 KB, one barrier a round) and group 0 folds them in chunk
//                       order and runs the epilogue.
// No CSR position is kept (there is no backward), so every offset is 64-bit.  No atomics touch the output.
#include "graph_rows.hip.h"

namespace spp {
namespace graph_agg_stats {

using namespace graph_rows;

constexpr int kMaxScalers = 3;
constexpr int64_t kMaxElems = (int64_t)1 << 62;

struct Args : Targets {
  int n_scalers;
  int kind[kMaxScalers];  // 0 identity, 1 amplification, 2 attenuation: the enabled ones, in that order
  float delta, eps;
  const float* add;  // [T, F] dense by OUTPUT row, or NULL
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

// aggregate_stats.hip's comparison rule without the positions: v, a LATER value, replaces the best only if it is
// strictly better or a NaN, and the best is not a NaN already
__device__ __forceinline__ void take_max(float& best, float v) { best = (!(v <= best) && best == best) ? v : best; }
__device__ __forceinline__ void take_min(float& best, float v) { best = (!(v >= best) && best == best) ? v : best; }
__device__ __forceinline__ void take_max(f4& best, f4 v) {
  take_max(best.x, v.x), take_max(best.y, v.y), take_max(best.z, v.z), take_max(best.w, v.w);
}
__device__ __forceinline__ void take_min(f4& best, f4 v) {
  take_min(best.x, v.x), take_min(best.y, v.y), take_min(best.z, v.z), take_min(best.w, v.w);
}

__device__ __forceinline__ float scaler(int kind, float logd, float delta) {
  return kind == 0 ? 1.f : kind == 1 ? logd / delta : delta / logd;
}
__device__ __forceinline__ f4 times(f4 a, float s) { return {a.x * s, a.y * s, a.z * s, a.w * s}; }
__device__ __forceinline__ f4 plus(f4 a, f4 b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

// four columns' running state over a run of entries, shifted by K
struct Stats {
  f4 mn, mx, s1, s2;
  // one column, one entry: k_agg_stats_fwd's Col::next
  static __device__ __forceinline__ void next1(float& mn, float& mx, float& s1, float& s2, float K, float v) {
    take_min(mn, v);
    take_max(mx, v);
    const float dv = v - K;  // shifted: a column like 1000 + noise keeps its digits
    s1 += dv;
    s2 = fmaf(dv, dv, s2);
  }
  __device__ __forceinline__ void next(const f4& K, f4 v) {
    next1(mn.x, mx.x, s1.x, s2.x, K.x, v.x);
    next1(mn.y, mx.y, s1.y, s2.y, K.y, v.y);
    next1(mn.z, mx.z, s1.z, s2.z, K.z, v.z);
    next1(mn.w, mx.w, s1.w, s2.w, K.w, v.w);
  }
  // columns c.. of the entries [b, e), b < e, in CSR order from zero sums; min and max start from entry b.  kOwnK: the
  // run is a whole row and its first entry IS the shift (returned in K; its own addend v - v is left out, as in
  // k_agg_stats_fwd); otherwise K is the row's, loaded by the caller.  Four rows are in flight; the arithmetic of a column stays sequential.
  template <bool kOwnK, typename Tin>
  __device__ __forceinline__ void run(const NodeRows<Tin>& row, const int64_t* __restrict__ col, f4& K, int64_t b, int64_t e,
                                      int64_t c) {
    const f4 first = load4(row(col[b]) + c);
    if constexpr (kOwnK) K = first;
    mn = mx = first;
    s1 = s2 = f4{0.f, 0.f, 0.f, 0.f};
    if constexpr (!kOwnK) next(K, first);  // (a chunk's first entry is an addend like any other; mn and mx keep it)
    int64_t k = b + 1;
    for (; k + 3 < e; k += 4) {
      const int64_t j0 = col[k], j1 = col[k + 1], j2 = col[k + 2], j3 = col[k + 3];
      const f4 v0 = load4(row(j0) + c), v1 = load4(row(j1) + c), v2 = load4(row(j2) + c), v3 = load4(row(j3) + c);
      next(K, v0);
      next(K, v1);
      next(K, v2);
      next(K, v3);
    }
    for (; k < e; ++k) next(K, load4(row(col[k]) + c));
  }
};

// an empty row, or a target outside the graph: zeros everywhere, add or not
template <typename Tout>
__device__ __forceinline__ void zeros(const Args& a, Tout* o, int64_t c) {
  const f4 z = {0.f, 0.f, 0.f, 0.f};
  for (int64_t w = 0; w < 4 * a.n_scalers; ++w) store4(o + w * a.F + c, z);
}

// k_agg_stats_fwd's epilogue: columns c.. of output row i, whose row has d > 0 entries
template <typename Tout>
__device__ __forceinline__ void finish(const Args& a, const f4& K, const Stats& q, int64_t d, int64_t i, Tout* o, int64_t c) {
  const float inv = 1.f / (float)d, logd = logf((float)d + 1.f);
  const f4 m1 = {q.s1.x * inv, q.s1.y * inv, q.s1.z * inv, q.s1.w * inv};
  f4 mean = {K.x + m1.x, K.y + m1.y, K.z + m1.z, K.w + m1.w};
  const f4 sd = {sqrtf(fmaxf(q.s2.x * inv - m1.x * m1.x, 0.f) + a.eps), sqrtf(fmaxf(q.s2.y * inv - m1.y * m1.y, 0.f) + a.eps),
                 sqrtf(fmaxf(q.s2.z * inv - m1.z * m1.z, 0.f) + a.eps), sqrtf(fmaxf(q.s2.w * inv - m1.w * m1.w, 0.f) + a.eps)};
  f4 mn = q.mn, mx = q.mx;
  if (a.add) {  // the target's own half of the message: mean, min and max move with it, the spread does not
    const f4 ad = load4(a.add + i * a.F + c);
    mean = plus(mean, ad), mn = plus(mn, ad), mx = plus(mx, ad);
  }
  for (int s = 0; s < a.n_scalers; ++s) {
    const float sc = scaler(a.kind[s], logd, a.delta);
    Tout* os = o + (int64_t)s * 4 * a.F + c;
    store4(os, times(mean, sc));
    store4(os + a.F, times(mn, sc));
    store4(os + 2 * a.F, times(mx, sc));
    store4(os + 3 * a.F, times(sd, sc));
  }
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(kNT) void k_graph_stats_rows(const Tin* __restrict__ x, Tout* __restrict__ out, Args a) {
  const NodeRows<Tin> row(x, a);
  const int lpr = 1 << a.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t i = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> a.lpr_log2;
  if (i >= a.T) return;
  const int64_t t = a.target(i);
  const bool in_graph = (uint64_t)t < (uint64_t)a.x_rows;
  const int64_t b = in_graph ? a.rowptr[t] : 0, e = in_graph ? a.rowptr[t + 1] : 0;
  if (e - b > kGraphChunk) {  // a long row: k_graph_stats_long's
    if (lane == 0) a.long_rows.append(i);
    return;
  }
  Tout* o = out + i * a.out_stride;
  for (int64_t c = (int64_t)lane * 4; c < a.F; c += (int64_t)lpr * 4) {
    if (b >= e) {
      zeros(a, o, c);
      continue;
    }
    f4 K;
    Stats q;
    q.template run<true>(row, a.col, K, b, e, c);
    finish(a, K, q, e - b, i, o, c);
  }
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(kNT) void k_graph_stats_long(const Tin* __restrict__ x, Tout* __restrict__ out, Args a) {
  __shared__ f4 part[2][4][kNT];  // [buffer][mn, mx, s1, s2][thread]: 32 KB
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
    Tout* o = out + i * a.out_stride;
    for (int64_t c0 = 0; c0 < a.F; c0 += (int64_t)lpr * 4) {
      const int64_t c = c0 + (int64_t)lane * 4;
      const bool active = c < a.F;  // (F = 260: the lanes behind the last piece idle, and still reach the barriers)
      f4 K = {0.f, 0.f, 0.f, 0.f};
      if (active && grp < chunks) K = load4(row(a.col[b]) + c);  // the ROW's shift, once per group, for all its chunks
      Stats total;
      total.mn = total.mx = total.s1 = total.s2 = f4{0.f, 0.f, 0.f, 0.f};
      for (int64_t j0 = 0; j0 < chunks; j0 += groups, ++round) {
        // group g takes chunk j0 + g; round k parks its state in part[k & 1], which is written again in round k + 2,
        // behind the barrier of round k + 1 that group 0 reaches after it has read them
        const int64_t j = j0 + grp;
        if (active && j < chunks) {
          const int64_t cb = b + j * kGraphChunk;
          Stats p;
          p.template run<false>(row, a.col, K, cb, std::min<int64_t>(e, cb + kGraphChunk), c);
          part[round & 1][0][threadIdx.x] = p.mn;
          part[round & 1][1][threadIdx.x] = p.mx;
          part[round & 1][2][threadIdx.x] = p.s1;
          part[round & 1][3][threadIdx.x] = p.s2;
        }
        __syncthreads();
        if (grp == 0 && active) {
          const int m = (int)std::min<int64_t>(groups, chunks - j0);  // (only chunks that were written are read)
          for (int g = 0; g < m; ++g) {
            const int at = (g << a.lpr_log2) + lane;
            const f4 qmn = part[round & 1][0][at], qmx = part[round & 1][1][at];
            if (j0 == 0 && g == 0) total.mn = qmn, total.mx = qmx;  // (they start from the first chunk's, not from zero)
            else take_min(total.mn, qmn), take_max(total.mx, qmx);
            Piece<true>::add(total.s1, part[round & 1][2][at]);
            Piece<true>::add(total.s2, part[round & 1][3][at]);
          }
        }
      }
      if (grp == 0 && active) finish(a, K, total, e - b, i, o, c);
    }
  }
}

}  // namespace graph_agg_stats
}  // namespace spp

using namespace spp;
using namespace spp::graph_agg_stats;

extern "C" spp_status spp_graph_agg_stats_forward(const spp_graph_agg_stats_desc* desc, void* workspace_dev,
                                                  int64_t workspace_bytes, void* stream) {
  const char* who = "spp_graph_agg_stats_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_agg_stats_desc& d = *desc;
  SPP_REQUIRE(d.scalers >= 1 && d.scalers <= 7, "%s: scalers must be a non-empty mask of identity 1, amplification 2, "
              "attenuation 4 (got %d)", who, (int)d.scalers);
  SPP_REQUIRE(d.delta > 0.f && d.delta <= 3.0e38f && d.eps >= 0.f && d.eps <= 3.0e38f,
              "%s: delta must be positive and eps non-negative, both finite", who);
  SPP_REQUIRE(d.F % 4 == 0, "%s: F %% 4 != 0 (F = %lld): four columns per lane only, there is no scalar form", who,
              (long long)d.F);
  Args a{};
  for (int s = 0; s < kMaxScalers; ++s)
    if (d.scalers >> s & 1) a.kind[a.n_scalers++] = s;
  SPP_REQUIRE(d.F <= 0 || d.num_targets < kMaxElems / (4 * kMaxScalers * d.F), "%s: num_targets * F out of range", who);
  const Common c{d.x_elem, d.out_elem,    d.rowptr_dev,     d.col_dev,     d.x_stride_elems, d.x_rows,
                 d.F,      d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,        d.out_stride_elems};
  Launch l;
  SPP_TRY(check_common(who, c, (int64_t)a.n_scalers * 4 * d.F, d.F, &d.x_dev, 1, true, workspace_dev, workspace_bytes, &l,
                       false, "spp_graph_agg_workspace_bytes"));
  if (l.empty) return SPP_OK;
  SPP_REQUIRE(l.vec && aligned_to(d.add_dev, 16),
              "%s: the vector form is the only form: x_dev and add_dev aligned to 4 elements, x_stride_elems %% 4 == 0", who);
  static_cast<Targets&>(a) = l.targets;
  a.delta = d.delta, a.eps = d.eps, a.add = d.add_dev, a.lpr_log2 = l.lpr_log2, a.long_rows = l.long_rows;
  hipStream_t st = as_stream(stream);
  SPP_HIP_TRY(hipMemsetAsync(workspace_dev, 0, kWorkspaceHeader, st));
  with_elem(d.x_elem, [&](auto tin) {
    with_f32_bf16(d.out_elem, [&](auto tout) {
      using Tin = typename decltype(tin)::type;
      using Tout = typename decltype(tout)::type;
      hipLaunchKernelGGL((k_graph_stats_rows<Tin, Tout>), dim3(l.grid), dim3(kNT), 0, st, static_cast<const Tin*>(d.x_dev),
                         static_cast<Tout*>(d.out_dev), a);
      hipLaunchKernelGGL((k_graph_stats_long<Tin, Tout>), dim3(l.long_grid), dim3(kNT), 0, st,
                         static_cast<const Tin*>(d.x_dev), static_cast<Tout*>(d.out_dev), a);
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
