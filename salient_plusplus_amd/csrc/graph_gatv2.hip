// f3w: GATv2Conv attention over rows of the RESIDENT graph -- the message passing of exact, layer-wise GATv2 inference,
// on rows the caller has projected (x_l = lin_l(x), x_r = lin_r(x), both [x_rows, H * C] and indexed by global node id):
//     e_j^h      = sum_c att[h,c] * leaky_relu(x_l[j,h,c] + x_r[t,h,c], slope)   j in col[rowptr[t] .. rowptr[t+1])
//                                                                                 without j == t, plus j = t
//     out[i,h,:] = sum_j softmax_j(e^h)_j * x_l[j,h,:]                           t = target_row0 + i  or  target_ids[i]
// What differs from a sampled hop (gatv2.hip, k_gatv2_fwd): the targets are any rows of the graph, a row is as long as
// the node's degree, and nothing is kept for a backward.  What differs from graph_gat.hip: the logit of an entry is a
// C-wide dot product per head with the LeakyReLU inside it, so there are no per-node logits to precompute and a lane
// cannot own a head's state alone: the lane mapping, the butterfly and the online softmax are gatv2_core.hip.h's, the
// ones k_gatv2_fwd runs, and a short row comes out with that kernel's bits.
//
// Softmax contract (include/spp.h, spp_graph_gatv2_forward): C_g = kGatv2Chunk.  A state is, per head, (m, s, acc) with
// acc the head's C columns.  A row of at most C_g raw entries is ONE online softmax in CSR order from the self loop's
// state (m = e_tt, s = 1, acc = x_l[t]).  A longer row is cut into consecutive chunks of C_g raw positions; chunk 0
// starts from the self loop's state, every other chunk from the empty state (m = -inf, s = 0, acc = 0), and the chunk
// states are merged in chunk order.  Nothing else enters: not the grid, not the slab, not the list order, not the other
// rows of the launch.  Weights by expf, as gatv2.hip (spp.h f3v).
//
// Load balance, two launches on the stream and no host wait (the shape of graph_gat.hip; graph_rows.hip.h holds what the
// families share):
//   k_graph_gatv2_rows  lpr lanes per target finish every row of at most C_g raw entries; lane 0 of a longer row appends
//                       its OUTPUT index to a list in the caller's workspace (one atomic on a counter the entry zeroes).
//   k_graph_gatv2_long  one workgroup per listed row, striding over the list: its 256 / lpr lane groups run 256 / lpr
//                       chunks at a time, park the per-head (m, s) and the D accumulator columns in LDS, and group 0
//                       merges them in chunk order (double-buffered: one barrier a round).
// Every loop bound around a barrier is workgroup-uniform, every bound around a shuffle group-uniform (b, e, t and the
// chunk are the group's).  Every offset is 64-bit.  No atomics touch the output.
#include "gatv2_core.hip.h"
#include "graph_rows.hip.h"

namespace spp {
namespace graph_gatv2 {

using namespace graph_rows;
using namespace gatv2;

constexpr int64_t kGatv2Chunk = 64;  // C_g

struct Args : Targets {  // (x_stride: x_l's; F = D = H * C)
  const float* att;      // [H, C]
  int64_t xr_stride;
  float slope;
  int32_t relu;
  int lpr_log2, seg_log2;
  LongRows long_rows;
};

template <typename Tout>
__device__ __forceinline__ void put(const Args& a, Tout* o, f4 r) {
  store4(o, a.relu ? Piece<true>::relu(r) : r);
}

template <int NQ, int CPH>
__device__ __forceinline__ Lane<NQ, CPH> lane_of(const Args& a) {
  Lane<NQ, CPH> L;
  L.slope = a.slope, L.lpr = 1 << a.lpr_log2, L.lane = threadIdx.x & (L.lpr - 1), L.seg_log2 = a.seg_log2;
  return L;
}

template <typename Tin, typename Tout, int NQ, int CPH>
__global__ __launch_bounds__(kNT) void k_graph_gatv2_rows(const Tin* xl, const Tin* xr, Tout* __restrict__ out, Args a) {
  Lane<NQ, CPH> L = lane_of<NQ, CPH>(a);
  const int64_t i = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> a.lpr_log2;
  if (i >= a.T) return;  // whole groups leave together (the shuffles stay inside a group), here and below
  const int64_t t = a.target(i);
  Tout* o = out + i * a.out_stride;
  if ((uint64_t)t >= (uint64_t)a.x_rows) {  // a target outside the graph: a row of zeros
#pragma unroll
    for (int q = 0; q < NQ; ++q) store4(o + L.col0(q), f4{0.f, 0.f, 0.f, 0.f});
    return;
  }
  const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
  if (e - b > kGatv2Chunk) {  // a long row: k_graph_gatv2_long's
    if (L.lane == 0) a.long_rows.append(i);
    return;
  }
  L.load(a.att, xr + t * a.xr_stride);
  State<NQ, CPH> st;
  self_state(st, L, xl + t * a.x_stride);
  walk(st, L, xl, a.x_stride, a.col, b, e, t, a.x_rows);
#pragma unroll
  for (int q = 0; q < NQ; ++q) put(a, o + L.col0(q), st.result(q));
}

template <typename Tin, typename Tout, int NQ, int CPH>
__global__ __launch_bounds__(kNT) void k_graph_gatv2_long(const Tin* xl, const Tin* xr, Tout* __restrict__ out, Args a) {
  constexpr int HL = NQ / CPH;
  // a thread's state at [buf][.][threadIdx.x]: consecutive lanes, consecutive 16 (4) bytes
  __shared__ f4 part_acc[2][NQ][kNT];
  __shared__ float part_m[2][HL][kNT], part_s[2][HL][kNT];
  Lane<NQ, CPH> L = lane_of<NQ, CPH>(a);
  const int groups = kNT >> a.lpr_log2, grp = threadIdx.x >> a.lpr_log2;
  const int64_t n = a.long_rows.count();
  unsigned round = 0;  // (workgroup-uniform, as every loop bound below: all 256 threads reach every barrier)
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = a.long_rows.list[r];
    const int64_t t = a.target(i);  // (inside the graph: the row was found long)
    const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
    const int64_t chunks = (e - b + kGatv2Chunk - 1) / kGatv2Chunk;
    L.load(a.att, xr + t * a.xr_stride);
    State<NQ, CPH> total;
    total.clear();  // (set from chunk 0's state in the first round)
    for (int64_t j0 = 0; j0 < chunks; j0 += groups, ++round) {
      // group g runs chunk j0 + g; round k parks its states in part_*[k & 1], which are written again in round k + 2,
      // behind the barrier of round k + 1 that group 0 reaches after it has read them
      const int64_t j = j0 + grp;
      State<NQ, CPH> st;
      st.clear();
      if (j < chunks) {
        const int64_t cb = b + j * kGatv2Chunk;
        if (j == 0) self_state(st, L, xl + t * a.x_stride);
        walk(st, L, xl, a.x_stride, a.col, cb, std::min<int64_t>(e, cb + kGatv2Chunk), t, a.x_rows);
      }
      const int buf = round & 1;
#pragma unroll
      for (int q = 0; q < NQ; ++q) part_acc[buf][q][threadIdx.x] = st.acc[q];
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) part_m[buf][hl][threadIdx.x] = st.mm[hl], part_s[buf][hl][threadIdx.x] = st.ss[hl];
      __syncthreads();
      if (grp == 0) {
        const int m = (int)std::min<int64_t>(groups, chunks - j0);
        for (int g = 0; g < m; ++g) {
          const int at = (g << a.lpr_log2) + L.lane;
          State<NQ, CPH> p;
#pragma unroll
          for (int q = 0; q < NQ; ++q) p.acc[q] = part_acc[buf][q][at];
#pragma unroll
          for (int hl = 0; hl < HL; ++hl) p.mm[hl] = part_m[buf][hl][at], p.ss[hl] = part_s[buf][hl][at];
          if (j0 == 0 && g == 0) total = p; else total.merge(p);
        }
      }
    }
    if (grp == 0) {
      Tout* o = out + i * a.out_stride;
#pragma unroll
      for (int q = 0; q < NQ; ++q) put(a, o + L.col0(q), total.result(q));
    }
  }
}

}  // namespace graph_gatv2
}  // namespace spp

using namespace spp;
using namespace spp::graph_gatv2;

extern "C" int64_t spp_graph_gatv2_chunk(void) { return kGatv2Chunk; }

extern "C" int64_t spp_graph_gatv2_workspace_bytes(int64_t num_targets) { return workspace_bytes(num_targets); }

extern "C" spp_status spp_graph_gatv2_forward(const spp_graph_gatv2_desc* desc, void* workspace_dev,
                                              int64_t workspace_bytes, void* stream) {
  const char* who = "spp_graph_gatv2_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_gatv2_desc& d = *desc;
  SPP_TRY(check_heads(who, d.heads));  // the shapes of spp_gatv2_forward, in its order
  SPP_TRY(check_channels(who, d.heads, d.C));
  const int64_t D = d.heads * d.C;
  const Common c{d.x_elem, d.out_elem,    d.rowptr_dev,     d.col_dev,     d.x_l_stride_elems, d.x_rows,
                 D,        d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,          d.out_stride_elems};
  const void* bases[2] = {d.x_l_dev, d.x_r_dev};
  Launch l;
  SPP_TRY(check_common(who, c, D, d.C, bases, 2, d.att_dev != nullptr, workspace_dev, workspace_bytes, &l, false,
                       "spp_graph_gatv2_workspace_bytes", "x_l_stride_elems"));
  if (l.empty) return SPP_OK;
  SPP_REQUIRE(d.x_r_stride_elems >= D, "%s: row stride (x_r_stride_elems) smaller than the row", who);
  SPP_REQUIRE(l.vec && d.x_r_stride_elems % 4 == 0 && aligned_to(d.att_dev, 16),
              "%s: misaligned buffer (rows of x_l and x_r: 4 elements, base and stride; att: 16 bytes)", who);
  const Shape sh = shape_of(d.heads, d.C);  // (lpr_log2 is check_common's: lanes_log2(D / 4))
  hipStream_t st = as_stream(stream);
  const Args a{l.targets, d.att_dev, d.x_r_stride_elems, d.negative_slope, d.relu != 0, sh.lpr_log2, sh.seg_log2, l.long_rows};
  SPP_HIP_TRY(hipMemsetAsync(workspace_dev, 0, kWorkspaceHeader, st));
  with_elem(d.x_elem, [&](auto tin) {
    with_f32_bf16(d.out_elem, [&](auto tout) {
      with_fwd_shape(sh.nq, sh.cph, [&](auto q, auto h) {
        using Tin = typename decltype(tin)::type;
        using Tout = typename decltype(tout)::type;
        constexpr int NQ = decltype(q)::value, CPH = decltype(h)::value;
        const Tin* xl = static_cast<const Tin*>(d.x_l_dev);
        const Tin* xr = static_cast<const Tin*>(d.x_r_dev);
        Tout* out = static_cast<Tout*>(d.out_dev);
        hipLaunchKernelGGL((k_graph_gatv2_rows<Tin, Tout, NQ, CPH>), dim3(l.grid), dim3(kNT), 0, st, xl, xr, out, a);
        hipLaunchKernelGGL((k_graph_gatv2_long<Tin, Tout, NQ, CPH>), dim3(l.long_grid), dim3(kNT), 0, st, xl, xr, out, a);
      });
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
