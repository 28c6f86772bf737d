// f3z: TransformerConv attention over rows of the RESIDENT graph -- the message passing of exact, layer-wise
// GraphTransformer inference, on rows the caller has projected (q = lin_query(x), k = lin_key(x), v = lin_value(x), each
// [x_rows, H * C] and indexed by global node id; optionally skip = lin_skip(x), likewise):
//     e_j^h      = scale * sum_c q[t,h,c] * k[j,h,c]             j in col[rowptr[t] .. rowptr[t+1]), EVERY entry
//     out[i,h,:] = sum_j softmax_j(e^h)_j * v[j,h,:]             t = target_row0 + i  or  target_ids[i]
//     then  + skip[t]  (if given),  max(., 0)  (if relu),  one rounding to out_elem
// What differs from a sampled hop (transformer_conv.hip, k_transformer_fwd): the targets are any rows of the graph, a row
// is as long as the node's degree, nothing is kept for a backward, and the layer's root term and ReLU ride in the
// epilogue.  What differs from graph_gatv2.hip: no self loop (so a row may be empty: zeros, nothing divided), no entry is
// skipped, the message row is not the key row, and the skip row is added after the attention and before the ReLU.
// The per-entry arithmetic is transformer_core.hip.h's walk, the one k_transformer_fwd runs: a short row comes out with
// that kernel's bits.
//
// Softmax contract (include/spp.h, spp_graph_transformer_forward): C_g = kTfChunk.  A row of at most C_g entries is ONE
// online softmax in CSR order from the empty state (m = -inf, s = 0, acc = 0).  A longer row is cut into consecutive
// chunks of C_g entries; EVERY chunk, chunk 0 included, starts from the empty state, and the chunk states are merged in
// chunk order into chunk 0's.  Every chunk of such a row holds at least one entry and every entry is taken, so every
// merged state is finite (transformer_core.hip.h says why two empty states never meet).  Nothing else enters: not the
// grid, not the slab, not the list order, not the other rows of the launch.  Weights by expf.
//
// Aliasing: skip may be the very rows the call writes (skip row of target t == output row i, same element type: a slab
// over a [x_rows, D] matrix).  A lane reads its four columns of the skip row before it writes those four columns and
// nobody else touches them, so `out` is NOT __restrict__ here.
//
// Two launches on the stream and no host wait, as graph_gatv2.hip:
//   k_graph_transformer_rows  lpr lanes per target finish every row of at most C_g entries; lane 0 of a longer row
//                             appends its OUTPUT index to the list in the caller's workspace.
//   k_graph_transformer_long  one workgroup per listed row, striding over the list: its 256 / lpr lane groups run
//                             256 / lpr chunks at a time, park (m, s, acc) in LDS, and group 0 merges them in chunk order
//                             (double-buffered: one barrier a round).  A group whose chunk index is past the row's end
//                             parks the empty state, which is never read.
// Every loop bound around a barrier is workgroup-uniform, every bound around a shuffle group-uniform.  Every offset is
// 64-bit.  No atomics touch the output.
#include "graph_rows.hip.h"
#include "transformer_core.hip.h"

#include <cmath>

namespace spp {
namespace graph_transformer {

using namespace graph_rows;
using namespace gatv2;
using namespace transformer;

constexpr int64_t kTfChunk = 64;  // C_g

struct Args : Targets {  // (x_stride: k's; F = D = H * C)
  int64_t q_stride, v_stride, skip_stride;
  float scale;
  int32_t relu;
  int lpr_log2, seg_log2;
  LongRows long_rows;
};

// the epilogue of one piece: + skip (one rounded fp32 addition a column), ReLU, one rounding to Tout.  The skip columns
// are read before the same columns of o are written (they may be the same addresses).
template <typename Tin, typename Tout>
__device__ __forceinline__ void put(const Args& a, Tout* o, const Tin* skip_row, f4 r) {
#pragma clang fp contract(off)
  if (skip_row) {
    const f4 s = load4(skip_row);
    r = {r.x + s.x, r.y + s.y, r.z + s.z, r.w + s.w};
  }
  store4(o, a.relu ? Piece<true>::relu(r) : r);
}

template <typename Tin, typename Tout, int NQ, int CPH>
__device__ __forceinline__ void finish(const Args& a, const State<NQ, CPH>& st, const int64_t (&c0)[NQ], Tout* o,
                                       const Tin* skip, int64_t t) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    f4 r = {0.f, 0.f, 0.f, 0.f};
    if (st.ss[q / CPH] != 0.f) r = st.result(q);  // a row without entries: zeros, nothing is divided
    put(a, o + c0[q], skip ? skip + t * a.skip_stride + c0[q] : nullptr, r);
  }
}

template <typename Tin, typename Tout, int NQ, int CPH>
__global__ __launch_bounds__(kNT) void k_graph_transformer_rows(const Tin* qm, const Tin* km, const Tin* vm,
                                                                const Tin* skip, Tout* out, Args a) {
  const int lpr = 1 << a.lpr_log2, lane = threadIdx.x & (lpr - 1);
  const int64_t i = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> a.lpr_log2;
  if (i >= a.T) return;  // whole groups leave together (the shuffles stay inside a group), here and below
  const int64_t t = a.target(i);
  Tout* o = out + i * a.out_stride;
  int64_t c0[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) c0[q] = ((int64_t)q * lpr + lane) * 4;
  if ((uint64_t)t >= (uint64_t)a.x_rows) {  // a target outside the graph: a row of zeros, no skip
#pragma unroll
    for (int q = 0; q < NQ; ++q) store4(o + c0[q], f4{0.f, 0.f, 0.f, 0.f});
    return;
  }
  const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
  if (e - b > kTfChunk) {  // a long row: k_graph_transformer_long's
    if (lane == 0) a.long_rows.append(i);
    return;
  }
  f4 qv[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) qv[q] = load4(qm + t * a.q_stride + c0[q]);
  State<NQ, CPH> st;
  st.clear();
  walk<tf_nb<NQ>()>(st, qv, c0, km, a.x_stride, vm, a.v_stride, a.col, b, e, a.x_rows, a.scale, a.seg_log2);
  finish(a, st, c0, o, skip, t);
}

template <typename Tin, typename Tout, int NQ, int CPH>
__global__ __launch_bounds__(kNT) void k_graph_transformer_long(const Tin* qm, const Tin* km, const Tin* vm,
                                                                const Tin* skip, Tout* out, Args a) {
  constexpr int HL = NQ / CPH;
  // a thread's state at [buf][.][threadIdx.x]: consecutive lanes, consecutive 16 (4) bytes
  __shared__ f4 part_acc[2][NQ][kNT];
  __shared__ float part_m[2][HL][kNT], part_s[2][HL][kNT];
  const int lpr = 1 << a.lpr_log2, lane = threadIdx.x & (lpr - 1);
  const int groups = kNT >> a.lpr_log2, grp = threadIdx.x >> a.lpr_log2;
  int64_t c0[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) c0[q] = ((int64_t)q * lpr + lane) * 4;
  const int64_t n = a.long_rows.count();
  unsigned round = 0;  // (workgroup-uniform, as every loop bound below: all 256 threads reach every barrier)
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = a.long_rows.list[r];
    const int64_t t = a.target(i);  // (inside the graph: the row was found long)
    const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
    const int64_t chunks = (e - b + kTfChunk - 1) / kTfChunk;  // >= 2, every one with at least one entry
    f4 qv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) qv[q] = load4(qm + t * a.q_stride + c0[q]);
    State<NQ, CPH> total;
    total.clear();  // (set from chunk 0's state in the first round)
    for (int64_t j0 = 0; j0 < chunks; j0 += groups, ++round) {
      // group g runs chunk j0 + g; round k parks its states in part_*[k & 1], which are written again in round k + 2,
      // behind the barrier of round k + 1 that group 0 reaches after it has read them
      const int64_t j = j0 + grp;
      State<NQ, CPH> st;
      st.clear();
      if (j < chunks) {
        const int64_t cb = b + j * kTfChunk;
        walk<tf_nb<NQ>()>(st, qv, c0, km, a.x_stride, vm, a.v_stride, a.col, cb, std::min<int64_t>(e, cb + kTfChunk),
                            a.x_rows, a.scale, a.seg_log2);
      }
      const int buf = round & 1;
#pragma unroll
      for (int q = 0; q < NQ; ++q) part_acc[buf][q][threadIdx.x] = st.acc[q];
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) part_m[buf][hl][threadIdx.x] = st.mm[hl], part_s[buf][hl][threadIdx.x] = st.ss[hl];
      __syncthreads();
      if (grp == 0) {
        const int m = (int)std::min<int64_t>(groups, chunks - j0);  // the parked states past it are empty: never merged
        for (int g = 0; g < m; ++g) {
          const int at = (g << a.lpr_log2) + lane;
          State<NQ, CPH> p;
#pragma unroll
          for (int q = 0; q < NQ; ++q) p.acc[q] = part_acc[buf][q][at];
#pragma unroll
          for (int hl = 0; hl < HL; ++hl) p.mm[hl] = part_m[buf][hl][at], p.ss[hl] = part_s[buf][hl][at];
          if (j0 == 0 && g == 0) total = p; else total.merge(p);
        }
      }
    }
    if (grp == 0) finish(a, total, c0, out + i * a.out_stride, skip, t);
  }
}

}  // namespace graph_transformer
}  // namespace spp

using namespace spp;
using namespace spp::graph_transformer;

extern "C" int64_t spp_graph_transformer_chunk(void) { return kTfChunk; }

extern "C" int64_t spp_graph_transformer_workspace_bytes(int64_t num_targets) { return workspace_bytes(num_targets); }

extern "C" spp_status spp_graph_transformer_forward(const spp_graph_transformer_desc* desc, void* workspace_dev,
                                                    int64_t workspace_bytes, void* stream) {
  const char* who = "spp_graph_transformer_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_transformer_desc& d = *desc;
  SPP_TRY(check_heads(who, d.heads));  // the shapes of spp_transformer_forward, in its order
  SPP_TRY(check_channels(who, d.heads, d.C));
  const int64_t D = d.heads * d.C;
  const Common c{d.x_elem, d.out_elem,    d.rowptr_dev,     d.col_dev,     d.k_stride_elems, d.x_rows,
                 D,        d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,        d.out_stride_elems};
  const void* bases[3] = {d.k_dev, d.q_dev, d.v_dev};
  Launch l;
  SPP_TRY(check_common(who, c, D, d.C, bases, 3, true, workspace_dev, workspace_bytes, &l, false,
                       "spp_graph_transformer_workspace_bytes", "k_stride_elems"));
  if (l.empty) return SPP_OK;
  const int64_t esz = elem_bytes(d.x_elem);
  SPP_REQUIRE(d.q_stride_elems >= D && d.v_stride_elems >= D && (!d.skip_dev || d.skip_stride_elems >= D),
              "%s: row stride (q_stride_elems, v_stride_elems or skip_stride_elems) smaller than the row", who);
  SPP_REQUIRE(l.vec && d.q_stride_elems % 4 == 0 && d.v_stride_elems % 4 == 0 &&
                  (!d.skip_dev || (d.skip_stride_elems % 4 == 0 && aligned_to(d.skip_dev, 4 * esz))),
              "%s: misaligned buffer (rows of q, k, v and skip: 4 elements, base and stride)", who);
  SPP_REQUIRE(std::isfinite(d.scale) && d.scale > 0.f, "%s: scale must be finite and positive", who);
  const Shape sh = shape_of(d.heads, d.C);  // (lpr_log2 is check_common's: lanes_log2(D / 4))
  hipStream_t st = as_stream(stream);
  Args a;
  static_cast<Targets&>(a) = l.targets;
  a.q_stride = d.q_stride_elems, a.v_stride = d.v_stride_elems, a.skip_stride = d.skip_stride_elems;
  a.scale = d.scale, a.relu = d.relu != 0, a.lpr_log2 = sh.lpr_log2, a.seg_log2 = sh.seg_log2, a.long_rows = l.long_rows;
  SPP_HIP_TRY(hipMemsetAsync(workspace_dev, 0, kWorkspaceHeader, st));
  with_elem(d.x_elem, [&](auto tin) {
    with_f32_bf16(d.out_elem, [&](auto tout) {
      with_fwd_shape(sh.nq, sh.cph, [&](auto q, auto h) {
        using Tin = typename decltype(tin)::type;
        using Tout = typename decltype(tout)::type;
        constexpr int NQ = decltype(q)::value, CPH = decltype(h)::value;
        const Tin* qm = static_cast<const Tin*>(d.q_dev);
        const Tin* km = static_cast<const Tin*>(d.k_dev);
        const Tin* vm = static_cast<const Tin*>(d.v_dev);
        const Tin* sk = static_cast<const Tin*>(d.skip_dev);
        Tout* out = static_cast<Tout*>(d.out_dev);
        hipLaunchKernelGGL((k_graph_transformer_rows<Tin, Tout, NQ, CPH>), dim3(l.grid), dim3(kNT), 0, st, qm, km, vm, sk,
                           out, a);
        hipLaunchKernelGGL((k_graph_transformer_long<Tin, Tout, NQ, CPH>), dim3(l.long_grid), dim3(kNT), 0, st, qm, km, vm,
                           sk, out, a);
      });
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
