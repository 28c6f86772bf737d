// f3h: GATConv attention over rows of the RESIDENT graph -- the message passing of exact, layer-wise GAT inference
// (reference: driver/models.py:228 GAT.inference through layerwise_inference, line 441), in PyG's project-first order:
//     e^h_tj = leaky_relu(a_src[j,h] + a_dst[t,h], slope)     j in col[rowptr[t] .. rowptr[t+1]) without j == t, plus j = t
//     out[i, h*C + c] = sum_j softmax_j(e^h_t.)_j * h[j, h*C + c]          t = target_row0 + i  or  target_ids[i]
// What differs from a sampled hop (gat.hip, k_gat_fwd / k_gat_mh_agg_fwd): the targets are any rows of h, a row
// is as long as the node's degree, and the rows of h are already projected, so a head owns C columns of the row.
//
// Softmax contract (include/spp.h, spp_graph_gat_forward): C_g = kGatChunk.  A state is (m, s, acc): the running
// maximum, the denominator and the weighted sum at that maximum.  A row of at most C_g raw entries is ONE online
// softmax in CSR order from the self loop's state (m = e_self, s = 1, acc = h_t): k_gat_fwd's arithmetic.  A longer
// row is cut into consecutive chunks of C_g raw positions; chunk 0 starts from the self loop's state, every other
// chunk from the empty state (m = -inf, s = 0, acc = 0), and the chunk states are merged in chunk order.  Nothing else
// enters: not the grid, not the slab, not the list order, not the other rows of the launch.
//
// Load balance, two launches on the stream and no host wait (the shape of graph_aggregate.hip; graph_rows.hip.h holds
// what the two share):
//   k_graph_gat_rows  lpr lanes per target finish every row of at most C_g raw entries; lane 0 of a longer row appends
//                     its OUTPUT index to a list in the caller's workspace (one atomic on a counter the entry zeroes).
//   k_graph_gat_long  one workgroup per listed row: its 256 / lpr lane groups run 256 / lpr chunks at a time, park the
//                     chunk STATES in LDS, and group 0 merges them in chunk order (double-buffered: one barrier a round).
// Every lane keeps the state of the head its columns belong to (head = column / C at run time); all lanes of a head
// walk the same entries, so the states need no exchange.  Every offset is 64-bit.  No atomics touch the output.
//
// f3k: the same two kernels over a ROW-PARTITIONED h with its logits (spp_graph_gat_parts_forward).  The row source is a
// template parameter: NodeRows reads one matrix h and the two logit matrices, PartRows finds the part that owns a
// global row first and takes the row of h AND the row of [a_src | a_dst] from that one lookup.  Same arithmetic, same
// order, same bits.
#include "graph_rows.hip.h"

namespace spp {
namespace graph_gat {

using namespace graph_rows;

constexpr int64_t kGatChunk = 64;             // C_g

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// the softmax state of one head over some entries, for the columns of one piece
template <bool VEC4>
struct State {
  using P = Piece<VEC4>;
  float m, s;
  typename P::type acc;
  static __device__ __forceinline__ State empty() { return {-INFINITY, 0.f, P::zero()}; }
  // one more entry with logit e and row piece v (k_gat_fwd's step)
  __device__ __forceinline__ void take(float e, typename P::type v) {
    if (e > m) {
      const float r = __expf(m - e);  // (m = -inf: r = 0, and s, acc are 0)
      acc = P::scaled(acc, r);
      s *= r;
      m = e;
    }
    const float w = __expf(e - m);
    s += w;
    acc = P::fma(w, v, acc);
  }
  // the state of the entries behind this one's.  *this is finite (it began with the self loop); o may be empty:
  // then o.m = -inf, f2 = 0 and f1 = 1, and nothing changes
  __device__ __forceinline__ void merge(const State& o) {
    const float mm = fmaxf(m, o.m);
    const float f1 = __expf(m - mm), f2 = __expf(o.m - mm);
    s = fmaf(o.s, f2, s * f1);
    acc = P::fma(f2, o.acc, P::scaled(acc, f1));
    m = mm;
  }
};

struct Args : Targets {
  const float* a_src;   // [x_rows, H]
  const float* a_dst;   // [x_rows, H]
  int32_t H, C;         // heads, columns per head (F = H * C)
  float slope;
  int32_t relu;
  int lpr_log2;
  LongRows long_rows;
};

// The row source of the kernels: Rows::Src is what the launch passes by value; Rows(src, a) answers, for a global row g
// INSIDE [0, x_rows): owner(g), then the address of g's row of h and g's two logits through that owner.
// one matrix h [x_rows, F] and the logits as two dense [x_rows, H] matrices (Args): nothing to find
template <typename Tin>
struct NodeRows {
  using elem = Tin;
  using Src = const Tin* __restrict__;
  using Owner = int;
  const Tin* __restrict__ x;
  const Args& a;
  __device__ __forceinline__ NodeRows(const Tin* __restrict__ src, const Args& args) : x(src), a(args) {}
  __device__ __forceinline__ Owner owner(int64_t) const { return 0; }
  __device__ __forceinline__ const Tin* h(Owner, int64_t g, int64_t c) const { return x + g * a.x_stride + c; }
  __device__ __forceinline__ float src(Owner, int64_t g, int hd) const { return a.a_src[g * a.H + hd]; }
  __device__ __forceinline__ float dst(Owner, int64_t g, int hd) const { return a.a_dst[g * a.H + hd]; }
};

// h and the logits as row ranges, each pair in allocations of its own (a rank's buffers, mapped into this process):
// graph_rows.hip.h's tables and owner search, table 0 for the rows of h and table 1 for the logits ([rows, a_stride]
// fp32, a_src in columns [0, H), a_dst in [H, 2H)); 384 bytes of LDS.  One search serves the row and its logit.
struct PartSrc {
  PartTable<2> tables;
  int64_t a_stride;
};
template <typename Tin>
struct PartRows {
  using elem = Tin;
  using Src = PartSrc;
  using Owner = int;
  const int64_t* first;       // LDS
  const Tin* const* hb;       // LDS
  const float* const* ab;     // LDS
  int64_t stride, a_stride;
  int H;
  // every thread of the workgroup constructs it, before any of them leaves the kernel (a barrier inside)
  __device__ __forceinline__ PartRows(const Src& src, const Args& a) : stride(a.x_stride), a_stride(src.a_stride), H(a.H) {
    __shared__ int64_t lds_first[kMaxParts];
    __shared__ const Tin* lds_h[kMaxParts];
    __shared__ const float* lds_a[kMaxParts];
    if (threadIdx.x == 0) {
      const PartTable<2>& t = src.tables;
#pragma unroll
      for (int p = 0; p < kMaxParts; ++p)
        lds_first[p] = t.first[p], lds_h[p] = static_cast<const Tin*>(t.base[0][p]),
        lds_a[p] = static_cast<const float*>(t.base[1][p]);
    }
    __syncthreads();
    first = lds_first, hb = lds_h, ab = lds_a;
  }
  __device__ __forceinline__ Owner owner(int64_t g) const { return part_owner(first, g); }
  __device__ __forceinline__ const Tin* h(Owner p, int64_t g, int64_t c) const { return hb[p] + g * stride + c; }
  __device__ __forceinline__ float src(Owner p, int64_t g, int hd) const { return ab[p][g * a_stride + hd]; }
  __device__ __forceinline__ float dst(Owner p, int64_t g, int hd) const { return ab[p][g * a_stride + H + hd]; }
};

// the state of target t's entries col[b .. e) (every entry equal to t skipped), columns c.. of head hd, continued
// from st in CSR order; four rows and their logits are in flight.  An entry outside [0, x_rows) is node 0: its row,
// its logit, and the comparison with t.
template <typename Rows, bool VEC4>
__device__ __forceinline__ void walk(State<VEC4>& st, const Args& a, const Rows& row, int64_t t, float ad, int hd,
                                     int64_t b, int64_t e, int64_t c) {
  using P = Piece<VEC4>;
  auto node = [&](int64_t k) {
    const int64_t j = a.col[k];
    return (uint64_t)j < (uint64_t)a.x_rows ? j : (int64_t)0;
  };
  int64_t k = b;
  for (; k + 3 < e; k += 4) {
    const int64_t j0 = node(k), j1 = node(k + 1), j2 = node(k + 2), j3 = node(k + 3);
    const auto o0 = row.owner(j0), o1 = row.owner(j1), o2 = row.owner(j2), o3 = row.owner(j3);
    const float s0 = row.src(o0, j0, hd), s1 = row.src(o1, j1, hd), s2 = row.src(o2, j2, hd), s3 = row.src(o3, j3, hd);
    const auto v0 = P::load(row.h(o0, j0, c)), v1 = P::load(row.h(o1, j1, c)), v2 = P::load(row.h(o2, j2, c)),
               v3 = P::load(row.h(o3, j3, c));
    if (j0 != t) st.take(lrelu(s0 + ad, a.slope), v0);
    if (j1 != t) st.take(lrelu(s1 + ad, a.slope), v1);
    if (j2 != t) st.take(lrelu(s2 + ad, a.slope), v2);
    if (j3 != t) st.take(lrelu(s3 + ad, a.slope), v3);
  }
  for (; k < e; ++k) {
    const int64_t j = node(k);
    const auto o = row.owner(j);
    const float s = row.src(o, j, hd);
    const auto v = P::load(row.h(o, j, c));
    if (j != t) st.take(lrelu(s + ad, a.slope), v);
  }
}

// the self loop's state of target t (inside the graph, owned by ot)
template <typename Rows, bool VEC4>
__device__ __forceinline__ State<VEC4> self_state(const Args& a, const Rows& row, typename Rows::Owner ot, int64_t t,
                                                  float ad, int hd, int64_t c) {
  return {lrelu(row.src(ot, t, hd) + ad, a.slope), 1.f, Piece<VEC4>::load(row.h(ot, t, c))};
}

template <typename Tout, bool VEC4>
__device__ __forceinline__ void finish(const Args& a, const State<VEC4>& st, Tout* o, int64_t c) {
  using P = Piece<VEC4>;
  const auto r = P::over(st.acc, st.s);
  P::store(o + c, a.relu ? P::relu(r) : r);
}

template <typename Rows, typename Tout, bool VEC4>
__global__ __launch_bounds__(kNT) void k_graph_gat_rows(typename Rows::Src src, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
  const Rows row(src, a);  // (PartRows: the whole workgroup, before anyone returns)
  const int lpr = 1 << a.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t i = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> a.lpr_log2;
  if (i >= a.T) return;
  const int64_t t = a.target(i);
  Tout* o = out + i * a.out_stride;
  if ((uint64_t)t >= (uint64_t)a.x_rows) {  // a target outside the graph: a row of zeros
    for (int64_t c = (int64_t)lane * P::kWidth; c < a.F; c += (int64_t)lpr * P::kWidth) P::store(o + c, P::zero());
    return;
  }
  const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
  if (e - b > kGatChunk) {  // a long row: k_graph_gat_long's
    if (lane == 0) a.long_rows.append(i);
    return;
  }
  const auto ot = row.owner(t);
  for (int64_t c = (int64_t)lane * P::kWidth; c < a.F; c += (int64_t)lpr * P::kWidth) {
    const int hd = (int)c / a.C;
    const float ad = row.dst(ot, t, hd);
    State<VEC4> st = self_state<Rows, VEC4>(a, row, ot, t, ad, hd, c);
    walk<Rows, VEC4>(st, a, row, t, ad, hd, b, e, c);
    finish<Tout, VEC4>(a, st, o, c);
  }
}

template <typename Rows, typename Tout, bool VEC4>
__global__ __launch_bounds__(kNT) void k_graph_gat_long(typename Rows::Src src, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
  using piece = typename P::type;
  __shared__ piece part_acc[2][kNT];
  __shared__ float part_m[2][kNT], part_s[2][kNT];
  const Rows row(src, a);
  const int lpr = 1 << a.lpr_log2, groups = kNT >> a.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1), grp = threadIdx.x >> a.lpr_log2;
  const int64_t n = a.long_rows.count();
  unsigned round = 0;  // (workgroup-uniform, as every loop bound below: all 256 threads reach every barrier)
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = a.long_rows.list[r];
    const int64_t t = a.target(i);  // (inside the graph: the row was found long)
    const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
    const int64_t chunks = (e - b + kGatChunk - 1) / kGatChunk;
    Tout* o = out + i * a.out_stride;
    const auto ot = row.owner(t);
    for (int64_t c0 = 0; c0 < a.F; c0 += (int64_t)lpr * P::kWidth) {
      const int64_t c = c0 + (int64_t)lane * P::kWidth;
      const bool active = c < a.F;
      const int hd = active ? (int)c / a.C : 0;
      const float ad = row.dst(ot, t, hd);
      State<VEC4> total = State<VEC4>::empty();  // (set from chunk 0's state in the first round)
      for (int64_t j0 = 0; j0 < chunks; j0 += groups, ++round) {
        // group g runs chunk j0 + g; round k parks its states in part_*[k & 1], which are written again in round
        // k + 2, behind the barrier of round k + 1 that group 0 reaches after it has read them
        const int64_t j = j0 + grp;
        State<VEC4> st = State<VEC4>::empty();
        if (active && j < chunks) {
          const int64_t cb = b + j * kGatChunk;
          if (j == 0) st = self_state<Rows, VEC4>(a, row, ot, t, ad, hd, c);
          walk<Rows, VEC4>(st, a, row, t, ad, hd, cb, std::min<int64_t>(e, cb + kGatChunk), c);
        }
        const int buf = round & 1;
        part_acc[buf][threadIdx.x] = st.acc;
        part_m[buf][threadIdx.x] = st.m;
        part_s[buf][threadIdx.x] = st.s;
        __syncthreads();
        if (grp == 0) {
          const int m = (int)std::min<int64_t>(groups, chunks - j0);
          for (int g = 0; g < m; ++g) {
            const int at = (g << a.lpr_log2) + lane;
            const State<VEC4> p{part_m[buf][at], part_s[buf][at], part_acc[buf][at]};
            if (j0 == 0 && g == 0) total = p; else total.merge(p);
          }
        }
      }
      if (grp == 0 && active) finish<Tout, VEC4>(a, total, o, c);
    }
  }
}

}  // namespace graph_gat
}  // namespace spp

using namespace spp;
using namespace spp::graph_gat;

extern "C" int64_t spp_graph_gat_chunk(void) { return kGatChunk; }

extern "C" int64_t spp_graph_gat_workspace_bytes(int64_t num_targets) { return workspace_bytes(num_targets); }

namespace {

// the attention's own fields of a descriptor
struct Attention {
  int32_t heads, relu;
  float slope;
};

// the sources of spp_graph_gat_forward: one matrix h and the two logit matrices
struct Whole {
  const void* x;
  const float* a_src;
  const float* a_dst;
};

// what both entries share; exactly one of whole / parts is given (a_stride: the parts' logits stride as given, 0 = dense)
spp_status forward(const char* who, const Common& d, const Attention& g, const Whole* whole, const Parts* parts,
                   int64_t a_stride, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  SPP_REQUIRE(g.heads >= 1 && d.F % g.heads == 0 && d.F < (1ll << 31), "%s: heads %d must be positive and divide F = %lld (< 2^31)",
              who, (int)g.heads, (long long)d.F);
  SPP_REQUIRE(!parts || a_stride == 0 || a_stride >= 2 * (int64_t)g.heads,
              "%s: a_stride_elems %lld smaller than the logits' row of 2 * heads = %d", who, (long long)a_stride,
              2 * (int)g.heads);
  const int64_t Cw = d.F / g.heads;  // (the vector form: four columns of ONE head per lane)
  Launch l;
  SPP_TRY(check_common(who, d, d.F, Cw, parts ? parts->base[0] : &whole->x, parts ? parts->n : 1,
                       parts || (whole->a_src && whole->a_dst), workspace_dev, workspace_bytes, &l));
  if (l.empty) return SPP_OK;
  hipStream_t st = as_stream(stream);
  const Args a{l.targets, parts ? nullptr : whole->a_src, parts ? nullptr : whole->a_dst, g.heads, (int32_t)Cw, g.slope,
               g.relu != 0, l.lpr_log2, l.long_rows};
  SPP_HIP_TRY(hipMemsetAsync(workspace_dev, 0, kWorkspaceHeader, st));
  with_in_out_vec(d.x_elem, d.out_elem, l.vec, [&](auto tin, auto tout, auto v) {
    using Tin = typename decltype(tin)::type;
    using Tout = typename decltype(tout)::type;
    constexpr bool V = decltype(v)::value;
    Tout* out = static_cast<Tout*>(d.out);
    if (parts) {
      PartSrc t{};
      t.a_stride = a_stride > 0 ? a_stride : 2 * (int64_t)g.heads;
      t.tables = part_table<2>(*parts, {d.x_stride * (int64_t)sizeof(Tin), t.a_stride * (int64_t)sizeof(float)});
      hipLaunchKernelGGL((k_graph_gat_rows<PartRows<Tin>, Tout, V>), dim3(l.grid), dim3(kNT), 0, st, t, out, a);
      hipLaunchKernelGGL((k_graph_gat_long<PartRows<Tin>, Tout, V>), dim3(l.long_grid), dim3(kNT), 0, st, t, out, a);
    } else {
      const Tin* x = static_cast<const Tin*>(whole->x);
      hipLaunchKernelGGL((k_graph_gat_rows<NodeRows<Tin>, Tout, V>), dim3(l.grid), dim3(kNT), 0, st, x, out, a);
      hipLaunchKernelGGL((k_graph_gat_long<NodeRows<Tin>, Tout, V>), dim3(l.long_grid), dim3(kNT), 0, st, x, out, a);
    }
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

}  // namespace

extern "C" spp_status spp_graph_gat_forward(const spp_graph_gat_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                            void* stream) {
  const char* who = "spp_graph_gat_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_gat_desc& d = *desc;
  const Common c{d.x_elem, d.out_elem,    d.rowptr_dev,     d.col_dev,     d.x_stride_elems, d.x_rows,
                 d.F,      d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,        d.out_stride_elems};
  const Whole w{d.x_dev, d.a_src_dev, d.a_dst_dev};
  return forward(who, c, {d.heads, d.relu, d.negative_slope}, &w, nullptr, 0, workspace_dev, workspace_bytes, stream);
}

extern "C" spp_status spp_graph_gat_parts_forward(const spp_graph_gat_parts_desc* desc, void* workspace_dev,
                                                  int64_t workspace_bytes, void* stream) {
  const char* who = "spp_graph_gat_parts_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_gat_parts_desc& d = *desc;
  Parts parts;
  SPP_TRY(check_parts(who, d.num_parts, d.part_offsets, d.h_parts_dev, "h base (h_parts_dev)",
                      reinterpret_cast<const void* const*>(d.a_parts_dev), "logits base (a_parts_dev)", &parts));
  SPP_REQUIRE(d.a_stride_elems >= 0, "%s: a_stride_elems %lld is negative", who, (long long)d.a_stride_elems);
  const Common c{d.x_elem, d.out_elem,    d.rowptr_dev,     d.col_dev,     d.x_stride_elems, d.part_offsets[d.num_parts],
                 d.F,      d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,        d.out_stride_elems};
  return forward(who, c, {d.heads, d.relu, d.negative_slope}, nullptr, &parts, d.a_stride_elems, workspace_dev,
                 workspace_bytes, stream);
}
