// f3h: GATConv attention over rows of the RESIDENT graph -- the message passing of exact, layer-wise GAT inference
// (reference: driver/models.py:228 GAT.inference through layerwise_inference, line 441), in PyG's project-first order:
//     e^h_tj = leaky_relu(a_src[j,h] + a_dst[t,h], slope)     j in col[rowptr[t] .. rowptr[t+1]) without j == t, plus j = t
//     out[i, h*C + c] = sum_j softmax_j(e^h_t.)_j * h[j, h*C + c]          t = target_row0 + i  or  target_ids[i]
// What differs from a sampled hop (aggregate.hip, k_gat_fwd / k_gat_mh_agg_fwd): the targets are any rows of h, a row
// is as long as the node's degree, and the rows of h are already projected, so a head owns C columns of the row.
//
// Softmax contract (include/spp.h, spp_graph_gat_forward): C_g = kGatChunk.  A state is (m, s, acc): the running
// maximum, the denominator and the weighted sum at that maximum.  A row of at most C_g raw entries is ONE online
// softmax in CSR order from the self loop's state (m = e_self, s = 1, acc = h_t): k_gat_fwd's arithmetic.  A longer
// row is cut into consecutive chunks of C_g raw positions; chunk 0 starts from the self loop's state, every other
// chunk from the empty state (m = -inf, s = 0, acc = 0), and the chunk states are merged in chunk order.  Nothing else
// enters: not the grid, not the slab, not the list order, not the other rows of the launch.
//
// Load balance, two launches on the stream and no host wait (graph_aggregate.hip's shape):
//   k_graph_gat_rows  lpr lanes per target finish every row of at most C_g raw entries; lane 0 of a longer row appends
//                     its OUTPUT index to a list in the caller's workspace (one atomic on a counter the entry zeroes).
//   k_graph_gat_long  one workgroup per listed row: its 256 / lpr lane groups run 256 / lpr chunks at a time, park the
//                     chunk STATES in LDS, and group 0 merges them in chunk order (double-buffered: one barrier a round).
// Every lane keeps the state of the head its columns belong to (head = column / C at run time); all lanes of a head
// walk the same entries, so the states need no exchange.  Every offset is 64-bit.  No atomics touch the output.
// (load4 / Piece / NodeRows are restated from graph_aggregate.hip, which stays as it is.)
//
// f3k: the same two kernels over a ROW-PARTITIONED h with its logits (spp_graph_gat_parts_forward).  The row source is a
// template parameter: NodeRows reads one matrix h and the two logit matrices, PartRows finds the part that owns a
// global row first and takes the row of h AND the row of [a_src | a_dst] from that one lookup.  Same arithmetic, same
// order, same bits.
#include "spp_internal.h"

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <type_traits>

namespace spp {
namespace graph_gat {

constexpr int kNT = 256;
constexpr int64_t kGatChunk = 64;             // C_g
constexpr int64_t kWorkspaceHeader = 16;      // the counter (8 bytes) and padding; the list follows
constexpr unsigned kLongGrid = 16384;         // workgroups of the long-row launch (they stride over the list)

using bf16 = __hip_bfloat16;
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

struct f4 {
  float x, y, z, w;
};

// loads convert to fp32 exactly; a bf16 store rounds once, to nearest even
__device__ __forceinline__ f4 load4(const float* p) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  return {v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ f4 load4(const __half* p) {
  const uint2 raw = *reinterpret_cast<const uint2*>(p);
  const __half2 a = *reinterpret_cast<const __half2*>(&raw.x), b = *reinterpret_cast<const __half2*>(&raw.y);
  const float2 fa = __half22float2(a), fb = __half22float2(b);
  return {fa.x, fa.y, fb.x, fb.y};
}
__device__ __forceinline__ f4 load4(const bf16* p) {
  const uint2 raw = *reinterpret_cast<const uint2*>(p);
  return {__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xffff0000u), __uint_as_float(raw.y << 16),
          __uint_as_float(raw.y & 0xffff0000u)};
}
__device__ __forceinline__ float load1(const float* p) { return *p; }
__device__ __forceinline__ float load1(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float load1(const bf16* p) {
  return __uint_as_float((uint32_t)*reinterpret_cast<const uint16_t*>(p) << 16);
}
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));
}
__device__ __forceinline__ void store4(float* p, f4 v) { *reinterpret_cast<float4*>(p) = make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void store4(bf16* p, f4 v) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
}
__device__ __forceinline__ void store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void store1(bf16* p, float v) { *p = __float2bfloat16(v); }

// the piece of a row one lane holds: four columns of one head (vector form) or one column
template <bool VEC4>
struct Piece {
  using type = f4;
  static constexpr int kWidth = 4;
  template <typename T> static __device__ __forceinline__ f4 load(const T* p) { return load4(p); }
  template <typename T> static __device__ __forceinline__ void store(T* p, f4 v) { store4(p, v); }
  static __device__ __forceinline__ f4 zero() { return {0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ f4 scaled(f4 a, float s) { return {a.x * s, a.y * s, a.z * s, a.w * s}; }
  static __device__ __forceinline__ f4 fma(float s, f4 o, f4 a) {
    return {fmaf(s, o.x, a.x), fmaf(s, o.y, a.y), fmaf(s, o.z, a.z), fmaf(s, o.w, a.w)};
  }
  static __device__ __forceinline__ f4 over(f4 a, float s) { return {a.x / s, a.y / s, a.z / s, a.w / s}; }
  static __device__ __forceinline__ f4 relu(f4 a) { return {fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f)}; }
};
template <>
struct Piece<false> {
  using type = float;
  static constexpr int kWidth = 1;
  template <typename T> static __device__ __forceinline__ float load(const T* p) { return load1(p); }
  template <typename T> static __device__ __forceinline__ void store(T* p, float v) { store1(p, v); }
  static __device__ __forceinline__ float zero() { return 0.f; }
  static __device__ __forceinline__ float scaled(float a, float s) { return a * s; }
  static __device__ __forceinline__ float fma(float s, float o, float a) { return fmaf(s, o, a); }
  static __device__ __forceinline__ float over(float a, float s) { return a / s; }
  static __device__ __forceinline__ float relu(float a) { return fmaxf(a, 0.f); }
};

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

struct Args {
  const int64_t* rowptr;
  const int64_t* col;
  const int64_t* ids;   // NULL: the slab row0 .. row0 + T
  int64_t row0, T;
  int64_t x_stride, x_rows, F;
  int64_t out_stride;
  const float* a_src;   // [x_rows, H]
  const float* a_dst;   // [x_rows, H]
  int32_t H, C;         // heads, columns per head (F = H * C)
  float slope;
  int32_t relu;
  int lpr_log2;
  unsigned long long* counter;
  int64_t* list;
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

// h and the logits as up to kMaxParts row ranges, each pair in allocations of its own (a rank's buffers, mapped into
// this process).  Entry p holds the first global row of the p-th NON-EMPTY part, its h base moved back by that many
// rows of h and its logits base ([rows, a_stride] fp32, a_src in columns [0, H), a_dst in [H, 2H)) moved back by that
// many rows of logits, so that row g of every part is base + g * stride; the entries behind the last part start at
// INT64_MAX (no row reaches them).  The launch passes the table by value.  Indexing that argument block with a per-lane
// owner would make the compiler keep a private copy of it in scratch, and a scalar loop over it
// was measured at 2.1-2.3 times NodeRows for the plain aggregation (f3j).  So thread 0 copies the three tables into LDS
// (384 bytes) once per workgroup, with compile-time indices, and a lane finds the owner by a branch-free binary search
// there: four dependent 8-byte LDS reads, then one for each base.  One search serves the row and its logit.
constexpr int kMaxParts = SPP_GRAPH_AGG_MAX_PARTS;
static_assert(kMaxParts == 16, "PartRows::owner searches exactly 16 entries");
template <typename Tin>
struct PartTable {
  int64_t first[kMaxParts];
  const Tin* h[kMaxParts];
  const float* a[kMaxParts];
  int64_t a_stride;
};
template <typename Tin>
struct PartRows {
  using elem = Tin;
  using Src = PartTable<Tin>;
  using Owner = int;
  const int64_t* first;       // LDS
  const Tin* const* hb;       // LDS
  const float* const* ab;     // LDS
  int64_t stride, a_stride;
  int H;
  // every thread of the workgroup constructs it, before any of them leaves the kernel (a barrier inside)
  __device__ __forceinline__ PartRows(const PartTable<Tin>& src, const Args& a)
      : stride(a.x_stride), a_stride(src.a_stride), H(a.H) {
    __shared__ int64_t lds_first[kMaxParts];
    __shared__ const Tin* lds_h[kMaxParts];
    __shared__ const float* lds_a[kMaxParts];
    if (threadIdx.x == 0) {
#pragma unroll
      for (int p = 0; p < kMaxParts; ++p) lds_first[p] = src.first[p], lds_h[p] = src.h[p], lds_a[p] = src.a[p];
    }
    __syncthreads();
    first = lds_first, hb = lds_h, ab = lds_a;
  }
  __device__ __forceinline__ Owner owner(int64_t g) const {
    int p = g >= first[8] ? 8 : 0;  // the last entry with first <= g (first[0] = 0)
    p += g >= first[p + 4] ? 4 : 0;
    p += g >= first[p + 2] ? 2 : 0;
    p += g >= first[p + 1] ? 1 : 0;
    return p;
  }
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
  const int64_t t = a.ids ? a.ids[i] : a.row0 + i;
  Tout* o = out + i * a.out_stride;
  if ((uint64_t)t >= (uint64_t)a.x_rows) {  // a target outside the graph: a row of zeros
    for (int64_t c = (int64_t)lane * P::kWidth; c < a.F; c += (int64_t)lpr * P::kWidth) P::store(o + c, P::zero());
    return;
  }
  const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
  if (e - b > kGatChunk) {  // a long row: k_graph_gat_long's
    if (lane == 0) a.list[atomicAdd(a.counter, 1ull)] = i;
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
  const int64_t n = (int64_t)*a.counter;
  unsigned round = 0;  // (workgroup-uniform, as every loop bound below: all 256 threads reach every barrier)
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = a.list[r];
    const int64_t t = a.ids ? a.ids[i] : a.row0 + i;  // (inside the graph: the row was found long)
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

static int lanes_log2(int64_t pieces) {
  int l = 0;
  while ((1 << l) < pieces && l < 6) ++l;
  return l;
}
static int64_t elem_bytes(int32_t elem) { return elem == SPP_ELEM_F32 ? 4 : 2; }
static bool aligned_to(const void* p, int64_t bytes) { return reinterpret_cast<uintptr_t>(p) % (uintptr_t)bytes == 0; }

template <typename T> struct Type { using type = T; };

}  // namespace graph_gat
}  // namespace spp

using namespace spp;
using namespace spp::graph_gat;

extern "C" int64_t spp_graph_gat_chunk(void) { return kGatChunk; }

extern "C" int64_t spp_graph_gat_workspace_bytes(int64_t num_targets) {
  return kWorkspaceHeader + 8 * std::max<int64_t>(num_targets, 0);
}

namespace {

// what both entries share: spp_graph_gat_desc without its sources
struct Call {
  int32_t x_elem, out_elem, heads, relu;
  const int64_t* rowptr;
  const int64_t* col;
  int64_t x_stride, x_rows, F, row0;
  const int64_t* ids;
  int64_t T;
  void* out;
  int64_t out_stride;
  float slope;
};

// the sources of spp_graph_gat_forward: one matrix h and the two logit matrices
struct Whole {
  const void* x;
  const float* a_src;
  const float* a_dst;
};

// the sources of spp_graph_gat_parts_forward: the non-empty parts in order
struct Parts {
  int n;
  int64_t first[kMaxParts];
  const void* h[kMaxParts];
  const float* a[kMaxParts];
  int64_t a_stride;  // as given: 0 = dense
};

// exactly one of whole / parts is given
spp_status forward(const char* who, const Call& d, const Whole* whole, const Parts* parts, void* workspace_dev,
                   int64_t workspace_bytes, void* stream) {
  SPP_REQUIRE(d.x_elem != SPP_ELEM_FP8_E4M3 && d.out_elem != SPP_ELEM_FP8_E4M3,
              "%s: fp8 rows are not read or written here (x_elem %d, out_elem %d)", who, (int)d.x_elem, (int)d.out_elem);
  SPP_REQUIRE((d.x_elem == SPP_ELEM_F32 || d.x_elem == SPP_ELEM_F16 || d.x_elem == SPP_ELEM_BF16) &&
                  (d.out_elem == SPP_ELEM_F32 || d.out_elem == SPP_ELEM_BF16),
              "%s: unknown or unsupported element code (x_elem %d, out_elem %d)", who, (int)d.x_elem, (int)d.out_elem);
  const bool by_ids = d.ids != nullptr, by_slab = d.row0 >= 0;
  SPP_REQUIRE(by_ids != by_slab, "%s: give the targets as a slab (target_row0 >= 0) or as a list (target_ids_dev), %s", who,
              by_ids ? "not both" : "one of them");
  const int64_t T = d.T, F = d.F;
  SPP_REQUIRE(T >= 0 && F >= 0 && d.x_rows >= 0, "%s: negative size (num_targets, F or x_rows)", who);
  SPP_REQUIRE(by_ids || (d.row0 <= d.x_rows && T <= d.x_rows - d.row0),
              "%s: the slab [%lld, %lld) (target_row0, num_targets) leaves the graph's %lld rows", who,
              (long long)d.row0, (long long)(d.row0 + T), (long long)d.x_rows);
  SPP_REQUIRE(d.heads >= 1 && F % d.heads == 0 && F < (1ll << 31), "%s: heads %d must be positive and divide F = %lld (< 2^31)",
              who, (int)d.heads, (long long)F);
  SPP_REQUIRE(!parts || parts->a_stride == 0 || parts->a_stride >= 2 * (int64_t)d.heads,
              "%s: a_stride_elems %lld smaller than the logits' row of 2 * heads = %d", who,
              parts ? (long long)parts->a_stride : 0ll, 2 * (int)d.heads);
  const int64_t out_stride = d.out_stride > 0 ? d.out_stride : F;
  SPP_REQUIRE(out_stride >= F, "%s: out_stride_elems smaller than the output row", who);
  SPP_REQUIRE(d.x_stride >= F, "%s: x_stride_elems smaller than the row", who);
  // the vector form: four columns of one head per lane.  Rows of h that do not allow it (with parts: the rows of any of
  // them) are read one column per lane instead; an output that does not is refused (the caller allocates it)
  const int64_t Cw = F / d.heads;
  bool vec = F > 0 && Cw % 4 == 0 && d.x_stride % 4 == 0;
  if (parts)
    for (int p = 0; p < parts->n; ++p) vec = vec && aligned_to(parts->h[p], 4 * elem_bytes(d.x_elem));
  else
    vec = vec && aligned_to(whole->x, 4 * elem_bytes(d.x_elem));
  SPP_REQUIRE(!vec || (out_stride % 4 == 0 && aligned_to(d.out, 4 * elem_bytes(d.out_elem))),
              "%s: C %% 4 == 0 needs out_dev aligned to 4 elements (base and stride)", who);
  SPP_REQUIRE(workspace_dev && aligned_to(workspace_dev, 16) && workspace_bytes >= spp_graph_gat_workspace_bytes(T),
              "%s: needs a 16-byte aligned workspace of spp_graph_gat_workspace_bytes(num_targets) = %lld bytes", who,
              (long long)spp_graph_gat_workspace_bytes(T));
  if (T == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr && d.col && (parts || (whole->x && whole->a_src && whole->a_dst)) && d.out && d.x_rows > 0,
              "%s: NULL buffer or empty graph", who);
  const int lpr_log2 = lanes_log2(vec ? F / 4 : F);
  const int64_t grid = ceil_div(T << lpr_log2, kNT);
  SPP_REQUIRE(grid < (1ll << 31), "%s: too many targets for one launch (num_targets %lld)", who, (long long)T);
  hipStream_t st = as_stream(stream);
  Args a{};
  a.rowptr = d.rowptr, a.col = d.col, a.ids = d.ids, a.row0 = by_ids ? 0 : d.row0, a.T = T;
  a.x_stride = d.x_stride, a.x_rows = d.x_rows, a.F = F, a.out_stride = out_stride;
  a.a_src = parts ? nullptr : whole->a_src, a.a_dst = parts ? nullptr : whole->a_dst, a.H = d.heads, a.C = (int32_t)Cw;
  a.slope = d.slope, a.relu = d.relu != 0, a.lpr_log2 = lpr_log2;
  a.counter = static_cast<unsigned long long*>(workspace_dev);
  a.list = reinterpret_cast<int64_t*>(static_cast<char*>(workspace_dev) + kWorkspaceHeader);
  SPP_HIP_TRY(hipMemsetAsync(workspace_dev, 0, kWorkspaceHeader, st));
  const unsigned long_grid = (unsigned)std::min<int64_t>(T, kLongGrid);
  auto launch = [&](auto tin, auto tout, auto v) {
    using Tin = typename decltype(tin)::type;
    using Tout = typename decltype(tout)::type;
    constexpr bool V = decltype(v)::value;
    Tout* out = static_cast<Tout*>(d.out);
    if (parts) {
      // each base moved back by its part's first row (never dereferenced below that row; integer arithmetic, the
      // address may lie before the allocation)
      PartTable<Tin> t{};
      t.a_stride = parts->a_stride > 0 ? parts->a_stride : 2 * (int64_t)d.heads;
      for (int p = 0; p < kMaxParts; ++p) t.first[p] = INT64_MAX;  // (behind the last part: never the owner)
      for (int p = 0; p < parts->n; ++p) {
        t.first[p] = parts->first[p];
        t.h[p] = reinterpret_cast<const Tin*>(reinterpret_cast<uintptr_t>(parts->h[p]) -
                                              (uintptr_t)parts->first[p] * (uintptr_t)d.x_stride * sizeof(Tin));
        t.a[p] = reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(parts->a[p]) -
                                                (uintptr_t)parts->first[p] * (uintptr_t)t.a_stride * sizeof(float));
      }
      hipLaunchKernelGGL((k_graph_gat_rows<PartRows<Tin>, Tout, V>), dim3((unsigned)grid), dim3(kNT), 0, st, t, out, a);
      hipLaunchKernelGGL((k_graph_gat_long<PartRows<Tin>, Tout, V>), dim3(long_grid), dim3(kNT), 0, st, t, out, a);
    } else {
      const Tin* x = static_cast<const Tin*>(whole->x);
      hipLaunchKernelGGL((k_graph_gat_rows<NodeRows<Tin>, Tout, V>), dim3((unsigned)grid), dim3(kNT), 0, st, x, out, a);
      hipLaunchKernelGGL((k_graph_gat_long<NodeRows<Tin>, Tout, V>), dim3(long_grid), dim3(kNT), 0, st, x, out, a);
    }
  };
  auto by_out = [&](auto tin, auto v) {
    d.out_elem == SPP_ELEM_BF16 ? launch(tin, Type<bf16>{}, v) : launch(tin, Type<float>{}, v);
  };
  auto by_in = [&](auto v) {
    d.x_elem == SPP_ELEM_BF16 ? by_out(Type<bf16>{}, v) : d.x_elem == SPP_ELEM_F16 ? by_out(Type<__half>{}, v)
                                                                                   : by_out(Type<float>{}, v);
  };
  vec ? by_in(std::true_type{}) : by_in(std::false_type{});
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

}  // namespace

extern "C" spp_status spp_graph_gat_forward(const spp_graph_gat_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                            void* stream) {
  const char* who = "spp_graph_gat_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_gat_desc& d = *desc;
  const Call c{d.x_elem, d.out_elem,    d.heads,          d.relu,        d.rowptr_dev, d.col_dev,          d.x_stride_elems,
               d.x_rows, d.F,           d.target_row0,    d.target_ids_dev, d.num_targets, d.out_dev, d.out_stride_elems,
               d.negative_slope};
  const Whole w{d.x_dev, d.a_src_dev, d.a_dst_dev};
  return forward(who, c, &w, nullptr, workspace_dev, workspace_bytes, stream);
}

extern "C" spp_status spp_graph_gat_parts_forward(const spp_graph_gat_parts_desc* desc, void* workspace_dev,
                                                  int64_t workspace_bytes, void* stream) {
  const char* who = "spp_graph_gat_parts_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_gat_parts_desc& d = *desc;
  SPP_REQUIRE(d.num_parts >= 1 && d.num_parts <= SPP_GRAPH_AGG_MAX_PARTS, "%s: num_parts %d outside 1..%d", who,
              (int)d.num_parts, (int)SPP_GRAPH_AGG_MAX_PARTS);
  SPP_REQUIRE(d.part_offsets[0] == 0, "%s: part_offsets[0] must be 0, got %lld", who, (long long)d.part_offsets[0]);
  SPP_REQUIRE(d.a_stride_elems >= 0, "%s: a_stride_elems %lld is negative", who, (long long)d.a_stride_elems);
  Parts parts{};
  parts.a_stride = d.a_stride_elems;
  for (int p = 0; p < d.num_parts; ++p) {
    SPP_REQUIRE(d.part_offsets[p + 1] >= d.part_offsets[p], "%s: part_offsets decrease at part %d (%lld after %lld)", who, p,
                (long long)d.part_offsets[p + 1], (long long)d.part_offsets[p]);
    if (d.part_offsets[p + 1] == d.part_offsets[p]) continue;  // an empty part owns no row: its bases may be NULL
    SPP_REQUIRE(d.h_parts_dev[p], "%s: part %d holds the rows [%lld, %lld) and its h base (h_parts_dev) is NULL", who, p,
                (long long)d.part_offsets[p], (long long)d.part_offsets[p + 1]);
    SPP_REQUIRE(d.a_parts_dev[p], "%s: part %d holds the rows [%lld, %lld) and its logits base (a_parts_dev) is NULL", who,
                p, (long long)d.part_offsets[p], (long long)d.part_offsets[p + 1]);
    parts.first[parts.n] = d.part_offsets[p], parts.h[parts.n] = d.h_parts_dev[p], parts.a[parts.n] = d.a_parts_dev[p];
    ++parts.n;
  }
  const Call c{d.x_elem, d.out_elem, d.heads, d.relu, d.rowptr_dev, d.col_dev, d.x_stride_elems,
               d.part_offsets[d.num_parts], d.F, d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,
               d.out_stride_elems, d.negative_slope};
  return forward(who, c, nullptr, &parts, workspace_dev, workspace_bytes, stream);
}
