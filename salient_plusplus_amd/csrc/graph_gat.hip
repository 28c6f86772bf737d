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

// the state of target t's entries col[b .. e) (every entry equal to t skipped), columns c.. of head hd, continued
// from st in CSR order; four rows and their logits are in flight.  An entry outside [0, x_rows) is node 0: its row,
// its logit, and the comparison with t.
template <typename Tin, bool VEC4>
__device__ __forceinline__ void walk(State<VEC4>& st, const Args& a, const Tin* __restrict__ x, int64_t t, float ad,
                                     int hd, int64_t b, int64_t e, int64_t c) {
  using P = Piece<VEC4>;
  auto node = [&](int64_t k) {
    const int64_t j = a.col[k];
    return (uint64_t)j < (uint64_t)a.x_rows ? j : (int64_t)0;
  };
  int64_t k = b;
  for (; k + 3 < e; k += 4) {
    const int64_t j0 = node(k), j1 = node(k + 1), j2 = node(k + 2), j3 = node(k + 3);
    const float s0 = a.a_src[j0 * a.H + hd], s1 = a.a_src[j1 * a.H + hd], s2 = a.a_src[j2 * a.H + hd],
                s3 = a.a_src[j3 * a.H + hd];
    const auto v0 = P::load(x + j0 * a.x_stride + c), v1 = P::load(x + j1 * a.x_stride + c),
               v2 = P::load(x + j2 * a.x_stride + c), v3 = P::load(x + j3 * a.x_stride + c);
    if (j0 != t) st.take(lrelu(s0 + ad, a.slope), v0);
    if (j1 != t) st.take(lrelu(s1 + ad, a.slope), v1);
    if (j2 != t) st.take(lrelu(s2 + ad, a.slope), v2);
    if (j3 != t) st.take(lrelu(s3 + ad, a.slope), v3);
  }
  for (; k < e; ++k) {
    const int64_t j = node(k);
    const float s = a.a_src[j * a.H + hd];
    const auto v = P::load(x + j * a.x_stride + c);
    if (j != t) st.take(lrelu(s + ad, a.slope), v);
  }
}

// the self loop's state of target t (inside the graph)
template <typename Tin, bool VEC4>
__device__ __forceinline__ State<VEC4> self_state(const Args& a, const Tin* __restrict__ x, int64_t t, float ad, int hd,
                                                  int64_t c) {
  return {lrelu(a.a_src[t * a.H + hd] + ad, a.slope), 1.f, Piece<VEC4>::load(x + t * a.x_stride + c)};
}

template <typename Tout, bool VEC4>
__device__ __forceinline__ void finish(const Args& a, const State<VEC4>& st, Tout* o, int64_t c) {
  using P = Piece<VEC4>;
  const auto r = P::over(st.acc, st.s);
  P::store(o + c, a.relu ? P::relu(r) : r);
}

template <typename Tin, typename Tout, bool VEC4>
__global__ __launch_bounds__(kNT) void k_graph_gat_rows(const Tin* __restrict__ x, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
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
  for (int64_t c = (int64_t)lane * P::kWidth; c < a.F; c += (int64_t)lpr * P::kWidth) {
    const int hd = (int)c / a.C;
    const float ad = a.a_dst[t * a.H + hd];
    State<VEC4> st = self_state<Tin, VEC4>(a, x, t, ad, hd, c);
    walk<Tin, VEC4>(st, a, x, t, ad, hd, b, e, c);
    finish<Tout, VEC4>(a, st, o, c);
  }
}

template <typename Tin, typename Tout, bool VEC4>
__global__ __launch_bounds__(kNT) void k_graph_gat_long(const Tin* __restrict__ x, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
  using piece = typename P::type;
  __shared__ piece part_acc[2][kNT];
  __shared__ float part_m[2][kNT], part_s[2][kNT];
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
    for (int64_t c0 = 0; c0 < a.F; c0 += (int64_t)lpr * P::kWidth) {
      const int64_t c = c0 + (int64_t)lane * P::kWidth;
      const bool active = c < a.F;
      const int hd = active ? (int)c / a.C : 0;
      const float ad = a.a_dst[t * a.H + hd];
      State<VEC4> total = State<VEC4>::empty();  // (set from chunk 0's state in the first round)
      for (int64_t j0 = 0; j0 < chunks; j0 += groups, ++round) {
        // group g runs chunk j0 + g; round k parks its states in part_*[k & 1], which are written again in round
        // k + 2, behind the barrier of round k + 1 that group 0 reaches after it has read them
        const int64_t j = j0 + grp;
        State<VEC4> st = State<VEC4>::empty();
        if (active && j < chunks) {
          const int64_t cb = b + j * kGatChunk;
          if (j == 0) st = self_state<Tin, VEC4>(a, x, t, ad, hd, c);
          walk<Tin, VEC4>(st, a, x, t, ad, hd, cb, std::min<int64_t>(e, cb + kGatChunk), c);
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

extern "C" spp_status spp_graph_gat_forward(const spp_graph_gat_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                            void* stream) {
  const char* who = "spp_graph_gat_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_gat_desc& d = *desc;
  SPP_REQUIRE(d.x_elem != SPP_ELEM_FP8_E4M3 && d.out_elem != SPP_ELEM_FP8_E4M3,
              "%s: fp8 rows are not read or written here (x_elem %d, out_elem %d)", who, (int)d.x_elem, (int)d.out_elem);
  SPP_REQUIRE((d.x_elem == SPP_ELEM_F32 || d.x_elem == SPP_ELEM_F16 || d.x_elem == SPP_ELEM_BF16) &&
                  (d.out_elem == SPP_ELEM_F32 || d.out_elem == SPP_ELEM_BF16),
              "%s: unknown or unsupported element code (x_elem %d, out_elem %d)", who, (int)d.x_elem, (int)d.out_elem);
  const bool by_ids = d.target_ids_dev != nullptr, by_slab = d.target_row0 >= 0;
  SPP_REQUIRE(by_ids != by_slab, "%s: give the targets as a slab (target_row0 >= 0) or as a list (target_ids_dev), %s", who,
              by_ids ? "not both" : "one of them");
  const int64_t T = d.num_targets, F = d.F;
  SPP_REQUIRE(T >= 0 && F >= 0 && d.x_rows >= 0, "%s: negative size (num_targets, F or x_rows)", who);
  SPP_REQUIRE(by_ids || (d.target_row0 <= d.x_rows && T <= d.x_rows - d.target_row0),
              "%s: the slab [%lld, %lld) (target_row0, num_targets) leaves the graph's %lld rows", who,
              (long long)d.target_row0, (long long)(d.target_row0 + T), (long long)d.x_rows);
  SPP_REQUIRE(d.heads >= 1 && F % d.heads == 0 && F < (1ll << 31), "%s: heads %d must be positive and divide F = %lld (< 2^31)",
              who, (int)d.heads, (long long)F);
  const int64_t out_stride = d.out_stride_elems > 0 ? d.out_stride_elems : F;
  SPP_REQUIRE(out_stride >= F, "%s: out_stride_elems smaller than the output row", who);
  SPP_REQUIRE(d.x_stride_elems >= F, "%s: x_stride_elems smaller than the row", who);
  // the vector form: four columns of one head per lane.  Rows of h that do not allow it are read one column per lane
  // instead; an output that does not is refused (the caller allocates it)
  const int64_t Cw = F / d.heads;
  const bool vec = F > 0 && Cw % 4 == 0 && d.x_stride_elems % 4 == 0 && aligned_to(d.x_dev, 4 * elem_bytes(d.x_elem));
  SPP_REQUIRE(!vec || (out_stride % 4 == 0 && aligned_to(d.out_dev, 4 * elem_bytes(d.out_elem))),
              "%s: C %% 4 == 0 needs out_dev aligned to 4 elements (base and stride)", who);
  SPP_REQUIRE(workspace_dev && aligned_to(workspace_dev, 16) && workspace_bytes >= spp_graph_gat_workspace_bytes(T),
              "%s: needs a 16-byte aligned workspace of spp_graph_gat_workspace_bytes(num_targets) = %lld bytes", who,
              (long long)spp_graph_gat_workspace_bytes(T));
  if (T == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr_dev && d.col_dev && d.x_dev && d.a_src_dev && d.a_dst_dev && d.out_dev && d.x_rows > 0,
              "%s: NULL buffer or empty graph", who);
  const int lpr_log2 = lanes_log2(vec ? F / 4 : F);
  const int64_t grid = ceil_div(T << lpr_log2, kNT);
  SPP_REQUIRE(grid < (1ll << 31), "%s: too many targets for one launch (num_targets %lld)", who, (long long)T);
  hipStream_t st = as_stream(stream);
  Args a{};
  a.rowptr = d.rowptr_dev, a.col = d.col_dev, a.ids = d.target_ids_dev, a.row0 = by_ids ? 0 : d.target_row0, a.T = T;
  a.x_stride = d.x_stride_elems, a.x_rows = d.x_rows, a.F = F, a.out_stride = out_stride;
  a.a_src = d.a_src_dev, a.a_dst = d.a_dst_dev, a.H = d.heads, a.C = (int32_t)Cw;
  a.slope = d.negative_slope, a.relu = d.relu != 0, a.lpr_log2 = lpr_log2;
  a.counter = static_cast<unsigned long long*>(workspace_dev);
  a.list = reinterpret_cast<int64_t*>(static_cast<char*>(workspace_dev) + kWorkspaceHeader);
  SPP_HIP_TRY(hipMemsetAsync(workspace_dev, 0, kWorkspaceHeader, st));
  const unsigned long_grid = (unsigned)std::min<int64_t>(T, kLongGrid);
  auto launch = [&](auto tin, auto tout, auto v) {
    using Tin = typename decltype(tin)::type;
    using Tout = typename decltype(tout)::type;
    constexpr bool V = decltype(v)::value;
    const Tin* x = static_cast<const Tin*>(d.x_dev);
    Tout* out = static_cast<Tout*>(d.out_dev);
    hipLaunchKernelGGL((k_graph_gat_rows<Tin, Tout, V>), dim3((unsigned)grid), dim3(kNT), 0, st, x, out, a);
    hipLaunchKernelGGL((k_graph_gat_long<Tin, Tout, V>), dim3(long_grid), dim3(kNT), 0, st, x, out, a);
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
