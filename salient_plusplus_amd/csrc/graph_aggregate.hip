// f3g: mean / operand / sum aggregation over rows of the RESIDENT graph's CSR -- the message passing of exact,
// layer-wise inference (reference: driver/models.py:441 layerwise_inference with SAGE.inference):
//     out[i,:] = epilogue( sum_{k in [rowptr[t], rowptr[t+1])} x[col[k],:] ),   t = target_row0 + i  or  target_ids[i]
// Two things differ from a sampled hop (aggregate.hip, k_agg_fwd): the targets are any rows of x, not its first ones,
// and a row is as long as the node's degree -- a hub of 10^5 neighbours next to a median of tens.
//
// Summation contract (include/spp.h, spp_graph_agg_forward): C = kGraphChunk.  A row of d <= C entries is summed in
// CSR order, one addend at a time, in fp32: the arithmetic of k_agg_fwd.  A longer row is cut into consecutive chunks
// of C entries (the last may be shorter), each chunk is summed that way from zero, and the chunk sums are added in
// chunk order.  Nothing else enters: not the grid, not the slab, not the other rows of the launch.
//
// Load balance, two launches on the stream and no host wait:
//   k_graph_agg_rows  lpr lanes per target (k_agg_fwd's shape) finish every row of d <= C; the lanes of a longer row
//                     append its OUTPUT index to a list in the caller's workspace (one atomic on a counter the entry
//                     zeroes; the list's order varies from run to run, the result of a row does not depend on it).
//   k_graph_agg_long  one workgroup per listed row: its 256 / lpr lane groups sum 256 / lpr chunks at a time, park the
//                     chunk sums in LDS, and group 0 adds them in chunk order (double-buffered: one barrier a round).
// Every offset is 64-bit (N * F reaches 2.8e10 elements at papers scale).  No atomics touch the output.
//
// f3j: the same two kernels over a ROW-PARTITIONED x (spp_graph_agg_parts_forward).  The row source is a template
// parameter: NodeRows reads one matrix, PartRows finds the part that owns a global row first.  Same arithmetic, same
// order, same bits.
#include "spp_internal.h"

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <type_traits>

namespace spp {
namespace graph_agg {

constexpr int kNT = 256;
constexpr int64_t kGraphChunk = 64;           // C
constexpr int64_t kWorkspaceHeader = 16;      // the counter (8 bytes) and padding; the list follows
constexpr unsigned kLongGrid = 16384;         // workgroups of the long-row launch (they stride over the list)

using bf16 = __hip_bfloat16;
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

struct f4 {
  float x, y, z, w;
};

// loads convert to fp32 exactly; a bf16 store rounds once, to nearest even (the rule of spp_agg_forward)
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

// the piece of a row one lane holds: four columns (vector form) or one
template <bool VEC4>
struct Piece {
  using type = f4;
  static constexpr int kWidth = 4;
  template <typename T> static __device__ __forceinline__ f4 load(const T* p) { return load4(p); }
  template <typename T> static __device__ __forceinline__ void store(T* p, f4 v) { store4(p, v); }
  static __device__ __forceinline__ f4 zero() { return {0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ void add(f4& a, f4 v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
  static __device__ __forceinline__ f4 scaled(f4 a, float s) { return {a.x * s, a.y * s, a.z * s, a.w * s}; }
  static __device__ __forceinline__ f4 fma(float s, f4 o, f4 a) {
    return {fmaf(s, o.x, a.x), fmaf(s, o.y, a.y), fmaf(s, o.z, a.z), fmaf(s, o.w, a.w)};
  }
};
template <>
struct Piece<false> {
  using type = float;
  static constexpr int kWidth = 1;
  template <typename T> static __device__ __forceinline__ float load(const T* p) { return load1(p); }
  template <typename T> static __device__ __forceinline__ void store(T* p, float v) { store1(p, v); }
  static __device__ __forceinline__ float zero() { return 0.f; }
  static __device__ __forceinline__ void add(float& a, float v) { a += v; }
  static __device__ __forceinline__ float scaled(float a, float s) { return a * s; }
  static __device__ __forceinline__ float fma(float s, float o, float a) { return fmaf(s, o, a); }
};

struct Args;

// The row source of the kernels: Rows::Src is what the launch passes by value, Rows(src, a) what a lane asks for the
// address of global row g.
// row g of the full matrix; an id outside [0, x_rows) reads row 0 (the rule of the Table source: no fault)
template <typename Tin>
struct NodeRows {
  using elem = Tin;
  using Src = const Tin* __restrict__;
  const Tin* x;
  int64_t stride, rows;
  __device__ __forceinline__ NodeRows(const Tin* src, const Args& a);
  __device__ __forceinline__ const Tin* operator()(int64_t g) const {
    return x + ((uint64_t)g < (uint64_t)rows ? g : 0) * stride;
  }
};

// The matrix as up to kMaxParts row ranges, each in an allocation of its own (a rank's partition, mapped into this
// process): entry p holds the first global row of the p-th NON-EMPTY part and its base moved back by that many rows, so
// that row g of every part is base + g * stride; the entries behind the last part start at INT64_MAX (no row reaches
// them).  The launch passes the table by value.  Indexing that argument block with a per-lane owner would make the
// compiler keep a private copy of it in scratch, and walking it entry by entry with scalar loads
// puts two dependent scalar-load waits per entry in front of every row fetch (measured: 2.1-2.3 times the time of
// NodeRows).  So thread 0 copies the table into LDS once per workgroup, with compile-time indices, and a lane finds the
// owner by a branch-free binary search there: four dependent 8-byte LDS reads and one for the base, no loop, and the
// searches of the four rows in flight overlap.
constexpr int kMaxParts = SPP_GRAPH_AGG_MAX_PARTS;
static_assert(kMaxParts == 16, "PartRows::operator() searches exactly 16 entries");
template <typename Tin>
struct PartTable {
  int64_t first[kMaxParts];
  const Tin* base[kMaxParts];
};
template <typename Tin>
struct PartRows {
  using elem = Tin;
  using Src = PartTable<Tin>;
  const int64_t* first;     // LDS
  const Tin* const* base;   // LDS
  int64_t stride, rows;
  // every thread of the workgroup constructs it, before any of them leaves the kernel (a barrier inside)
  __device__ __forceinline__ PartRows(const PartTable<Tin>& src, const Args& a);
  __device__ __forceinline__ const Tin* operator()(int64_t g) const {
    g = (uint64_t)g < (uint64_t)rows ? g : 0;
    int p = g >= first[8] ? 8 : 0;  // the last entry with first <= g (first[0] = 0)
    p += g >= first[p + 4] ? 4 : 0;
    p += g >= first[p + 2] ? 2 : 0;
    p += g >= first[p + 1] ? 1 : 0;
    return base[p] + g * stride;
  }
};

// columns c.. of the entries [b, e), added in CSR order one at a time from zero; four rows are in flight
template <typename Rows, bool VEC4>
__device__ __forceinline__ typename Piece<VEC4>::type sum_entries(const Rows& row, const int64_t* __restrict__ col,
                                                                  int64_t b, int64_t e, int64_t c) {
  using P = Piece<VEC4>;
  typename P::type acc = P::zero();
  int64_t k = b;
  for (; k + 3 < e; k += 4) {
    const int64_t j0 = col[k], j1 = col[k + 1], j2 = col[k + 2], j3 = col[k + 3];
    const auto v0 = P::load(row(j0) + c), v1 = P::load(row(j1) + c), v2 = P::load(row(j2) + c), v3 = P::load(row(j3) + c);
    P::add(acc, v0);
    P::add(acc, v1);
    P::add(acc, v2);
    P::add(acc, v3);
  }
  for (; k < e; ++k) P::add(acc, P::load(row(col[k]) + c));
  return acc;
}

struct Args {
  const int64_t* rowptr;
  const int64_t* col;
  const int64_t* ids;   // NULL: the slab row0 .. row0 + T
  int64_t row0, T;
  int64_t x_stride, x_rows, F;
  int64_t out_stride;
  int32_t epilogue;     // SPP_AGG_MEAN / _OPERAND / _SUM
  float self_scale;
  int lpr_log2;
  unsigned long long* counter;
  int64_t* list;
};
template <typename Tin>
__device__ __forceinline__ NodeRows<Tin>::NodeRows(const Tin* src, const Args& a) : x(src), stride(a.x_stride), rows(a.x_rows) {}
template <typename Tin>
__device__ __forceinline__ PartRows<Tin>::PartRows(const PartTable<Tin>& src, const Args& a)
    : stride(a.x_stride), rows(a.x_rows) {
  __shared__ int64_t lds_first[kMaxParts];
  __shared__ const Tin* lds_base[kMaxParts];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < kMaxParts; ++p) lds_first[p] = src.first[p], lds_base[p] = src.base[p];
  }
  __syncthreads();
  first = lds_first, base = lds_base;
}

// what the sum of node t's row becomes, columns c.. of output row o (own: node t's row of x, NULL for a target id
// outside the graph, whose output row is all zeros)
template <typename Tin, typename Tout, bool VEC4>
__device__ __forceinline__ void finish(const Args& a, typename Piece<VEC4>::type acc, int64_t deg, const Tin* own,
                                       Tout* o, int64_t c) {
  using P = Piece<VEC4>;
  if (a.epilogue == SPP_AGG_SUM) {
    if (a.self_scale != 0.f && own) acc = P::fma(a.self_scale, P::load(own + c), acc);
  } else {
    acc = P::scaled(acc, 1.0f / (float)(deg > 0 ? deg : 1));
    if (a.epilogue == SPP_AGG_OPERAND) P::store(o + a.F + c, own ? P::load(own + c) : P::zero());
  }
  P::store(o + c, acc);
}

template <typename Rows, typename Tout, bool VEC4>
__global__ __launch_bounds__(kNT) void k_graph_agg_rows(typename Rows::Src src, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
  using Tin = typename Rows::elem;
  const Rows row(src, a);  // (PartRows: the whole workgroup, before anyone returns)
  const int lpr = 1 << a.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t i = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> a.lpr_log2;
  if (i >= a.T) return;
  const int64_t t = a.ids ? a.ids[i] : a.row0 + i;
  const bool in_graph = (uint64_t)t < (uint64_t)a.x_rows;
  const int64_t b = in_graph ? a.rowptr[t] : 0, e = in_graph ? a.rowptr[t + 1] : 0;
  if (e - b > kGraphChunk) {  // a long row: k_graph_agg_long's
    if (lane == 0) a.list[atomicAdd(a.counter, 1ull)] = i;
    return;
  }
  const Tin* own = in_graph ? row(t) : nullptr;
  Tout* o = out + i * a.out_stride;
  for (int64_t c = (int64_t)lane * P::kWidth; c < a.F; c += (int64_t)lpr * P::kWidth)
    finish<Tin, Tout, VEC4>(a, sum_entries<Rows, VEC4>(row, a.col, b, e, c), e - b, own, o, c);
}

template <typename Rows, typename Tout, bool VEC4>
__global__ __launch_bounds__(kNT) void k_graph_agg_long(typename Rows::Src src, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
  using piece = typename P::type;
  using Tin = typename Rows::elem;
  __shared__ piece part[2][kNT];
  const int lpr = 1 << a.lpr_log2, groups = kNT >> a.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1), grp = threadIdx.x >> a.lpr_log2;
  const Rows row(src, a);
  const int64_t n = (int64_t)*a.counter;
  unsigned round = 0;  // (workgroup-uniform, as every loop bound below: all 256 threads reach every barrier)
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = a.list[r];
    const int64_t t = a.ids ? a.ids[i] : a.row0 + i;  // (inside the graph: the row was found long)
    const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
    const int64_t chunks = (e - b + kGraphChunk - 1) / kGraphChunk;
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
          p = sum_entries<Rows, VEC4>(row, a.col, cb, std::min<int64_t>(e, cb + kGraphChunk), c);
        }
        part[round & 1][threadIdx.x] = p;
        __syncthreads();
        if (grp == 0) {
          const int m = (int)std::min<int64_t>(groups, chunks - j0);
          for (int g = 0; g < m; ++g) P::add(total, part[round & 1][(g << a.lpr_log2) + lane]);
        }
      }
      if (grp == 0 && active) finish<Tin, Tout, VEC4>(a, total, e - b, row(t), o, c);
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

}  // namespace graph_agg
}  // namespace spp

using namespace spp;
using namespace spp::graph_agg;

extern "C" int64_t spp_graph_agg_chunk(void) { return kGraphChunk; }

extern "C" int64_t spp_graph_agg_workspace_bytes(int64_t num_targets) {
  return kWorkspaceHeader + 8 * std::max<int64_t>(num_targets, 0);
}

namespace {

// what both entries share: spp_graph_agg_desc without its source
struct Call {
  int32_t epilogue, x_elem, out_elem;
  const int64_t* rowptr;
  const int64_t* col;
  int64_t x_stride, x_rows, F, row0;
  const int64_t* ids;
  int64_t T;
  void* out;
  int64_t out_stride;
  float self_scale;
};

// the source of spp_graph_agg_parts_forward: the non-empty parts in order
struct Parts {
  int n;
  int64_t first[kMaxParts];
  const void* base[kMaxParts];
};

// exactly one of x / parts is given
spp_status forward(const char* who, const Call& d, const void* x_dev, const Parts* parts, void* workspace_dev,
                   int64_t workspace_bytes, void* stream) {
  SPP_REQUIRE(d.epilogue == SPP_AGG_MEAN || d.epilogue == SPP_AGG_OPERAND || d.epilogue == SPP_AGG_SUM,
              "%s: epilogue %d (the mean, the operand and the sum; no activation on load)", who, (int)d.epilogue);
  SPP_REQUIRE(d.x_elem != SPP_ELEM_FP8_E4M3, "%s: fp8 rows are not read here (dequantise the table first)", who);
  SPP_REQUIRE((d.x_elem == SPP_ELEM_F32 || d.x_elem == SPP_ELEM_F16 || d.x_elem == SPP_ELEM_BF16) &&
                  (d.out_elem == SPP_ELEM_F32 || d.out_elem == SPP_ELEM_BF16),
              "%s: unknown or unsupported element code (x %d, out %d)", who, (int)d.x_elem, (int)d.out_elem);
  const bool by_ids = d.ids != nullptr, by_slab = d.row0 >= 0;
  SPP_REQUIRE(by_ids != by_slab, "%s: give the targets as a slab (target_row0 >= 0) or as a list (target_ids_dev), %s", who,
              by_ids ? "not both" : "one of them");
  const int64_t T = d.T, F = d.F;
  SPP_REQUIRE(T >= 0 && F >= 0 && d.x_rows >= 0, "%s: negative size", who);
  SPP_REQUIRE(by_ids || (d.row0 <= d.x_rows && T <= d.x_rows - d.row0),
              "%s: the slab [%lld, %lld) leaves the graph's %lld rows", who, (long long)d.row0, (long long)(d.row0 + T),
              (long long)d.x_rows);
  const int64_t width = d.epilogue == SPP_AGG_OPERAND ? 2 * F : F;
  const int64_t out_stride = d.out_stride > 0 ? d.out_stride : width;
  SPP_REQUIRE(out_stride >= width, "%s: output stride smaller than the output row", who);
  SPP_REQUIRE(workspace_dev && aligned_to(workspace_dev, 16) && workspace_bytes >= spp_graph_agg_workspace_bytes(T),
              "%s: needs a 16-byte aligned workspace of spp_graph_agg_workspace_bytes(num_targets) = %lld bytes", who,
              (long long)spp_graph_agg_workspace_bytes(T));
  if (T == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr && d.col && (parts || x_dev) && d.out && d.x_rows > 0, "%s: NULL buffer or empty graph", who);
  SPP_REQUIRE(d.x_stride >= F, "%s: row stride smaller than the row", who);
  // the vector form: four columns per lane.  Rows of x that do not allow it (with parts: the rows of any of them) are
  // read one column per lane instead; an output that does not is refused (the caller allocates it)
  bool vec = F % 4 == 0 && d.x_stride % 4 == 0;
  if (parts)
    for (int p = 0; p < parts->n; ++p) vec = vec && aligned_to(parts->base[p], 4 * elem_bytes(d.x_elem));
  else
    vec = vec && aligned_to(x_dev, 4 * elem_bytes(d.x_elem));
  SPP_REQUIRE(!vec || (out_stride % 4 == 0 && aligned_to(d.out, 4 * elem_bytes(d.out_elem))),
              "%s: F %% 4 == 0 needs the output aligned to 4 elements (base and stride)", who);
  const int lpr_log2 = lanes_log2(vec ? F / 4 : F);
  const int64_t grid = ceil_div(T << lpr_log2, kNT);
  SPP_REQUIRE(grid < (1ll << 31), "%s: too many targets for one launch (%lld)", who, (long long)T);
  hipStream_t st = as_stream(stream);
  Args a{};
  a.rowptr = d.rowptr, a.col = d.col, a.ids = d.ids, a.row0 = by_ids ? 0 : d.row0, a.T = T;
  a.x_stride = d.x_stride, a.x_rows = d.x_rows, a.F = F, a.out_stride = out_stride;
  a.epilogue = d.epilogue, a.self_scale = d.self_scale, a.lpr_log2 = lpr_log2;
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
      for (int p = 0; p < kMaxParts; ++p) t.first[p] = INT64_MAX;  // (behind the last part: never the owner)
      for (int p = 0; p < parts->n; ++p) {
        t.first[p] = parts->first[p];
        t.base[p] = reinterpret_cast<const Tin*>(reinterpret_cast<uintptr_t>(parts->base[p]) -
                                                 (uintptr_t)parts->first[p] * (uintptr_t)d.x_stride * sizeof(Tin));
      }
      hipLaunchKernelGGL((k_graph_agg_rows<PartRows<Tin>, Tout, V>), dim3((unsigned)grid), dim3(kNT), 0, st, t, out, a);
      hipLaunchKernelGGL((k_graph_agg_long<PartRows<Tin>, Tout, V>), dim3(long_grid), dim3(kNT), 0, st, t, out, a);
    } else {
      const Tin* x = static_cast<const Tin*>(x_dev);
      hipLaunchKernelGGL((k_graph_agg_rows<NodeRows<Tin>, Tout, V>), dim3((unsigned)grid), dim3(kNT), 0, st, x, out, a);
      hipLaunchKernelGGL((k_graph_agg_long<NodeRows<Tin>, Tout, V>), dim3(long_grid), dim3(kNT), 0, st, x, out, a);
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

extern "C" spp_status spp_graph_agg_forward(const spp_graph_agg_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                            void* stream) {
  const char* who = "spp_graph_agg_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_agg_desc& d = *desc;
  const Call c{d.epilogue,    d.x_elem,         d.out_elem,    d.rowptr_dev, d.col_dev,          d.x_stride_elems, d.x_rows, d.F,
               d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,    d.out_stride_elems, d.self_scale};
  return forward(who, c, d.x_dev, nullptr, workspace_dev, workspace_bytes, stream);
}

extern "C" spp_status spp_graph_agg_parts_forward(const spp_graph_agg_parts_desc* desc, void* workspace_dev,
                                                  int64_t workspace_bytes, void* stream) {
  const char* who = "spp_graph_agg_parts_forward";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_agg_parts_desc& d = *desc;
  SPP_REQUIRE(d.num_parts >= 1 && d.num_parts <= SPP_GRAPH_AGG_MAX_PARTS, "%s: num_parts %d outside 1..%d", who,
              (int)d.num_parts, (int)SPP_GRAPH_AGG_MAX_PARTS);
  SPP_REQUIRE(d.part_offsets[0] == 0, "%s: part_offsets[0] must be 0, got %lld", who, (long long)d.part_offsets[0]);
  Parts parts{};
  for (int p = 0; p < d.num_parts; ++p) {
    SPP_REQUIRE(d.part_offsets[p + 1] >= d.part_offsets[p], "%s: part_offsets decrease at part %d (%lld after %lld)", who, p,
                (long long)d.part_offsets[p + 1], (long long)d.part_offsets[p]);
    if (d.part_offsets[p + 1] == d.part_offsets[p]) continue;  // an empty part owns no row: its base may be NULL
    SPP_REQUIRE(d.x_parts_dev[p], "%s: part %d holds the rows [%lld, %lld) and its base is NULL", who, p,
                (long long)d.part_offsets[p], (long long)d.part_offsets[p + 1]);
    parts.first[parts.n] = d.part_offsets[p], parts.base[parts.n] = d.x_parts_dev[p], ++parts.n;
  }
  const Call c{d.epilogue,    d.x_elem,         d.out_elem,    d.rowptr_dev, d.col_dev,          d.x_stride_elems,
               d.part_offsets[d.num_parts],     d.F,
               d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,    d.out_stride_elems, d.self_scale};
  return forward(who, c, nullptr, &parts, workspace_dev, workspace_bytes, stream);
}
