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
//
// f3o: the same two kernels over an fp8 TABLE read in place (spp_graph_agg_forward_fp8, spp_graph_agg_parts_forward_fp8):
// rows of e4m3 bytes with one power-of-two exponent per column (include/spp.h, f3c).  A load returns
// v = float32(code) * 2^e -- both steps exact -- so everything behind the load is the fp32 rows' arithmetic on v: same
// order, same bits as over the table dequantised to fp32.  The exponents ride with the row source (Fp8NodeRows /
// Fp8PartRows: new instantiations, no existing kernel's arguments change).
//
// f3q: the MAXIMUM over the row instead of its sum (SPP_AGG_MAX / SPP_AGG_MAX_OPERAND; one matrix only, not the parts):
// kMax instantiations of the same two kernels.  The best starts as the first entry and a later one replaces it by the
// rule of spp_agg_max_forward; a long row's chunk maxima are combined by that rule in chunk order.  Nothing is rounded, so
// the result is the bits of spp_agg_max_forward on the same row for EVERY row length.
#include "graph_rows.hip.h"

namespace spp {
namespace graph_agg {

using namespace graph_rows;

struct Args : Targets {
  int32_t epilogue;     // SPP_AGG_MEAN / _OPERAND / _SUM; kMax kernels: SPP_AGG_MAX / _MAX_OPERAND
  float self_scale;
  int lpr_log2;
  LongRows long_rows;
};

// The row source of the kernels: Rows::Src is what the launch passes by value, Rows(src, a) what a lane asks for the
// address of global row g, and cols(c) what a load of the columns c.. needs besides the address: nothing (NoScale) for
// fp32 / fp16 / bf16 rows, the columns' factors for fp8 rows (f3o, below).
struct NoScale {};
// row g of the full matrix; an id outside [0, x_rows) reads row 0 (the rule of the Table source: no fault)
template <typename Tin>
struct NodeRows {
  using elem = Tin;
  using Src = const Tin* __restrict__;
  const Tin* x;
  int64_t stride, rows;
  __device__ __forceinline__ NodeRows(const Tin* src, const Args& a) : x(src), stride(a.x_stride), rows(a.x_rows) {}
  __device__ __forceinline__ const Tin* operator()(int64_t g) const {
    return x + ((uint64_t)g < (uint64_t)rows ? g : 0) * stride;
  }
  __device__ __forceinline__ NoScale cols(int64_t) const { return {}; }
};

// row g of the part that owns it (graph_rows.hip.h: the tables and the owner search), NodeRows' rule for an id outside
template <typename Tin>
struct PartRows {
  using elem = Tin;
  using Src = PartTable<1>;
  const int64_t* first;     // LDS
  const Tin* const* base;   // LDS
  int64_t stride, rows;
  // every thread of the workgroup constructs it, before any of them leaves the kernel (a barrier inside)
  __device__ __forceinline__ PartRows(const Src& src, const Args& a) : stride(a.x_stride), rows(a.x_rows) {
    __shared__ int64_t lds_first[kMaxParts];
    __shared__ const Tin* lds_base[kMaxParts];
    if (threadIdx.x == 0) {
#pragma unroll
      for (int p = 0; p < kMaxParts; ++p) lds_first[p] = src.first[p], lds_base[p] = static_cast<const Tin*>(src.base[0][p]);
    }
    __syncthreads();
    first = lds_first, base = lds_base;
  }
  __device__ __forceinline__ const Tin* operator()(int64_t g) const {
    g = (uint64_t)g < (uint64_t)rows ? g : 0;
    return base[part_owner(first, g)] + g * stride;
  }
  __device__ __forceinline__ NoScale cols(int64_t) const { return {}; }
};

// fp8 rows (f3o): OCP e4m3 bytes, one power-of-two exponent per COLUMN (the load of aggregate.hip's fp8 kernels,
// repeated here so that those come out unchanged).  A lane's piece is one dword: four columns, always the vector form
// (F % 16 == 0, rows F bytes apart).
struct e4m3 {
  uint8_t bits;
};
typedef float f32x2_fp8 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float exp2_i8(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }  // e in [-64, 63]

// cols(c) of an e4m3 source: the factors 2^e of the columns c .. c+3 -- built once per column piece, outside the loop
// over the row's entries, and again for every piece of a lane that takes several
struct Fp8Scale4 {
  f4 s;
  __device__ __forceinline__ Fp8Scale4(const int8_t* __restrict__ scale_log2, int64_t c) {
    const uint32_t raw = *reinterpret_cast<const uint32_t*>(scale_log2 + c);
    s = {exp2_i8((int8_t)raw), exp2_i8((int8_t)(raw >> 8)), exp2_i8((int8_t)(raw >> 16)), exp2_i8((int8_t)(raw >> 24))};
  }
};
template <class P, typename Tin>
__device__ __forceinline__ typename P::type load_piece(const Tin* p, NoScale) { return P::load(p); }
template <class P>
__device__ __forceinline__ f4 load_piece(const e4m3* p, const Fp8Scale4& sc) {
  const uint32_t raw = *reinterpret_cast<const uint32_t*>(p);
  const f32x2_fp8 a = __builtin_amdgcn_cvt_pk_f32_fp8(raw, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(raw, true);
  return {a.x * sc.s.x, a.y * sc.s.y, b.x * sc.s.z, b.y * sc.s.w};
}

// the two row sources over an e4m3 table: Src adds the exponents to what the launch passes by value
template <class Base>
struct Fp8Rows : Base {
  struct Src {
    typename Base::Src rows;
    const int8_t* scale_log2;
  };
  const int8_t* scale_log2;
  __device__ __forceinline__ Fp8Rows(const Src& src, const Args& a) : Base(src.rows, a), scale_log2(src.scale_log2) {}
  __device__ __forceinline__ Fp8Scale4 cols(int64_t c) const { return Fp8Scale4(scale_log2, c); }
};
using Fp8NodeRows = Fp8Rows<NodeRows<e4m3>>;
using Fp8PartRows = Fp8Rows<PartRows<e4m3>>;

// columns c.. of the entries [b, e), added in CSR order one at a time from zero; four rows are in flight
template <typename Rows, bool VEC4, class Scale>
__device__ __forceinline__ typename Piece<VEC4>::type sum_entries(const Rows& row, const int64_t* __restrict__ col,
                                                                  int64_t b, int64_t e, int64_t c, const Scale& sc) {
  using P = Piece<VEC4>;
  typename P::type acc = P::zero();
  int64_t k = b;
  for (; k + 3 < e; k += 4) {
    const int64_t j0 = col[k], j1 = col[k + 1], j2 = col[k + 2], j3 = col[k + 3];
    const auto v0 = load_piece<P>(row(j0) + c, sc), v1 = load_piece<P>(row(j1) + c, sc), v2 = load_piece<P>(row(j2) + c, sc),
               v3 = load_piece<P>(row(j3) + c, sc);
    P::add(acc, v0);
    P::add(acc, v1);
    P::add(acc, v2);
    P::add(acc, v3);
  }
  for (; k < e; ++k) P::add(acc, load_piece<P>(row(col[k]) + c, sc));
  return acc;
}

// the comparison rule of the maximum (include/spp.h f3q): v, a LATER value, replaces the best only if !(v <= best) and
// the best is not a NaN
__device__ __forceinline__ void take_max(float& best, float v) { best = (!(v <= best) && best == best) ? v : best; }
__device__ __forceinline__ void take_max(f4& best, f4 v) {
  take_max(best.x, v.x);
  take_max(best.y, v.y);
  take_max(best.z, v.z);
  take_max(best.w, v.w);
}

// columns c.. of the entries [b, e): their maximum, from the first entry on in CSR order (an empty range gives zero);
// two rows are in flight, as in k_agg_max_fwd
template <typename Rows, bool VEC4, class Scale>
__device__ __forceinline__ typename Piece<VEC4>::type max_entries(const Rows& row, const int64_t* __restrict__ col,
                                                                  int64_t b, int64_t e, int64_t c, const Scale& sc) {
  using P = Piece<VEC4>;
  if (b >= e) return P::zero();
  typename P::type best = load_piece<P>(row(col[b]) + c, sc);
  int64_t k = b + 1;
  for (; k + 1 < e; k += 2) {
    const int64_t j0 = col[k], j1 = col[k + 1];
    const auto v0 = load_piece<P>(row(j0) + c, sc), v1 = load_piece<P>(row(j1) + c, sc);
    take_max(best, v0);
    take_max(best, v1);
  }
  if (k < e) take_max(best, load_piece<P>(row(col[k]) + c, sc));
  return best;
}

template <typename Rows, bool VEC4, bool kMax, class Scale>
__device__ __forceinline__ typename Piece<VEC4>::type reduce_entries(const Rows& row, const int64_t* __restrict__ col,
                                                                     int64_t b, int64_t e, int64_t c, const Scale& sc) {
  if constexpr (kMax) return max_entries<Rows, VEC4>(row, col, b, e, c, sc);
  else return sum_entries<Rows, VEC4>(row, col, b, e, c, sc);
}

// what the sum of node t's row becomes, columns c.. of output row o (own: node t's row of x, NULL for a target id
// outside the graph, whose output row is all zeros)
template <typename Tin, typename Tout, bool VEC4, bool kMax, class Scale>
__device__ __forceinline__ void finish(const Args& a, typename Piece<VEC4>::type acc, int64_t deg, const Tin* own,
                                       Tout* o, int64_t c, const Scale& sc) {
  using P = Piece<VEC4>;
  if constexpr (kMax) {  // the maximum as it is; [max | x[target]] for the operand
    if (a.epilogue == SPP_AGG_MAX_OPERAND) P::store(o + a.F + c, own ? load_piece<P>(own + c, sc) : P::zero());
  } else if (a.epilogue == SPP_AGG_SUM) {
    if (a.self_scale != 0.f && own) acc = P::fma(a.self_scale, load_piece<P>(own + c, sc), acc);
  } else {
    acc = P::scaled(acc, 1.0f / (float)(deg > 0 ? deg : 1));
    if (a.epilogue == SPP_AGG_OPERAND) P::store(o + a.F + c, own ? load_piece<P>(own + c, sc) : P::zero());
  }
  P::store(o + c, acc);
}

template <typename Rows, typename Tout, bool VEC4, bool kMax>
__global__ __launch_bounds__(kNT) void k_graph_agg_rows(typename Rows::Src src, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
  using Tin = typename Rows::elem;
  const Rows row(src, a);  // (PartRows: the whole workgroup, before anyone returns)
  const int lpr = 1 << a.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t i = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> a.lpr_log2;
  if (i >= a.T) return;
  const int64_t t = a.target(i);
  const bool in_graph = (uint64_t)t < (uint64_t)a.x_rows;
  const int64_t b = in_graph ? a.rowptr[t] : 0, e = in_graph ? a.rowptr[t + 1] : 0;
  if (e - b > kGraphChunk) {  // a long row: k_graph_agg_long's
    if (lane == 0) a.long_rows.append(i);
    return;
  }
  const Tin* own = in_graph ? row(t) : nullptr;
  Tout* o = out + i * a.out_stride;
  for (int64_t c = (int64_t)lane * P::kWidth; c < a.F; c += (int64_t)lpr * P::kWidth) {
    const auto sc = row.cols(c);
    finish<Tin, Tout, VEC4, kMax>(a, reduce_entries<Rows, VEC4, kMax>(row, a.col, b, e, c, sc), e - b, own, o, c, sc);
  }
}

template <typename Rows, typename Tout, bool VEC4, bool kMax>
__global__ __launch_bounds__(kNT) void k_graph_agg_long(typename Rows::Src src, Tout* __restrict__ out, Args a) {
  using P = Piece<VEC4>;
  using piece = typename P::type;
  using Tin = typename Rows::elem;
  __shared__ piece part[2][kNT];
  const int lpr = 1 << a.lpr_log2, groups = kNT >> a.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1), grp = threadIdx.x >> a.lpr_log2;
  const Rows row(src, a);
  const int64_t n = a.long_rows.count();
  unsigned round = 0;  // (workgroup-uniform, as every loop bound below: all 256 threads reach every barrier)
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = a.long_rows.list[r];
    const int64_t t = a.target(i);  // (inside the graph: the row was found long)
    const int64_t b = a.rowptr[t], e = a.rowptr[t + 1];
    const int64_t chunks = (e - b + kGraphChunk - 1) / kGraphChunk;
    Tout* o = out + i * a.out_stride;
    for (int64_t c0 = 0; c0 < a.F; c0 += (int64_t)lpr * P::kWidth) {
      const int64_t c = c0 + (int64_t)lane * P::kWidth;
      const bool active = c < a.F;
      const auto sc = row.cols(active ? c : 0);  // (a lane behind the row's last piece loads nothing past the scales)
      piece total = P::zero();
      for (int64_t j0 = 0; j0 < chunks; j0 += groups, ++round) {
        // group g sums chunk j0 + g; round k parks its sums in part[k & 1], which is written again in round k + 2,
        // behind the barrier of round k + 1 that group 0 reaches after it has read them
        const int64_t j = j0 + grp;
        piece p = P::zero();
        if (active && j < chunks) {
          const int64_t cb = b + j * kGraphChunk;
          p = reduce_entries<Rows, VEC4, kMax>(row, a.col, cb, std::min<int64_t>(e, cb + kGraphChunk), c, sc);
        }
        part[round & 1][threadIdx.x] = p;
        __syncthreads();
        if (grp == 0) {
          const int m = (int)std::min<int64_t>(groups, chunks - j0);
          for (int g = 0; g < m; ++g) {
            const piece q = part[round & 1][(g << a.lpr_log2) + lane];
            if constexpr (!kMax) P::add(total, q);
            else if (j0 == 0 && g == 0) total = q;  // (the maximum starts from the first chunk's, not from zero)
            else take_max(total, q);
          }
        }
      }
      if (grp == 0 && active) finish<Tin, Tout, VEC4, kMax>(a, total, e - b, row(t), o, c, sc);
    }
  }
}

}  // namespace graph_agg
}  // namespace spp

using namespace spp;
using namespace spp::graph_agg;

extern "C" int64_t spp_graph_agg_chunk(void) { return kGraphChunk; }

extern "C" int64_t spp_graph_agg_workspace_bytes(int64_t num_targets) { return workspace_bytes(num_targets); }

namespace {

template <typename Rows, typename Tout, bool V, bool kMax = false>
void launch(const Launch& l, const typename Rows::Src& src, void* out, const Args& a, hipStream_t st) {
  hipLaunchKernelGGL((k_graph_agg_rows<Rows, Tout, V, kMax>), dim3(l.grid), dim3(kNT), 0, st, src, static_cast<Tout*>(out), a);
  hipLaunchKernelGGL((k_graph_agg_long<Rows, Tout, V, kMax>), dim3(l.long_grid), dim3(kNT), 0, st, src, static_cast<Tout*>(out), a);
}

// what the four entries share; exactly one of x / parts is given.  scale_log2 (the _fp8 entries; NULL elsewhere): the
// rows are e4m3 bytes read in place with these per-column exponents.
spp_status forward(const char* who, const Common& d, int32_t epilogue, float self_scale, const void* x_dev,
                   const Parts* parts, const int8_t* scale_log2, bool fp8, void* workspace_dev, int64_t workspace_bytes,
                   void* stream) {
  const bool max = epilogue == SPP_AGG_MAX || epilogue == SPP_AGG_MAX_OPERAND;
  SPP_REQUIRE(epilogue == SPP_AGG_MEAN || epilogue == SPP_AGG_OPERAND || epilogue == SPP_AGG_SUM || (max && !parts),
              "%s: epilogue %d (the mean, the operand and the sum; no activation on load%s)", who, (int)epilogue,
              parts ? "; the maximum is not built over parts" : "; the maximum and its operand");
  if (fp8) {
    SPP_REQUIRE(d.x_elem == SPP_ELEM_FP8_E4M3,
                "%s: x_elem %d: this entry reads an fp8 table in place (SPP_ELEM_FP8_E4M3); other rows go to the entry without _fp8",
                who, (int)d.x_elem);
    SPP_REQUIRE(d.F % 16 == 0, "%s: F (%lld) must be a multiple of 16 (fp8 rows, include/spp.h f3c)", who, (long long)d.F);
  }
  Launch l;
  SPP_TRY(check_common(who, d, epilogue == SPP_AGG_OPERAND || epilogue == SPP_AGG_MAX_OPERAND ? 2 * d.F : d.F, d.F, parts ? parts->base[0] : &x_dev,
                       parts ? parts->n : 1, true, workspace_dev, workspace_bytes, &l, fp8));
  if (l.empty) return SPP_OK;
  if (fp8) {
    SPP_REQUIRE(scale_log2 && aligned_to(scale_log2, 4), "%s: scale_log2_dev must be there and 4-byte aligned (int8 [F])", who);
    SPP_REQUIRE(l.vec, "%s: fp8 rows are read a dword at a time: every base and x_stride_elems (bytes) must be a multiple of 4",
                who);
  }
  hipStream_t st = as_stream(stream);
  const Args a{l.targets, epilogue, self_scale, l.lpr_log2, l.long_rows};
  SPP_HIP_TRY(hipMemsetAsync(workspace_dev, 0, kWorkspaceHeader, st));
  if (fp8) {
    with_f32_bf16(d.out_elem, [&](auto tout) {
      using Tout = typename decltype(tout)::type;
      if (parts)
        launch<Fp8PartRows, Tout, true>(l, {part_table<1>(*parts, {d.x_stride}), scale_log2}, d.out, a, st);
      else if (max)
        launch<Fp8NodeRows, Tout, true, true>(l, {static_cast<const e4m3*>(x_dev), scale_log2}, d.out, a, st);
      else
        launch<Fp8NodeRows, Tout, true>(l, {static_cast<const e4m3*>(x_dev), scale_log2}, d.out, a, st);
    });
  } else {
    with_in_out_vec(d.x_elem, d.out_elem, l.vec, [&](auto tin, auto tout, auto v) {
      using Tin = typename decltype(tin)::type;
      using Tout = typename decltype(tout)::type;
      constexpr bool V = decltype(v)::value;
      if (parts)
        launch<PartRows<Tin>, Tout, V>(l, part_table<1>(*parts, {d.x_stride * (int64_t)sizeof(Tin)}), d.out, a, st);
      else if (max)
        launch<NodeRows<Tin>, Tout, V, true>(l, static_cast<const Tin*>(x_dev), d.out, a, st);
      else
        launch<NodeRows<Tin>, Tout, V>(l, static_cast<const Tin*>(x_dev), d.out, a, st);
    });
  }
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

spp_status whole(const char* who, const spp_graph_agg_desc* desc, const int8_t* scale_log2, bool fp8, void* workspace_dev,
                 int64_t workspace_bytes, void* stream) {
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_agg_desc& d = *desc;
  const Common c{d.x_elem, d.out_elem,    d.rowptr_dev,     d.col_dev,     d.x_stride_elems, d.x_rows,
                 d.F,      d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,        d.out_stride_elems};
  return forward(who, c, d.epilogue, d.self_scale, d.x_dev, nullptr, scale_log2, fp8, workspace_dev, workspace_bytes, stream);
}

spp_status over_parts(const char* who, const spp_graph_agg_parts_desc* desc, const int8_t* scale_log2, bool fp8,
                      void* workspace_dev, int64_t workspace_bytes, void* stream) {
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_graph_agg_parts_desc& d = *desc;
  Parts parts;
  SPP_TRY(check_parts(who, d.num_parts, d.part_offsets, d.x_parts_dev, "base (x_parts_dev)", nullptr, nullptr, &parts));
  const Common c{d.x_elem, d.out_elem,    d.rowptr_dev,     d.col_dev,     d.x_stride_elems, d.part_offsets[d.num_parts],
                 d.F,      d.target_row0, d.target_ids_dev, d.num_targets, d.out_dev,        d.out_stride_elems};
  return forward(who, c, d.epilogue, d.self_scale, nullptr, &parts, scale_log2, fp8, workspace_dev, workspace_bytes, stream);
}

}  // namespace

extern "C" spp_status spp_graph_agg_forward(const spp_graph_agg_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                            void* stream) {
  return whole("spp_graph_agg_forward", desc, nullptr, false, workspace_dev, workspace_bytes, stream);
}

extern "C" spp_status spp_graph_agg_parts_forward(const spp_graph_agg_parts_desc* desc, void* workspace_dev,
                                                  int64_t workspace_bytes, void* stream) {
  return over_parts("spp_graph_agg_parts_forward", desc, nullptr, false, workspace_dev, workspace_bytes, stream);
}

// f3o: the same entries over an fp8 table read in place; one exponent vector for the whole table (all parts)
extern "C" spp_status spp_graph_agg_forward_fp8(const spp_graph_agg_desc* desc, const int8_t* scale_log2_dev,
                                                void* workspace_dev, int64_t workspace_bytes, void* stream) {
  return whole("spp_graph_agg_forward_fp8", desc, scale_log2_dev, true, workspace_dev, workspace_bytes, stream);
}

extern "C" spp_status spp_graph_agg_parts_forward_fp8(const spp_graph_agg_parts_desc* desc, const int8_t* scale_log2_dev,
                                                      void* workspace_dev, int64_t workspace_bytes, void* stream) {
  return over_parts("spp_graph_agg_parts_forward_fp8", desc, scale_log2_dev, true, workspace_dev, workspace_bytes, stream);
}
