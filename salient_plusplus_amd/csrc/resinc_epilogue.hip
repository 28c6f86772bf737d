// f3i: the layer tail of SAGEResInception in eval mode, leaky_relu(BatchNorm(z)) + residual, as ONE pass over the
// GEMM tile that holds z (reference: driver/models.py:127-192, `x = F.leaky_relu(self.bns[i](h)); x += res`):
//     y        = fma(a[c], z[i,c], b[c])           a, b: BatchNorm's running statistics folded by the caller
//     y        = y >= 0 ? y : negative_slope * y
//     out[i,c] = round_once(y + r[row(i), c])      row(i) = r_row0 + i  or  r_ids[i];  no r: round_once(y)
// (include/spp.h, spp_resinc_epilogue, states the contract.)  As torch ops the tail is about five element-wise passes
// over an fp32 tile; here z and the residual row are read once and the slab of the next activation matrix is written
// once, in place.
//
// Shape (gather_body.hip.h's): lpr lanes (a power of two, at most 64) own one row, a workgroup's 256 / lpr lane groups
// take kUnroll rows each, and the loads of those rows -- the ids of a list first, then z and the residual rows -- are
// issued back to back before the first use.  Two bodies, chosen by a WORKGROUP-UNIFORM condition: the full one (every
// row of the tile exists, every lane owns a piece in every sweep) stores without a predicate; the other clamps its
// loads to row n - 1 / piece 0 and predicates the stores alone.  A residual row outside [0, r_rows) is loaded from row 0
// and the OUTPUT row is zeros (the target rule of the graph kernels): a select, not a branch.  The vector form moves
// W = 4 columns per lane when any of z, r, out is fp32 and W = 8 when all are 16-bit, so the widest operand moves in
// 16-byte pieces; the scalar form is the same code with W = 1.  No atomics, no LDS, every offset 64-bit.
#include "elem_io.hip.h"

namespace spp {
namespace resinc {

constexpr int kNT = 256;
constexpr int kUnroll = 4;  // rows in flight per lane group

struct NoRes {};  // the residual's element type when there is none

__device__ __forceinline__ float2 half2_of(uint32_t w) { return __half22float2(*reinterpret_cast<const __half2*>(&w)); }

// loads convert to fp32 exactly (elem_io.hip.h: PieceN, the bf16 halves and the packed store convert)
template <int W>
__device__ __forceinline__ PieceN<W> load(const float* p) {
  PieceN<W> o;
  if constexpr (W == 1) {
    o.v[0] = *p;
  } else {
#pragma unroll
    for (int k = 0; k < W; k += 4) {
      const float4 q = *reinterpret_cast<const float4*>(p + k);
      o.v[k] = q.x, o.v[k + 1] = q.y, o.v[k + 2] = q.z, o.v[k + 3] = q.w;
    }
  }
  return o;
}
template <int W>
__device__ __forceinline__ PieceN<W> load(const bf16* p) {
  PieceN<W> o;
  if constexpr (W == 1) {
    o.v[0] = __uint_as_float((uint32_t)*reinterpret_cast<const uint16_t*>(p) << 16);
  } else if constexpr (W == 4) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    o.v[0] = bf16_lo(q.x), o.v[1] = bf16_hi(q.x), o.v[2] = bf16_lo(q.y), o.v[3] = bf16_hi(q.y);
  } else {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    o.v[0] = bf16_lo(q.x), o.v[1] = bf16_hi(q.x), o.v[2] = bf16_lo(q.y), o.v[3] = bf16_hi(q.y);
    o.v[4] = bf16_lo(q.z), o.v[5] = bf16_hi(q.z), o.v[6] = bf16_lo(q.w), o.v[7] = bf16_hi(q.w);
  }
  return o;
}
template <int W>
__device__ __forceinline__ PieceN<W> load(const __half* p) {
  PieceN<W> o;
  if constexpr (W == 1) {
    o.v[0] = __half2float(*p);
  } else if constexpr (W == 4) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    const float2 x = half2_of(q.x), y = half2_of(q.y);
    o.v[0] = x.x, o.v[1] = x.y, o.v[2] = y.x, o.v[3] = y.y;
  } else {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const float2 x = half2_of(q.x), y = half2_of(q.y), z = half2_of(q.z), w = half2_of(q.w);
    o.v[0] = x.x, o.v[1] = x.y, o.v[2] = y.x, o.v[3] = y.y, o.v[4] = z.x, o.v[5] = z.y, o.v[6] = w.x, o.v[7] = w.y;
  }
  return o;
}
template <int W>
__device__ __forceinline__ PieceN<W> load(const NoRes*) {
  return PieceN<W>{};
}

// a bf16 store rounds once, to nearest even
template <int W>
__device__ __forceinline__ void store(float* p, const PieceN<W>& o) {
  if constexpr (W == 1) {
    *p = o.v[0];
  } else {
#pragma unroll
    for (int k = 0; k < W; k += 4) *reinterpret_cast<float4*>(p + k) = make_float4(o.v[k], o.v[k + 1], o.v[k + 2], o.v[k + 3]);
  }
}
template <int W>
__device__ __forceinline__ void store(bf16* p, const PieceN<W>& o) {
  if constexpr (W == 1) {
    *p = __float2bfloat16(o.v[0]);
  } else if constexpr (W == 4) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(o.v[0], o.v[1]), pack_bf16x2(o.v[2], o.v[3]));
  } else {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(o.v[0], o.v[1]), pack_bf16x2(o.v[2], o.v[3]),
                                              pack_bf16x2(o.v[4], o.v[5]), pack_bf16x2(o.v[6], o.v[7]));
  }
}

struct Args {
  const float* a;      // [C]
  const float* b;      // [C]
  const int64_t* ids;  // NULL: the slab r_row0 .. r_row0 + n
  int64_t row0, r_rows;
  int64_t n, C;
  int64_t z_stride, r_stride, out_stride;
  float slope;
  int lpr_log2;
};

// the contract's arithmetic for one element; the intrinsics keep the compiler from contracting slope * y + r into an fma
template <bool kRes>
__device__ __forceinline__ float tail(float a, float z, float b, float slope, float r) {
  float y = fmaf(a, z, b);
  y = y >= 0.f ? y : __fmul_rn(slope, y);
  return kRes ? __fadd_rn(y, r) : y;
}

template <typename Tz, typename Tr, typename Tout, int W, bool kFull>
__device__ __forceinline__ void tile_body(const Tz* __restrict__ z, const Tr* __restrict__ r, Tout* __restrict__ out,
                                          const Args& a, int64_t base) {
  constexpr bool kRes = !std::is_same<Tr, NoRes>::value;
  const int lpr = 1 << a.lpr_log2, gpb = kNT >> a.lpr_log2;
  const int g = threadIdx.x >> a.lpr_log2, l = threadIdx.x & (lpr - 1);
  const int64_t pieces = a.C / W;
  int64_t i[kUnroll], row[kUnroll];
  bool ok[kUnroll], inside[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int64_t iu = base + (int64_t)u * gpb + g;
    ok[u] = kFull || iu < a.n;
    i[u] = ok[u] ? iu : a.n - 1;  // (clamped: loaded, never stored)
  }
  if constexpr (kRes) {
    if (a.ids) {  // (a kernel argument: one scalar branch around the four id loads)
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) row[u] = a.ids[i[u]];
    } else {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) row[u] = a.row0 + i[u];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      inside[u] = (uint64_t)row[u] < (uint64_t)a.r_rows;
      row[u] = inside[u] ? row[u] : 0;  // (r_rows >= 1: the entry checked)
    }
  }
  for (int64_t p0 = 0; p0 < pieces; p0 += lpr) {  // (workgroup-uniform bounds)
    const int64_t p = p0 + l;
    const bool on = kFull || p < pieces;
    const int64_t c = (on ? p : 0) * W;
    const PieceN<W> av = load<W>(a.a + c), bv = load<W>(a.b + c);
    PieceN<W> zv[kUnroll], rv[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) zv[u] = load<W>(z + i[u] * a.z_stride + c);
    if constexpr (kRes) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) rv[u] = load<W>(r + row[u] * a.r_stride + c);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      PieceN<W> o;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const float y = tail<kRes>(av.v[k], zv[u].v[k], bv.v[k], a.slope, kRes ? rv[u].v[k] : 0.f);
        o.v[k] = !kRes || inside[u] ? y : 0.f;
      }
      Tout* dst = out + i[u] * a.out_stride + c;
      if constexpr (kFull) {
        store<W>(dst, o);
      } else {
        if (ok[u] && on) store<W>(dst, o);
      }
    }
  }
}

template <typename Tz, typename Tr, typename Tout, int W>
__global__ __launch_bounds__(kNT) void k_resinc_epilogue(const Tz* __restrict__ z, const Tr* __restrict__ r,
                                                         Tout* __restrict__ out, Args a) {
  const int lpr = 1 << a.lpr_log2;
  const int64_t rows_per_tile = (int64_t)(kNT >> a.lpr_log2) * kUnroll;
  const int64_t base = (int64_t)blockIdx.x * rows_per_tile;
  if (base + rows_per_tile <= a.n && (a.C / W) % lpr == 0)
    tile_body<Tz, Tr, Tout, W, true>(z, r, out, a, base);
  else
    tile_body<Tz, Tr, Tout, W, false>(z, r, out, a, base);
}

}  // namespace resinc
}  // namespace spp

using namespace spp;
using namespace spp::resinc;

extern "C" spp_status spp_resinc_epilogue(const spp_resinc_epilogue_desc* desc, void* stream) {
  const char* who = "spp_resinc_epilogue";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_resinc_epilogue_desc& d = *desc;
  SPP_REQUIRE(d.z_dev && d.out_dev && d.a_dev && d.b_dev, "%s: NULL buffer (z_dev, out_dev, a_dev or b_dev)", who);
  const bool res = d.r_dev != nullptr;
  SPP_REQUIRE((d.z_elem == SPP_ELEM_F32 || d.z_elem == SPP_ELEM_BF16) &&
                  (d.out_elem == SPP_ELEM_F32 || d.out_elem == SPP_ELEM_BF16) &&
                  (!res || d.r_elem == SPP_ELEM_F32 || d.r_elem == SPP_ELEM_F16 || d.r_elem == SPP_ELEM_BF16),
              "%s: unknown or unsupported element code (z_elem %d, r_elem %d, out_elem %d)", who, (int)d.z_elem,
              (int)d.r_elem, (int)d.out_elem);
  const int64_t n = d.n, C = d.C;
  SPP_REQUIRE(C >= 1 && C < (1ll << 31), "%s: C = %lld must be in [1, 2^31)", who, (long long)C);
  SPP_REQUIRE(n >= 0, "%s: negative n (%lld)", who, (long long)n);
  SPP_REQUIRE(d.z_stride_elems >= 0 && d.out_stride_elems >= 0 && d.r_stride_elems >= 0,
              "%s: negative row stride (z %lld, r %lld, out %lld)", who, (long long)d.z_stride_elems,
              (long long)d.r_stride_elems, (long long)d.out_stride_elems);
  const int64_t z_stride = d.z_stride_elems ? d.z_stride_elems : C, out_stride = d.out_stride_elems ? d.out_stride_elems : C,
                r_stride = d.r_stride_elems ? d.r_stride_elems : C;
  SPP_REQUIRE(z_stride >= C && out_stride >= C && (!res || r_stride >= C), "%s: a row stride smaller than the row (C = %lld)",
              who, (long long)C);
  const bool by_ids = d.r_ids_dev != nullptr, by_slab = d.r_row0 >= 0;
  SPP_REQUIRE(!(by_ids && by_slab), "%s: address the residual as a slab (r_row0 >= 0) or as a list (r_ids_dev), not both", who);
  SPP_REQUIRE(!res || by_ids || by_slab, "%s: a residual needs its rows: a slab (r_row0 >= 0) or a list (r_ids_dev)", who);
  SPP_REQUIRE(!res || d.r_rows >= 0, "%s: negative r_rows (%lld)", who, (long long)d.r_rows);
  if (n == 0) return SPP_OK;
  SPP_REQUIRE(!res || d.r_rows >= 1, "%s: a residual matrix without rows (r_rows = 0) for n = %lld output rows", who,
              (long long)n);
  // the vector form: the widest of z, r, out moves 16-byte pieces
  const bool any32 = d.z_elem == SPP_ELEM_F32 || d.out_elem == SPP_ELEM_F32 || (res && d.r_elem == SPP_ELEM_F32);
  const int64_t W = any32 ? 4 : 8;
  const bool vec = C % W == 0 && z_stride % W == 0 && out_stride % W == 0 && (!res || r_stride % W == 0) &&
                   aligned_to(d.z_dev, W * elem_bytes(d.z_elem)) && aligned_to(d.out_dev, W * elem_bytes(d.out_elem)) &&
                   (!res || aligned_to(d.r_dev, W * elem_bytes(d.r_elem))) && aligned_to(d.a_dev, 16) && aligned_to(d.b_dev, 16);
  const int lpr_log2 = lanes_log2(vec ? C / W : C);
  const int64_t grid = ceil_div(n, (int64_t)(kNT >> lpr_log2) * kUnroll);
  SPP_REQUIRE(grid < (1ll << 31), "%s: too many rows for one launch (n %lld)", who, (long long)n);
  Args a{};
  a.a = d.a_dev, a.b = d.b_dev, a.ids = d.r_ids_dev, a.row0 = by_slab ? d.r_row0 : 0, a.r_rows = res ? d.r_rows : 0;
  a.n = n, a.C = C, a.z_stride = z_stride, a.r_stride = r_stride, a.out_stride = out_stride;
  a.slope = d.negative_slope, a.lpr_log2 = lpr_log2;
  hipStream_t st = as_stream(stream);
  auto launch = [&](auto tz, auto tr, auto tout, auto w) {
    using Tz = typename decltype(tz)::type;
    using Tr = typename decltype(tr)::type;
    using Tout = typename decltype(tout)::type;
    constexpr int Wc = decltype(w)::value;
    hipLaunchKernelGGL((k_resinc_epilogue<Tz, Tr, Tout, Wc>), dim3((unsigned)grid), dim3(kNT), 0, st,
                       static_cast<const Tz*>(d.z_dev), static_cast<const Tr*>(d.r_dev), static_cast<Tout*>(d.out_dev), a);
  };
  // W follows from the types: 8 where all are 16-bit, else 4; 1 in the scalar form
  auto by_w = [&](auto tz, auto tr, auto tout) {
    using Tz = typename decltype(tz)::type;
    using Tr = typename decltype(tr)::type;
    using Tout = typename decltype(tout)::type;
    constexpr bool k32 = sizeof(Tz) == 4 || sizeof(Tout) == 4 || (!std::is_same<Tr, NoRes>::value && sizeof(Tr) == 4);
    vec ? launch(tz, tr, tout, std::integral_constant<int, k32 ? 4 : 8>{})
        : launch(tz, tr, tout, std::integral_constant<int, 1>{});
  };
  auto by_out = [&](auto tz, auto tr) {
    d.out_elem == SPP_ELEM_BF16 ? by_w(tz, tr, Type<bf16>{}) : by_w(tz, tr, Type<float>{});
  };
  auto by_r = [&](auto tz) {
    if (!res) by_out(tz, Type<NoRes>{});
    else if (d.r_elem == SPP_ELEM_BF16) by_out(tz, Type<bf16>{});
    else if (d.r_elem == SPP_ELEM_F16) by_out(tz, Type<__half>{});
    else by_out(tz, Type<float>{});
  };
  d.z_elem == SPP_ELEM_BF16 ? by_r(Type<bf16>{}) : by_r(Type<float>{});
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
