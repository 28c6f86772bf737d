// Element I/O of the aggregation and inference kernels (aggregate.hip, gat.hip, graph_aggregate.hip, graph_gat.hip,
// resinc_epilogue.hip, classify.hip): fp32 / fp16 / bf16 rows as fp32 pieces on the device, and on the host the
// element-code helpers and the dispatch from element codes to kernel template arguments.
#pragma once

#include "spp_internal.h"

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <type_traits>

namespace spp {

struct f4 {
  float x, y, z, w;
};

// bf16 rows (torch.autocast(dtype=torch.bfloat16)): bf16 -> fp32 is exact (the 16 bits become the high half); fp32 ->
// bf16 is rounded once per stored element, to nearest even, by the packed hardware convert (v_cvt_pk_bf16_f32)
using bf16 = __hip_bfloat16;
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));
}

// loads convert to fp32 exactly; a bf16 store rounds once (the rule of spp_agg_forward)
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
  return {bf16_lo(raw.x), bf16_hi(raw.x), bf16_lo(raw.y), bf16_hi(raw.y)};
}
__device__ __forceinline__ float load1(const float* p) { return *p; }
__device__ __forceinline__ float load1(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float load1(const bf16* p) { return bf16_lo(*reinterpret_cast<const uint16_t*>(p)); }
__device__ __forceinline__ void store4(float* p, f4 v) { *reinterpret_cast<float4*>(p) = make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void store4(bf16* p, f4 v) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
}
__device__ __forceinline__ void store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void store1(bf16* p, float v) { *p = __float2bfloat16(v); }

// the piece of a row one lane of a graph kernel holds: four columns (vector form) or one
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
  static __device__ __forceinline__ void add(float& a, float v) { a += v; }
  static __device__ __forceinline__ float scaled(float a, float s) { return a * s; }
  static __device__ __forceinline__ float fma(float s, float o, float a) { return fmaf(s, o, a); }
  static __device__ __forceinline__ float over(float a, float s) { return a / s; }
  static __device__ __forceinline__ float relu(float a) { return fmaxf(a, 0.f); }
};

// W columns of a row as an array (the row-tile kernels: resinc_epilogue.hip, classify.hip)
template <int W>
struct PieceN {
  float v[W];
};

// ---- host: element codes (spp.h: SPP_ELEM_*) ----
static inline bool elem_ok(int32_t elem) { return elem == SPP_ELEM_F32 || elem == SPP_ELEM_F16 || elem == SPP_ELEM_BF16; }
static inline bool f32_bf16_ok(int32_t elem) { return elem == SPP_ELEM_F32 || elem == SPP_ELEM_BF16; }
static inline int64_t elem_bytes(int32_t elem) { return elem == SPP_ELEM_F32 ? 4 : elem == SPP_ELEM_FP8_E4M3 ? 1 : 2; }
static inline bool aligned_to(const void* p, int64_t bytes) { return reinterpret_cast<uintptr_t>(p) % (uintptr_t)bytes == 0; }

// the lanes that share a row of `pieces` pieces: the first power of two that covers them, at most a wavefront
static int lanes_log2(int64_t pieces) {
  int l = 0;
  while ((1 << l) < pieces && l < 6) ++l;
  return l;
}

// fn(Type<T>{}) for the element code `elem` (the caller has checked it); with_elem_vec adds
// std::integral_constant<bool, VEC4>{}.  with_f32_bf16: the codes without fp16 (outputs, gradients).
// with_in_out_vec: fn(Type<Tin>{}, Type<Tout>{}, vec) for a kernel over <Tin, Tout, VEC4>.
template <typename T> struct Type { using type = T; };
template <class Fn>
static void with_elem(int32_t elem, Fn&& fn) {
  elem == SPP_ELEM_BF16 ? fn(Type<bf16>{}) : elem ? fn(Type<__half>{}) : fn(Type<float>{});
}
template <class Fn>
static void with_elem_vec(int32_t elem, bool vec, Fn&& fn) {
  with_elem(elem, [&](auto tin) { vec ? fn(tin, std::true_type{}) : fn(tin, std::false_type{}); });
}
template <class Fn>
static void with_f32_bf16(int32_t elem, Fn&& fn) {
  elem == SPP_ELEM_BF16 ? fn(Type<bf16>{}) : fn(Type<float>{});
}
template <class Fn>
static void with_in_out_vec(int32_t x_elem, int32_t out_elem, bool vec, Fn&& fn) {
  auto by_in = [&](auto v) {
    with_elem(x_elem, [&](auto tin) { with_f32_bf16(out_elem, [&](auto tout) { fn(tin, tout, v); }); });
  };
  vec ? by_in(std::true_type{}) : by_in(std::false_type{});
}

}  // namespace spp
