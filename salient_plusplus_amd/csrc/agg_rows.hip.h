// What the hop kernels (aggregate.hip: mean / operand / sum; aggregate_max.hip: max) share on the load side: where batch
// row j comes from (Rows<Tin, Src>) and the fp8 rows' load with its per-column factors (ColScale4 / ColScale1).
#pragma once

#include "elem_io.hip.h"

#include <type_traits>

namespace spp {

// fp8 rows (f3c, include/spp.h): OCP e4m3 bytes with one power-of-two exponent per COLUMN.  A load returns
// v = float32(code) * 2^e -- both steps exact (v_cvt_pk_f32_fp8; e in [-64, 63]) -- so everything behind the load is the
// fp32 kernel's arithmetic on v.  The exponents ride in the epilogue record (Fp8<Epi>: a new instantiation of the same
// kernel, no existing kernel's arguments change); the factors of a lane's columns are built once per column step,
// outside the loop over the row's entries.
struct fp8e4m3 {
  uint8_t bits;
};
template <class Epi>
struct Fp8 : Epi {
  const int8_t* scale_log2;
};
typedef float f32x2_fp8 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float exp2_i8(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }
// the factors of columns c .. c+3 (ColScale4) / of column c (ColScale1); empty for every other element type
template <bool kFp8>
struct ColScale4 {
  template <class Epi>
  __device__ __forceinline__ ColScale4(const Epi&, int64_t) {}
};
template <>
struct ColScale4<true> {
  f4 s;
  template <class Epi>
  __device__ __forceinline__ ColScale4(const Epi& epi, int64_t c) {
    const uint32_t raw = *reinterpret_cast<const uint32_t*>(epi.scale_log2 + c);
    s = {exp2_i8((int8_t)raw), exp2_i8((int8_t)(raw >> 8)), exp2_i8((int8_t)(raw >> 16)), exp2_i8((int8_t)(raw >> 24))};
  }
};
template <bool kFp8>
struct ColScale1 {
  template <class Epi>
  __device__ __forceinline__ ColScale1(const Epi&, int64_t) {}
};
template <>
struct ColScale1<true> {
  float s;
  template <class Epi>
  __device__ __forceinline__ ColScale1(const Epi& epi, int64_t c) : s(exp2_i8(epi.scale_log2[c])) {}
};
template <typename T>
__device__ __forceinline__ f4 load4(const T* p, const ColScale4<false>&) { return load4(p); }
template <typename T>
__device__ __forceinline__ float load1(const T* p, const ColScale1<false>&) { return load1(p); }
__device__ __forceinline__ f4 load4(const fp8e4m3* p, const ColScale4<true>& sc) {
  const uint32_t raw = *reinterpret_cast<const uint32_t*>(p);
  const f32x2_fp8 a = __builtin_amdgcn_cvt_pk_f32_fp8(raw, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(raw, true);
  return {a.x * sc.s.x, a.y * sc.s.y, b.x * sc.s.z, b.y * sc.s.w};
}
__device__ __forceinline__ float load1(const fp8e4m3* p, const ColScale1<true>& sc) {
  return __builtin_amdgcn_cvt_f32_fp8((uint32_t)p->bits, 0) * sc.s;
}

// ---- neighbour reduction over a hop: where row j comes from (Rows<Tin, Src>(j)) ----
//   Dense: x + j * x_stride, the batch's matrix (targets are its first rows).
//   Table (first layer, opt-in): x is the RESIDENT feature table and row j of the batch is x[nid[j]] (nid = the batch's
//     n_id, int64) -- the batch's feature matrix is never written and re-read (242 MB each way at papers scale); the
//     sum runs over the same rows in the same order as over a materialised x[n_id]: bit-identical.  An id outside
//     [0, x_rows) reads row 0 (no fault).
//   Refs (first layer, opt-in, partitioned path): the F elements at ADDRESS nid[j] (row references, spp_mfg_out.row_addr:
//     local partition / VIP cache / received rows / a peer's partition); x and x_stride are unused.
struct Dense {};
struct Table {};
struct Refs {};
template <typename Tin, class Src>
struct Rows {
  const Tin* x;
  int64_t x_stride;
  const int64_t* nid;
  int64_t x_rows;
  __device__ __forceinline__ const Tin* operator()(int64_t j) const {
    if constexpr (std::is_same<Src, Refs>::value) return reinterpret_cast<const Tin*>((uintptr_t)nid[j]);
    if constexpr (std::is_same<Src, Table>::value) {
      const int64_t g = nid[j];
      j = (uint64_t)g < (uint64_t)x_rows ? g : 0;
    }
    return x + j * x_stride;
  }
};

}  // namespace spp
