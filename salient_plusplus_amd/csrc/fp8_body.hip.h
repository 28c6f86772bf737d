// f3c: the dequantising row loop shared by k_gather_rows_fp8 (gather_fp8.hip) and the fp8 assembly of the fused
// delivery (sampler.hip, k_deliver<16, false, true>): e4m3 rows with per-column power-of-two scales in, fp16 rows out,
//     dst[r, c] = fp16( float32(q[src(r), c]) * 2^scale_log2[c] ).
// The loop is move_rows_vec_body<16> (gather_body.hip.h) with a conversion between the load and the store: a group of
// LPR lanes moves one row, each lane loads 16 bytes (16 elements) of the source row and stores 32 bytes of fp16;
// consecutive groups take consecutive output rows, every group keeps kGatherUnroll rows in flight, and the keys of
// the next grid-stride iteration are requested right behind the row loads of this one.  A lane keeps its column chunk
// across rows, so its 16 scales are loaded once and kept as fp32 factors 2^e (the product with an e4m3 value is exact
// for e in [-64, 63]); fp32 -> fp16 rounds once, to nearest even.  The properties the plain gather was tuned for hold:
// the unconditional body is chosen by a workgroup-uniform condition, the stores carry no per-lane predicate there, and
// the row loads of a round are issued together (no wait between them).
#pragma once

#include <hip/hip_fp16.h>

#include "gather_body.hip.h"

namespace spp {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

struct Fp8Scales {
  float s[16];
};

// the 16 factors 2^e of the columns [16 * chunk, 16 * chunk + 16)
__device__ __forceinline__ Fp8Scales load_fp8_scales(const int8_t* __restrict__ scale_log2, int chunk) {
  const u32x4 raw = *reinterpret_cast<const u32x4*>(scale_log2 + 16 * chunk);
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
  Fp8Scales o;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = (int)(int8_t)(w[i >> 2] >> (8 * (i & 3)));
    o.s[i] = __uint_as_float((uint32_t)(e + 127) << 23);  // 2^e, e in [-64, 63]: a normal fp32
  }
  return o;
}

// 16 e4m3 elements -> 16 fp16 (two 16-byte halves)
__device__ __forceinline__ void dequant16(u32x4 v, const Fp8Scales& sc, u32x4& lo, u32x4& hi) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);  // bytes 0, 1
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);   // bytes 2, 3
    const f32x2 pa = {a.x * sc.s[4 * i], a.y * sc.s[4 * i + 1]};
    const f32x2 pb = {b.x * sc.s[4 * i + 2], b.y * sc.s[4 * i + 3]};
    o[2 * i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(pa, f16x2));
    o[2 * i + 1] = __builtin_bit_cast(uint32_t, __builtin_convertvector(pb, f16x2));
  }
  lo = u32x4{o[0], o[1], o[2], o[3]};
  hi = u32x4{o[4], o[5], o[6], o[7]};
}

// dst[r, :] = dequantised *ptr_of(key_of(r)) for r < n.  key_of / ptr_of: as in move_rows_body (a pure load, then the
// address arithmetic).  row_bytes = F source bytes per row, output rows 2 * row_bytes apart; chunks = F / 16 sixteen-byte
// pieces per source row; lpr = the power of two >= chunks (<= 64).
template <typename KeyFn, typename PtrFn>
__device__ __forceinline__ void dequant_rows_body(KeyFn key_of, PtrFn ptr_of, const int8_t* __restrict__ scale_log2,
                                                  int64_t n, int64_t row_bytes, int chunks, int lpr_log2,
                                                  char* __restrict__ dst, int64_t vblock, int64_t nvblocks) {
  using K = decltype(key_of((int64_t)0));
  const int lpr = 1 << lpr_log2;
  const int g = threadIdx.x >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int gpb = kGatherThreads >> lpr_log2;
  const int64_t rows_per_iter = (int64_t)gpb * kGatherUnroll;
  const int64_t stride = nvblocks * rows_per_iter;
  const int64_t dst_row_bytes = 2 * row_bytes;
  int64_t base = vblock * rows_per_iter;
  if (base >= n) return;
  // lanes past the row's last piece load piece 0 (not predicated) and store nothing
  const bool lane_on = l < chunks;
  const int l0 = lane_on ? l : 0;
  const Fp8Scales sc = load_fp8_scales(scale_log2, l0);
  K key_next[kGatherUnroll];
#pragma unroll
  for (int u = 0; u < kGatherUnroll; ++u) {
    const int64_t r = base + (int64_t)u * gpb + g;
    key_next[u] = key_of(r < n ? r : n - 1);
  }
  const bool dense_lanes = chunks == lpr;
  for (; base < n; base += stride) {
    const u32x4* s[kGatherUnroll];
    u32x4* d[kGatherUnroll];
    u32x4 v[kGatherUnroll];
    const int64_t nbase = base + stride;
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) {
      const int64_t r = base + (int64_t)u * gpb + g;
      d[u] = reinterpret_cast<u32x4*>(dst + r * dst_row_bytes);
      s[u] = reinterpret_cast<const u32x4*>(ptr_of(key_next[u]));
    }
    if (dense_lanes && base + rows_per_iter <= n) {  // workgroup-uniform: every row exists, every lane has a piece
#pragma unroll
      for (int u = 0; u < kGatherUnroll; ++u) v[u] = s[u][l];
#pragma unroll
      for (int u = 0; u < kGatherUnroll; ++u) {  // next iteration's keys (clamped: past the end they are never used)
        const int64_t r = nbase + (int64_t)u * gpb + g;
        key_next[u] = key_of(r < n ? r : n - 1);
      }
#pragma unroll
      for (int u = 0; u < kGatherUnroll; ++u) {
        u32x4 lo, hi;
        dequant16(v[u], sc, lo, hi);
        row_store(lo, &d[u][2 * l]);
        row_store(hi, &d[u][2 * l + 1]);
      }
      continue;
    }
    bool ok[kGatherUnroll];
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) ok[u] = base + (int64_t)u * gpb + g < n;
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) v[u] = s[u][l0];
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) {
      const int64_t r = nbase + (int64_t)u * gpb + g;
      key_next[u] = key_of(r < n ? r : n - 1);
    }
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) {
      u32x4 lo, hi;
      dequant16(v[u], sc, lo, hi);
      if (ok[u] && lane_on) {
        row_store(lo, &d[u][2 * l]);
        row_store(hi, &d[u][2 * l + 1]);
      }
    }
    for (int c = l + lpr; c < chunks; c += lpr) {  // rows wider than 64 pieces (F > 1024): scales per piece
      const Fp8Scales sc2 = load_fp8_scales(scale_log2, c);
#pragma unroll
      for (int u = 0; u < kGatherUnroll; ++u) v[u] = s[u][c];
#pragma unroll
      for (int u = 0; u < kGatherUnroll; ++u) {
        u32x4 lo, hi;
        dequant16(v[u], sc2, lo, hi);
        if (ok[u]) {
          row_store(lo, &d[u][2 * c]);
          row_store(hi, &d[u][2 * c + 1]);
        }
      }
    }
  }
}

}  // namespace spp
