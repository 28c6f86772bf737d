// f3c: dequantising row gather of an fp8 (OCP e4m3) feature table with per-column power-of-two scales
//     dst[j, c] = fp16( float32(q[idx[j], c]) * 2^scale_log2[c] )        (include/spp.h, spp_gather_rows_fp8)
// The loop, the scale loading and the conversion live in fp8_body.hip.h (shared with the fp8 assembly of the fused
// delivery, sampler.hip); this file adds the caller-supplied (untrusted) indices and the entry point.
#include "spp_internal.h"

#include "fp8_body.hip.h"

#include <algorithm>

namespace spp {

// chunks = F / 16 sixteen-byte pieces per source row; lpr = the power of two >= chunks (<= 64)
template <typename IdxT>
__global__ __launch_bounds__(kGatherThreads) void k_gather_rows_fp8(const char* __restrict__ src, int64_t src_rows,
                                                                     const int8_t* __restrict__ scale_log2,
                                                                     const IdxT* __restrict__ idx, int64_t n,
                                                                     int64_t row_bytes, int chunks, int lpr_log2,
                                                                     char* __restrict__ dst, int32_t* err) {
  dequant_rows_body([=](int64_t r) { return idx[r]; },
                    [=](IdxT k) {
                      int64_t i = (int64_t)k;
                      if ((uint64_t)i >= (uint64_t)src_rows) {
                        raise_async_error(err, SPP_AERR_GATHER_INDEX);
                        i = 0;
                      }
                      return src + i * row_bytes;
                    },
                    scale_log2, n, row_bytes, chunks, lpr_log2, dst, blockIdx.x, gridDim.x);
}

// f3o: rows of the table as dense fp32, dst[j, c] = float32(q[row(j), c]) * 2^scale_log2[c] -- the exact value, nothing
// rounded -- for the GEMM tiles of exact inference over an fp8 table (include/spp.h, spp_fp8_rows_f32).  One lane per
// piece of four columns: a dword of the source row in, 16 bytes of fp32 out, consecutive lanes on consecutive pieces of
// a row and then of the next row (the output is one dense array of n * F / 4 pieces); a grid-stride loop.  row(j) is
// row0 + j (ids == NULL) or ids[j], with the gather's rule for an id outside the table.
__global__ __launch_bounds__(kGatherThreads) void k_fp8_rows_f32(const char* __restrict__ src, int64_t src_rows,
                                                                  const int8_t* __restrict__ scale_log2, int64_t row0,
                                                                  const int64_t* __restrict__ ids, int64_t n,
                                                                  int64_t pieces, float* __restrict__ dst, int32_t* err) {
  const int64_t total = n * pieces, step = (int64_t)gridDim.x * kGatherThreads;
  for (int64_t k = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x; k < total; k += step) {
    const int64_t j = k / pieces, c = 4 * (k - j * pieces);
    int64_t i = ids ? ids[j] : row0 + j;
    if ((uint64_t)i >= (uint64_t)src_rows) {
      raise_async_error(err, SPP_AERR_GATHER_INDEX);
      i = 0;
    }
    const uint32_t raw = *reinterpret_cast<const uint32_t*>(src + i * (4 * pieces) + c);
    const uint32_t e = *reinterpret_cast<const uint32_t*>(scale_log2 + c);
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(raw, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(raw, true);
    const auto f = [e](int s) { return __uint_as_float((uint32_t)((int)(int8_t)(e >> s) + 127) << 23); };  // 2^e
    *reinterpret_cast<float4*>(dst + 4 * k) = make_float4(a.x * f(0), a.y * f(8), b.x * f(16), b.y * f(24));
  }
}

}  // namespace spp

extern "C" spp_status spp_fp8_rows_f32(const void* q_dev, int64_t src_rows, int64_t F, const int8_t* scale_log2_dev,
                                       int64_t row0, const int64_t* ids_dev, int64_t n, void* dst_dev, void* stream) {
  using namespace spp;
  const char* who = "spp_fp8_rows_f32";
  SPP_REQUIRE(F >= 0 && n >= 0 && src_rows >= 0, "%s: negative size", who);
  SPP_REQUIRE(F % 16 == 0, "%s: F (%lld) must be a multiple of 16", who, (long long)F);
  const bool by_ids = ids_dev != nullptr, by_slab = row0 >= 0;
  SPP_REQUIRE(by_ids != by_slab, "%s: give the rows as a slab (row0 >= 0) or as a list (ids_dev), %s", who,
              by_ids ? "not both" : "one of them");
  SPP_REQUIRE(by_ids || (row0 <= src_rows && n <= src_rows - row0), "%s: the slab [%lld, %lld) (row0, n) leaves the table's %lld rows",
              who, (long long)row0, (long long)(row0 + n), (long long)src_rows);
  if (n == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(q_dev && scale_log2_dev && dst_dev, "%s: NULL buffer", who);
  SPP_REQUIRE(src_rows > 0, "%s: %lld rows requested from an empty table", who, (long long)n);
  SPP_REQUIRE(((reinterpret_cast<uintptr_t>(q_dev) | reinterpret_cast<uintptr_t>(dst_dev)) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(scale_log2_dev) & 3) == 0,
              "%s: the table and the destination must be 16-byte aligned, the scales 4-byte aligned", who);
  hipStream_t st = as_stream(stream);
  const int64_t pieces = F / 4;
  const int64_t grid = std::min<int64_t>(ceil_div(n * pieces, kGatherThreads), 1 << 16);
  hipLaunchKernelGGL(k_fp8_rows_f32, dim3((unsigned)grid), dim3(kGatherThreads), 0, st, static_cast<const char*>(q_dev),
                     src_rows, scale_log2_dev, by_ids ? 0 : row0, ids_dev, n, pieces, static_cast<float*>(dst_dev),
                     async_err_word_current());
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_gather_rows_fp8(const void* q_dev, int64_t src_rows, int64_t F, const int8_t* scale_log2_dev,
                                          const int64_t* idx_dev, int64_t n, void* dst_dev, void* stream) {
  using namespace spp;
  SPP_REQUIRE(F >= 0 && n >= 0, "spp_gather_rows_fp8: negative size");
  SPP_REQUIRE(F % 16 == 0, "spp_gather_rows_fp8: F (%lld) must be a multiple of 16", (long long)F);
  if (n == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(q_dev && scale_log2_dev && idx_dev && dst_dev, "spp_gather_rows_fp8: NULL buffer");
  SPP_REQUIRE(src_rows > 0, "spp_gather_rows_fp8: %lld rows requested from an empty table", (long long)n);
  SPP_REQUIRE(((reinterpret_cast<uintptr_t>(q_dev) | reinterpret_cast<uintptr_t>(scale_log2_dev) |
                reinterpret_cast<uintptr_t>(dst_dev)) & 15) == 0,
              "spp_gather_rows_fp8: the table, the scales and the destination must be 16-byte aligned");
  // geometry of a 16-byte gather over the SOURCE rows (F bytes each): F / 16 pieces per row
  const GatherGeom gg = gather_geometry(q_dev, dst_dev, F, n, F, /*allow_span=*/false);
  SPP_REQUIRE(gg.vec == 16, "spp_gather_rows_fp8: internal geometry error");
  hipStream_t st = as_stream(stream);
  const int prof = prof_begin(SPP_PROF_GATHER, st, n);
  hipLaunchKernelGGL(k_gather_rows_fp8<int64_t>, dim3((unsigned)gg.grid), dim3(kGatherThreads), 0, st,
                     static_cast<const char*>(q_dev), src_rows, scale_log2_dev, idx_dev, n, F, gg.chunks, gg.lpr_log2,
                     static_cast<char*>(dst_dev), async_err_word_current());
  prof_end(SPP_PROF_GATHER, prof, st);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
