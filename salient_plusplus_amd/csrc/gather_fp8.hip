// f3c: dequantising row gather of an fp8 (OCP e4m3) feature table with per-column power-of-two scales
//     dst[j, c] = fp16( float32(q[idx[j], c]) * 2^scale_log2[c] )        (include/spp.h, spp_gather_rows_fp8)
// The loop, the scale loading and the conversion live in fp8_body.hip.h (shared with the fp8 assembly of the fused
// delivery, sampler.hip); this file adds the caller-supplied (untrusted) indices and the entry point.
#include "spp_internal.h"

#include "fp8_body.hip.h"

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

}  // namespace spp

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
