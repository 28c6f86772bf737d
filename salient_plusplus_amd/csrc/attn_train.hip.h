// What the two attention training pairs share (gatv2.hip, transformer_conv.hip) beyond gatv2_core.hip.h's lane
// mapping, State and dispatch tables.  Device: the forward's dropout heads and epilogue (kEmptyRows: TransformerConv's
// target without entries stores out = 0, row_max = 0, row_sum = 0; GATv2's self loop makes row_sum >= 1, no compare
// there), the backward's draw and row write.  Host: the block size, the shape check, the backward's geometry, one
// (element, shape, drop) dispatch per direction, the order of an entry's checks and the entry pairs.  A training file
// keeps its hot loops, the backward's per-target prologue, its row checks and its launches.
#pragma once

#include "gatv2_core.hip.h"

namespace spp {
namespace gatv2 {

constexpr int kAttnNT = 256;  // threads of a workgroup, all four kernels

// Forward: the global head behind each of a lane's HL local ones, and the call's draw arguments
template <int CPH, int HL>
__device__ __forceinline__ void fwd_drop_heads(Drop<HL>& dr, const ActArgs& a, int H, int lpr, int lane, int g_log2) {
  dr.a = a, dr.H = H;
#pragma unroll
  for (int hl = 0; hl < HL; ++hl) dr.head[hl] = ((hl * CPH) * lpr + lane) >> g_log2;
}

// target t's out pieces (acc / s; kDrop: acc * (drop_scale / s)) and, from the lane that holds a head's first piece,
// row_max and row_sum.  kEmptyRows: a row without entries stores out = 0, row_max = 0, row_sum = 0, nothing is divided
template <bool kDrop, bool kEmptyRows, int NQ, int CPH>
__device__ __forceinline__ void fwd_store(const State<NQ, CPH>& st, int64_t t, int lpr, int lane, int g_log2, int H,
                                          float drop_scale, float* __restrict__ out, float* __restrict__ row_max,
                                          float* __restrict__ row_sum) {
  const int64_t D = (int64_t)NQ * lpr * 4;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int hl = q / CPH;
    const int p = q * lpr + lane;
    const bool empty = kEmptyRows && st.ss[hl] == 0.f;
    f4 r = {0.f, 0.f, 0.f, 0.f};
    if (!empty) r = st.template result<kDrop>(q, drop_scale);
    *reinterpret_cast<float4*>(out + t * D + (int64_t)p * 4) = make_float4(r.x, r.y, r.z, r.w);
    if ((p & ((1 << g_log2) - 1)) == 0) {  // the head's first piece
      row_max[t * H + (p >> g_log2)] = empty ? 0.f : st.mm[hl];
      row_sum[t * H + (p >> g_log2)] = st.ss[hl];
    }
  }
}

// the target's own row gradient (grad_x_r, grad_q), kept in registers across the row and written once
template <int NS>
__device__ __forceinline__ void bwd_store_row(float* __restrict__ grad, int64_t t, int lane, int lpt,
                                              const float (&acc)[NS]) {
  const int64_t D = (int64_t)NS * lpt;
#pragma unroll
  for (int i = 0; i < NS; ++i) grad[t * D + lane + lpt * i] = acc[i];
}

// The backward's draw of (entry, head): attn_keep_head(entry, H, head, a), for every argument.  kWaveHash (NS >= 4, so
// D >= 256: lpt = 64, a wavefront is ONE target, and C >= 32, so the two heads that share a hash sit in the same step of
// every lane): entry and head & ~1 are the same in all lanes, so the hash's argument is taken from the first lane and
// the 64-bit mix runs once per wavefront on the scalar unit; only the choice of the hash's half stays per lane.  Left
// on the vector unit, four hashes in flight cost <*, 4, 1> two waves per SIMD.
// What kWaveHash relies on, all of it given by NS >= 4 and the entries' shape checks (check_heads, check_channels):
//   lpt == 64, so the 64 lanes of a wavefront are ONE group, one target, one entry k at a time, and they leave the
//     kernel together (t >= T): the first active lane's entry is every lane's;
//   C >= 32 (H <= 8 and D >= 256), so head & ~1 = ((lane + 64 * hl * SPH) >> c_log2) & ~1 does not depend on the lane:
//     C = 32: head = 2 hl + (lane >> 5); C = 64: head = hl; C >= 128: SPH = C / 64 and head = hl;
//   H == 1 or H even (check_heads: 1, 2, 4, 8): the line that forms i2 says where.  An odd H > 1 would need
//     (entry * H + head) >> 1 with the lane's own head, which is not uniform.
template <bool kWaveHash>
__device__ __forceinline__ bool bwd_keep(uint64_t entry, int H, int head, const ActArgs& a) {
  if constexpr (!kWaveHash) {
    return attn_keep_head(entry, H, head, a);
  } else {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)entry);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(entry >> 32));
    const uint32_t he = __builtin_amdgcn_readfirstlane((uint32_t)head & ~1u);
    // i = entry * H + head.  H even: entry * H is even, so i >> 1 = (entry * H + (head & ~1)) >> 1; H = 1: head = 0 and
    // i >> 1 = entry >> 1.  Holds for H in {1, even} ONLY (check_heads admits 1, 2, 4, 8)
    const uint64_t i2 = ((((uint64_t)hi << 32) | lo) * (uint64_t)H + he) >> 1;
    const uint64_t r = mix64(a.seed + i2 * 0x9E3779B97F4A7C15ull);
    const bool odd = (((uint32_t)entry * (uint32_t)H + (uint32_t)head) & 1u) != 0;
    return (uint32_t)(odd ? r >> 32 : r) < a.keep_thr;
  }
}

// ---- host ----
// The fields both descriptors (spp_gatv2_desc, spp_transformer_desc) have under the same names, and their checks in the
// order include/spp.h documents (after the descriptor itself): head count, element code, C, power of two, D, sizes.
struct HopShape {
  int32_t heads, x_elem;
  int64_t C, num_targets, num_sources;
};
static inline spp_status check_shape(const HopShape& h, const char* who) {
  SPP_TRY(check_heads(who, h.heads));
  SPP_REQUIRE(elem_ok(h.x_elem), "%s: unknown element code %d", who, (int)h.x_elem);
  SPP_TRY(check_channels(who, h.heads, h.C));
  SPP_REQUIRE(h.num_targets >= 0 && h.num_sources >= h.num_targets, "%s: needs 0 <= T <= S", who);
  return SPP_OK;
}

// the backward's geometry of D = heads * C columns (the forward's is Shape, shape_of)
struct BwdShape {
  int lpt_log2, seg_log2, c_log2, ns, sph;
};
static inline BwdShape bwd_shape_of(int64_t heads, int64_t C) {
  const int64_t D = heads * C;
  BwdShape s;
  s.lpt_log2 = log2_of(std::min<int64_t>(D, kWave));
  const int64_t lpt = 1ll << s.lpt_log2;
  s.ns = (int)(D / lpt), s.sph = (int)std::max<int64_t>(1, C / kWave);
  s.seg_log2 = log2_of(std::min<int64_t>(C, lpt)), s.c_log2 = log2_of(C);
  return s;
}
// workgroups for T targets of 2^lanes_log2 lanes each, one target per lane group
static inline unsigned grid_of(int64_t T, int lanes_log2) { return (unsigned)ceil_div(T << lanes_log2, kAttnNT); }

// fn(Type<Tin>{}, IC<NQ>{}, IC<CPH>{}, bool_constant<kDrop>{}, shape) / fn(Type<Tin>{}, IC<NS>{}, IC<SPH>{}, ...)
template <class Fn>
static void dispatch_fwd(int32_t elem, int64_t heads, int64_t C, bool drop, Fn&& fn) {
  const Shape sh = shape_of(heads, C);
  with_elem(elem, [&](auto tin) {
    with_fwd_shape(sh.nq, sh.cph, [&](auto q, auto c) { with_drop(drop, [&](auto dr) { fn(tin, q, c, dr, sh); }); });
  });
}
template <class Fn>
static void dispatch_bwd(int32_t elem, int64_t heads, int64_t C, bool drop, Fn&& fn) {
  const BwdShape sh = bwd_shape_of(heads, C);
  with_elem(elem, [&](auto tin) {
    with_bwd_shape(sh.ns, sh.sph, [&](auto n, auto s) { with_drop(drop, [&](auto dr) { fn(tin, n, s, dr, sh); }); });
  });
}

// An entry: the shape; the dropout arguments (in eval mode too); first(), what the family checks whatever T is; rows()
// for T > 0; always(), what it writes whatever T is (GATv2's backward: grad_att); the T == 0 return; launch().
struct NoStep {
  spp_status operator()() const { return SPP_OK; }
};
template <class Desc, class Rows, class Launch, class First = NoStep, class Always = NoStep>
static spp_status attn_entry(const Desc* d, const char* who, const AttnDrop& dr, Rows&& rows, Launch&& launch,
                             First&& first = {}, Always&& always = {}) {
  SPP_REQUIRE(d != nullptr, "%s: NULL descriptor", who);
  SPP_TRY(check_shape(HopShape{d->heads, d->x_elem, d->C, d->num_targets, d->num_sources}, who));
  SPP_TRY(attn_drop_check(dr, who));
  SPP_TRY(first());
  if (d->num_targets > 0) SPP_TRY(rows());
  SPP_TRY(always());
  if (d->num_targets == 0) return SPP_OK;
  launch();
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// the two entries of one direction: `name` without dropout and `name_drop` with (p, training, seed) after `stream`
#define SPP_ATTN_ENTRIES(name, name_drop, Desc, impl)                                                      \
  extern "C" spp_status name(const Desc* d, void* stream) { return impl(d, stream, #name, AttnDrop{}); }   \
  extern "C" spp_status name_drop(const Desc* d, void* stream, float p, int32_t training, uint64_t seed) { \
    return impl(d, stream, #name_drop, AttnDrop{true, p, training, seed});                                 \
  }

}  // namespace gatv2
}  // namespace spp
