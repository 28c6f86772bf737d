// f3y: TransformerConv (Shi et al., "Masked Label Prediction"; PyG's TransformerConv) training over an MFG hop: the
// forward / backward pair behind spp_transformer_forward / spp_transformer_backward of include/spp.h.
//     q [T, H, C] = lin_query(x_target),   k [S, H, C] = lin_key(x),   v [S, H, C] = lin_value(x)   (projected by the caller)
//     e_ij^h     = scale * sum_c q[i,h,c] * k[j,h,c]
//     out[i,h,:] = sum_j softmax_j(e_ij^h) * v[j,h,:]
// over ALL CSR entries of row i in CSR order: no self loop, diagonal entries kept, a repeated entry counted as often as
// it appears.  A row without entries is a real case: out = 0, row_max = 0, row_sum = 0, grad_q = 0.
// What differs from gatv2.hip: the logit is a plain dot product, the message row (v) is not the key row (k), the
// backward has three row gradients, and there is no grad_att (so no LDS reduction and one group per target).  What is
// kept: gatv2_core.hip.h's lane mapping, per-head online softmax (State), butterfly and (NQ, CPH) dispatch, unchanged;
// several neighbours' loads in flight per round; one fp32 atomic per column per entry on contiguous wave-wide segments.
// Attention dropout (spp_transformer_forward_drop / spp_transformer_backward_drop, spp.h f4a) is the kDrop = true
// instantiation of the same two kernels: the keep rule of f3t without self-loop draws, the mask never in the softmax.
// Not here: edge features.  The kernels over the resident graph are graph_transformer.hip's; the forward's per-entry
// body is shared with them (transformer_core.hip.h).
#include "attn_train.hip.h"
#include "transformer_core.hip.h"

#include <cmath>

namespace spp {

using namespace gatv2;
using namespace transformer;

// THE LOGIT'S SUMMATION TREE (transformer_core.hip.h states it, with piece4 and the forward's walk) is walked bit for bit
// by both kernels: the backward recomputes alpha = expf(e - row_max) / row_sum from the forward's e.

// Forward.  lpr lanes per target, 4 columns per lane and chunk (gatv2_core.hip.h's mapping); the lane keeps its pieces of
// q[t] for the whole row; the row itself is transformer_core.hip.h's walk.  Per round: NB ids, then their k and v pieces, then the partial dots, then ONE butterfly that
// carries all NB * HL values (the logit's tree above); the logit is the butterfly's sum times scale (one product, the
// same bits in every lane of the head's segment); State::take does the online softmax on the v pieces.  The row starts from the empty state.
// No atomics: the same bits in every run.
// kDrop: out[i,h,:] = sum_j d_ij^h alpha_ij^h v[j,h,:], d = keep / (1 - p) per (entry, head) by the keep rule of f3t
// (entry k for CSR entry k, no self loop).  The softmax runs over ALL entries -- row_max and row_sum are the
// kDrop = false bits -- and only acc skips a dropped entry.  fwd_drop_heads finds the global head of the lane's head hl.
template <typename Tin, int NQ, int CPH, bool kDrop>
__global__ __launch_bounds__(kAttnNT) void k_transformer_fwd(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t T, const Tin* qm, int64_t q_stride,
    const Tin* km, int64_t k_stride, const Tin* vm, int64_t v_stride, float scale, int lpr_log2, int seg_log2,
    int g_log2, int H, float* __restrict__ out, float* __restrict__ row_max, float* __restrict__ row_sum,
    [[maybe_unused]] ActArgs drop) {
#pragma clang fp contract(off)
  constexpr int NB = tf_nb<NQ>();
  const int lpr = 1 << lpr_log2, lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kAttnNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;  // whole groups leave together (the shuffles below stay inside a group)
  int64_t c0[NQ];
  f4 qv[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    c0[q] = ((int64_t)q * lpr + lane) * 4;
    qv[q] = load4(qm + t * q_stride + c0[q]);
  }
  State<NQ, CPH> st;
  st.clear();
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  if constexpr (kDrop) {
    Drop<NQ / CPH> dr;
    fwd_drop_heads<CPH>(dr, drop, H, lpr, lane, g_log2);
    walk<NB, true>(st, qv, c0, km, k_stride, vm, v_stride, col, b, e, (int64_t)-1, scale, seg_log2, &dr);
  } else {
    walk<NB>(st, qv, c0, km, k_stride, vm, v_stride, col, b, e, (int64_t)-1, scale, seg_log2);  // (an MFG hop: ids as they are)
  }
  fwd_store<kDrop, true>(st, t, lpr, lane, g_log2, H, drop.scale, out, row_max, row_sum);
}

// Backward.  ONE column per lane and step, c = lane + lpt * i, i < NS, lpt = min(64, D) lanes per target, as k_gatv2_bwd:
// the fp32 atomics of an entry on grad_k and grad_v are contiguous 4 * lpt-byte segments, one atomic per column per
// entry and buffer.  A head is C consecutive columns: C <= lpt lanes of one step (SPH = 1) or SPH = C / 64 whole steps;
// a lane takes part in HL = NS / SPH heads.  Per entry the logit (recomputed; alpha = expf(e - row_max) / row_sum, no
// [E, H] array) and gv^h = g_i . v[j] are reduced by one butterfly; grad_q stays in registers across the row and is
// written once, zeros for a row without entries (whose row_sum = 0 is never divided by).  The logit is the forward's,
// bit for bit (the tree at the top of the file; contraction off, so that the product by scale is rounded before
// row_max is subtracted, as it is there).
// kDrop (the forward's (p, seed)): go is taken on the saved DROPPED out, so sum_j d alpha gh = go and
// ge = alpha (d gh - go) is the softmax gradient again -- a dropped entry (d = 0) still sends -alpha go to its logit --
// and grad_v[j] takes d alpha g_i.  d = keep ? 1 / (1 - p) : 0 per (entry, head), the forward's draws: the lane's head
// hl is global head (lane + lpt * hl * SPH) >> c_log2.  The draw is attn_train.hip.h's bwd_keep: for NS < 4 every lane
// hashes for the heads it holds (attn_keep_head); from NS = 4 on the hash runs once per wavefront on the first lane's
// argument and a lane only picks its half of it.
template <typename Tin, int NS, int SPH, bool kDrop>
__global__ __launch_bounds__(kAttnNT) void k_transformer_bwd(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t T, const Tin* qm, int64_t q_stride,
    const Tin* km, int64_t k_stride, const Tin* vm, int64_t v_stride, float scale, int lpt_log2, int seg_log2,
    int c_log2, int H, const float* __restrict__ out, const float* __restrict__ row_max,
    const float* __restrict__ row_sum, const float* __restrict__ g, float* __restrict__ grad_q, float* grad_k,
    float* grad_v, [[maybe_unused]] ActArgs drop) {
#pragma clang fp contract(off)
  constexpr int HL = NS / SPH;
  const int lpt = 1 << lpt_log2;
  const int lane = threadIdx.x & (lpt - 1);
  const int64_t D = (int64_t)NS * lpt;
  const int64_t t = ((int64_t)blockIdx.x * kAttnNT + threadIdx.x) >> lpt_log2;
  if (t >= T) return;  // whole groups leave together
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  float gv[NS], qv[NS], gq[NS], go[HL], m[HL], inv_s[HL];
  [[maybe_unused]] int heads[HL];
#pragma unroll
  for (int hl = 0; hl < HL; ++hl) {
    const int head = (lane + lpt * hl * SPH) >> c_log2;
    if constexpr (kDrop) heads[hl] = head;
    const float s = row_sum[t * H + head];
    m[hl] = row_max[t * H + head];
    inv_s[hl] = s > 0.f ? 1.f / s : 0.f;
    go[hl] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int64_t c = lane + lpt * i;
    gv[i] = g[t * D + c];
    qv[i] = load1(qm + t * q_stride + c);
    gq[i] = 0.f;
    go[i / SPH] += gv[i] * out[t * D + c];
  }
  for (int d = (1 << seg_log2) >> 1; d >= 1; d >>= 1)
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) go[hl] += __shfl_xor(go[hl], d, kWave);
  int64_t jn = b < e ? col[b] : 0;  // the next entry's id is read one entry ahead of its rows
  for (int64_t k = b; k < e; ++k) {
    const int64_t j = jn;
    jn = col[k + 1 < e ? k + 1 : k];
    float kx[NS], vx[NS], pp[NS], pe[HL], gh[HL];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      kx[i] = load1(km + j * k_stride + lane + lpt * i);
      vx[i] = load1(vm + j * v_stride + lane + lpt * i);
    }
    [[maybe_unused]] float dq[HL];  // kDrop: d = keep / (1 - p)
    if constexpr (kDrop) {
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) dq[hl] = bwd_keep<(NS >= 4)>((uint64_t)k, H, heads[hl], drop) ? drop.scale : 0.f;
    }
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) gh[hl] = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      pp[i] = qv[i] * kx[i];
      gh[i / SPH] += gv[i] * vx[i];
    }
    // the logit's tree (top of the file) with one column per lane and step: column distances 1 and 2 are lane
    // distances, every step's value on its own; then the head's steps (column distance 64 * step distance), widest
    // first; then the lane distances from the segment's half down to 4
#pragma unroll
    for (int d = 1; d <= 2; d <<= 1)
#pragma unroll
      for (int i = 0; i < NS; ++i) pp[i] += __shfl_xor(pp[i], d, kWave);
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) {
#pragma unroll
      for (int d = SPH / 2; d >= 1; d >>= 1)
#pragma unroll
        for (int i = 0; i < d; ++i) pp[hl * SPH + i] += pp[hl * SPH + i + d];
      pe[hl] = pp[hl * SPH];
    }
    for (int d = (1 << seg_log2) >> 1; d >= 4; d >>= 1)
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) pe[hl] += __shfl_xor(pe[hl], d, kWave);
    for (int d = (1 << seg_log2) >> 1; d >= 1; d >>= 1)
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) gh[hl] += __shfl_xor(gh[hl], d, kWave);
    float a[HL], ges[HL];
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) {
      a[hl] = expf(pe[hl] * scale - m[hl]) * inv_s[hl];
      if constexpr (kDrop) {
        ges[hl] = a[hl] * (dq[hl] * gh[hl] - go[hl]) * scale;  // ge * scale
        a[hl] *= dq[hl];  // from here on a is the message's weight d alpha
      } else {
        ges[hl] = a[hl] * (gh[hl] - go[hl]) * scale;  // ge * scale
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      gq[i] += ges[i / SPH] * kx[i];
      if (grad_k) unsafeAtomicAdd(grad_k + j * D + lane + lpt * i, ges[i / SPH] * qv[i]);
      if (grad_v) unsafeAtomicAdd(grad_v + j * D + lane + lpt * i, a[i / SPH] * gv[i]);
    }
  }
  bwd_store_row(grad_q, t, lane, lpt, gq);
}

}  // namespace spp

using namespace spp;
using namespace spp::gatv2;

// The row checks of both entries, after attn_train.hip.h's shape check and the T == 0 decision, in the order include/spp.h
// documents: strides, NULL buffers, alignment, scale.  Nothing here touches the device.
static spp_status tf_check_rows(const spp_transformer_desc* d, const char* who, bool backward) {
  const int64_t D = d->heads * d->C, esz = elem_bytes(d->x_elem);
  SPP_REQUIRE(d->q_stride_elems >= D && d->k_stride_elems >= D && d->v_stride_elems >= D &&
                  d->q_stride_elems % 4 == 0 && d->k_stride_elems % 4 == 0 && d->v_stride_elems % 4 == 0,
              "%s: a row stride is smaller than D or not a multiple of 4 elements", who);
  SPP_REQUIRE(d->rowptr_dev && d->q_dev && d->k_dev && d->v_dev && d->out_dev && d->row_max_dev && d->row_sum_dev &&
                  (!backward || (d->grad_out_dev && d->grad_q_dev)),
              "%s: NULL buffer", who);
  SPP_REQUIRE(aligned_to(d->q_dev, 4 * esz) && aligned_to(d->k_dev, 4 * esz) && aligned_to(d->v_dev, 4 * esz) &&
                  aligned_to(d->out_dev, 16) && aligned_to(d->row_max_dev, 4) && aligned_to(d->row_sum_dev, 4) &&
                  aligned_to(d->rowptr_dev, 8) && aligned_to(d->col_dev, 8),
              "%s: misaligned buffer (rows: 4 elements; out: 16 bytes)", who);
  SPP_REQUIRE(!backward || (aligned_to(d->grad_out_dev, 16) && aligned_to(d->grad_q_dev, 16) &&
                            aligned_to(d->grad_k_dev, 16) && aligned_to(d->grad_v_dev, 16)),
              "%s: misaligned buffer (grad_out, grad_q, grad_k, grad_v: 16 bytes)", who);
  SPP_REQUIRE(std::isfinite(d->scale) && d->scale > 0.f, "%s: scale must be finite and positive", who);
  return SPP_OK;
}

// attn_entry checks the _drop entries' AttnDrop (spp.h f4a) right after the shape, before T == 0, in eval mode too
static spp_status tf_forward(const spp_transformer_desc* d, void* stream, const char* who, const AttnDrop& dr) {
  return attn_entry(d, who, dr, [&] { return tf_check_rows(d, who, false); }, [&] {
    dispatch_fwd(d->x_elem, d->heads, d->C, dr.on(), [&](auto tin, auto q, auto c, auto drop, const Shape& sh) {
      using Tin = typename decltype(tin)::type;
      hipLaunchKernelGGL((k_transformer_fwd<Tin, decltype(q)::value, decltype(c)::value, decltype(drop)::value>),
                         dim3(grid_of(d->num_targets, sh.lpr_log2)), dim3(kAttnNT), 0, as_stream(stream), d->rowptr_dev,
                         d->col_dev, d->num_targets, static_cast<const Tin*>(d->q_dev), d->q_stride_elems,
                         static_cast<const Tin*>(d->k_dev), d->k_stride_elems, static_cast<const Tin*>(d->v_dev),
                         d->v_stride_elems, d->scale, sh.lpr_log2, sh.seg_log2, sh.g_log2, (int)d->heads, d->out_dev,
                         d->row_max_dev, d->row_sum_dev, dr.args());
    });
  });
}

// T == 0: nothing is touched, grad_k / grad_v stay as the caller zeroed them
static spp_status tf_backward(const spp_transformer_desc* d, void* stream, const char* who, const AttnDrop& dr) {
  return attn_entry(d, who, dr, [&] { return tf_check_rows(d, who, true); }, [&] {
    dispatch_bwd(d->x_elem, d->heads, d->C, dr.on(), [&](auto tin, auto n, auto s, auto drop, const BwdShape& sh) {
      using Tin = typename decltype(tin)::type;
      hipLaunchKernelGGL((k_transformer_bwd<Tin, decltype(n)::value, decltype(s)::value, decltype(drop)::value>),
                         dim3(grid_of(d->num_targets, sh.lpt_log2)), dim3(kAttnNT), 0, as_stream(stream), d->rowptr_dev,
                         d->col_dev, d->num_targets, static_cast<const Tin*>(d->q_dev), d->q_stride_elems,
                         static_cast<const Tin*>(d->k_dev), d->k_stride_elems, static_cast<const Tin*>(d->v_dev),
                         d->v_stride_elems, d->scale, sh.lpt_log2, sh.seg_log2, sh.c_log2, (int)d->heads, d->out_dev,
                         d->row_max_dev, d->row_sum_dev, d->grad_out_dev, d->grad_q_dev, d->grad_k_dev, d->grad_v_dev,
                         dr.args());
    });
  });
}

SPP_ATTN_ENTRIES(spp_transformer_forward, spp_transformer_forward_drop, spp_transformer_desc, tf_forward)
SPP_ATTN_ENTRIES(spp_transformer_backward, spp_transformer_backward_drop, spp_transformer_desc, tf_backward)
