// What the TransformerConv forward kernels share (transformer_conv.hip: k_transformer_fwd over an MFG hop;
// graph_transformer.hip: k_graph_transformer_rows / k_graph_transformer_long over rows of the resident graph): the
// logit's summation tree and the walk over a stretch of CSR entries.  ONE body for both translation units, as
// gatv2_core.hip.h is for the GATv2 pair: a short row of the graph kernels is the bits of k_transformer_fwd because it
// runs this very function.  The lane mapping, State (take / merge / result), butterfly and the (NQ, CPH) dispatch are
// gatv2_core.hip.h's, unchanged.
//
// Merging chunk states here (graph_transformer.hip): TransformerConv adds no self loop, so State::merge's comment
// ("*this is finite: it began with the self loop") does not carry over by itself.  What holds instead: every chunk of a
// row that is cut into chunks has at least one entry (a row is cut only when it is longer than one chunk, and chunk j
// exists only if b + j * C_g < e), every entry is taken, so every chunk state that is merged has a finite m and s >= 1.
// The running state is chunk 0's, finite from the start.  The empty state (m = -inf) is parked only by a lane group
// whose chunk index is past the row's end, and that one is never merged.  Two empty states are never merged: it would
// compute expf(-inf - -inf) = NaN.
#pragma once

#include "gatv2_core.hip.h"

namespace spp {
namespace transformer {

using namespace gatv2;

// THE LOGIT'S SUMMATION TREE, walked bit for bit by the forward kernels (here) and the backward (transformer_conv.hip).
// The C products q[c] k[c] of a head, each rounded, are added pairwise by xor distance of the column index within the
// head, in the order 1, 2, then C / 2, C / 4, ..., 4; every addition is a rounded fp32 addition of two partial sums that
// are the same bits on both sides, so whoever holds a partner ends with the same bits.  Then ONE rounded product by
// scale.  No fused multiply-add anywhere in it (contraction is off in every kernel).  The backward recomputes
// alpha = expf(e - row_max) / row_sum from THIS e: with a logit added in another order, a row dominated by one entry got
// alpha = 1 + (e' - e) -- 1e-6 off at logits of 18, seen at model level -- where the forward's
// own weight is 1 to the bit.
// Forward: distances 1 and 2 are inside a lane's 4-column piece (piece4), distances >= 4 are piece distances: chunks of
// the head in the lane first (widest), then the butterfly over the head's lanes, widest first.
__device__ __forceinline__ float piece4(const f4& a, const f4& b) {
#pragma clang fp contract(off)
  return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
}

// neighbours in flight per round: every one is a k piece set AND a v piece set, twice gatv2's Lane::NB row data, so at
// NQ = 4 (16 columns per lane and row) one fewer than there: 2 * 2 * 16 = 64 registers of rows, as NQ = 2 has with 4.
// NB enters no result: the entries are taken one at a time in CSR order.
template <int NQ>
constexpr int tf_nb() { return NQ <= 2 ? 4 : 2; }

// st continued over the entries col[b .. e) in CSR order, every one taken (no self loop, diagonal entries kept, repeats
// counted).  qv: the lane's pieces of q[t], c0: their first columns.  Per round: NB ids, then their k and v pieces, then
// the partial dots (piece4, the head's chunks widest first), then ONE butterfly that carries all NB * HL values; the
// logit is the butterfly's sum times scale (one product, the same bits in every lane of the head's segment);
// State::take does the online softmax on the v pieces.  x_rows >= 0: an entry outside [0, x_rows) is node 0;
// x_rows < 0: the ids are taken as they are (an MFG hop's).  b and e are the same for all lanes of the group.
// kDrop (attention dropout of the training pair, spp.h f4a): CSR entry k is softmax entry k of the keep rule
// (its absolute position in col); every lane draws for its own heads, dr->head, and the draws are issued right after
// the rows' loads, ahead of the butterfly.  The softmax (mm, ss) takes every entry; only acc skips a dropped one.
template <int NB, bool kDrop = false, typename Tin, int NQ, int CPH>
__device__ __forceinline__ void walk(State<NQ, CPH>& st, const f4 (&qv)[NQ], const int64_t (&c0)[NQ], const Tin* km,
                                     int64_t k_stride, const Tin* vm, int64_t v_stride,
                                     const int64_t* __restrict__ col, int64_t b, int64_t e, int64_t x_rows,
                                     float scale, int seg_log2,
                                     [[maybe_unused]] const Drop<NQ / CPH>* dr = nullptr) {
#pragma clang fp contract(off)
  constexpr int HL = NQ / CPH;
  for (int64_t k0 = b; k0 < e; k0 += NB) {
    int64_t j[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      j[u] = col[k0 + u < e ? k0 + u : e - 1];  // clamped, unpredicated
      if (x_rows >= 0 && (uint64_t)j[u] >= (uint64_t)x_rows) j[u] = 0;
    }
    f4 kv[NB][NQ], vv[NB][NQ];
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        kv[u][q] = load4(km + j[u] * k_stride + c0[q]);
        vv[u][q] = load4(vm + j[u] * v_stride + c0[q]);
      }
    [[maybe_unused]] bool keep[NB * HL];
    if constexpr (kDrop) {
#pragma unroll
      for (int u = 0; u < NB; ++u)
#pragma unroll
        for (int hl = 0; hl < HL; ++hl)
          keep[u * HL + hl] = attn_keep_head((uint64_t)(k0 + u), dr->H, dr->head[hl], dr->a);
    }
    float pd[NB * HL];
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) {
        float ch[CPH];  // the head's chunks: piece distance 64 * (chunk distance), the widest of the tree's >= 4 part
#pragma unroll
        for (int q = 0; q < CPH; ++q) ch[q] = piece4(qv[hl * CPH + q], kv[u][hl * CPH + q]);
#pragma unroll
        for (int d = CPH / 2; d >= 1; d >>= 1)
#pragma unroll
          for (int q = 0; q < d; ++q) ch[q] += ch[q + d];
        pd[u * HL + hl] = ch[0];
      }
    butterfly(pd, seg_log2);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (k0 + u >= e) continue;
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) {
        if constexpr (kDrop) st.template take<true>(hl, pd[u * HL + hl] * scale, vv[u], keep[u * HL + hl]);
        else st.take(hl, pd[u * HL + hl] * scale, vv[u]);
      }
    }
  }
}

}  // namespace transformer
}  // namespace spp
