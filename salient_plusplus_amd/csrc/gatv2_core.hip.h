// What the GATv2 forward kernels share (gatv2.hip: k_gatv2_fwd over an MFG hop; graph_gatv2.hip: k_graph_gatv2_rows /
// k_graph_gatv2_long over rows of the resident graph): the lane mapping, the logit of an entry, the step of a head's
// online softmax and the merge of two states.  ONE body for both translation units: a short row of the graph kernels
// is the bits of k_gatv2_fwd because it runs these very functions.  The lane mapping, State and butterfly are
// TransformerConv's as well (transformer_core.hip.h), and so is the host section for all four translation units
// (gatv2.hip, transformer_conv.hip, graph_gatv2.hip, graph_transformer.hip): the refusals of (heads, C), the launch
// geometry, and the forward's (NQ, CPH) and the backward's (NS, SPH) dispatch.
//
// 4 columns per lane: piece p = q * lpr + lane holds columns 4p .. 4p + 3, q < NQ chunks of lpr = min(64, D / 4) lanes.
// A head is G = C / 4 consecutive pieces: G <= lpr lanes of one chunk (CPH = 1: a lane sees NQ heads, one per chunk) or
// CPH = G / lpr whole chunks (a lane sees NQ / CPH heads).  A lane's partial dot of a head is the sum over its CPH
// chunks, four products each, from 0.f in chunk order; the partials are added by an xor butterfly over the min(G, lpr)
// lanes of the head's segment, widest step first, so every lane of the segment holds the logit and runs the head's
// online softmax for its own columns.  That order is fixed by (H, C) and by nothing else.
//
// kDrop (attention dropout of the training pair, spp.h f3x) is a compile-time parameter of take, result and walk that
// defaults to false: the graph kernels and the p = 0 training forward instantiate the bodies they always had.  With
// kDrop the softmax (mm, ss) takes every entry as before and only acc skips a dropped one.
#pragma once

#include "act_keep.hip.h"

#include <algorithm>
#include <type_traits>

namespace spp {
namespace gatv2 {

// Every product and sum below is written out: `#pragma clang fp contract(off)` in each body and fmaf where a fused
// multiply-add is meant.  Left to the compiler's contraction, the same source came out with different last bits in
// different kernels; written out, the kernels that run these bodies agree bit for bit by construction.
__device__ __forceinline__ float lrelu(float v, float slope) {
#pragma clang fp contract(off)
  return v > 0.f ? v : v * slope;
}
// a.x l_x, then one fused multiply-add per further column, in column order
__device__ __forceinline__ float dot_lrelu(const f4& a, const f4& x, const f4& r, float slope) {
#pragma clang fp contract(off)
  return fmaf(a.w, lrelu(x.w + r.w, slope),
              fmaf(a.z, lrelu(x.z + r.z, slope), fmaf(a.y, lrelu(x.y + r.y, slope), a.x * lrelu(x.x + r.x, slope))));
}

// what a lane keeps of its target for the whole row: att and x_r[t] for its columns, and where it sits
template <int NQ, int CPH>
struct Lane {
  static constexpr int HL = NQ / CPH;           // heads a lane takes part in
  static constexpr int NB = NQ <= 2 ? 4 : 2;    // neighbours in flight (NQ = 4: 16 columns per lane and neighbour)
  f4 av[NQ], rv[NQ];
  float slope;
  int lpr, lane, seg_log2;
  __device__ __forceinline__ int64_t col0(int q) const { return ((int64_t)q * lpr + lane) * 4; }
  template <typename Tin>
  __device__ __forceinline__ void load(const float* __restrict__ att, const Tin* xr_row) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      av[q] = load4(att + col0(q));
      rv[q] = load4(xr_row + col0(q));
    }
  }
  // the lane's partial dots of one row piece set, one per head
  __device__ __forceinline__ void partial(const f4 (&xv)[NQ], float (&pd)[HL]) const {
#pragma clang fp contract(off)
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) {
      pd[hl] = 0.f;
#pragma unroll
      for (int q = hl * CPH; q < (hl + 1) * CPH; ++q) pd[hl] += dot_lrelu(av[q], xv[q], rv[q], slope);
    }
  }
};

// the softmax state of the lane's heads over some entries, for the lane's columns: (m, s) per head, acc per piece
template <int NQ, int CPH>
struct State {
  static constexpr int HL = NQ / CPH;
  f4 acc[NQ];
  float mm[HL], ss[HL];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) mm[hl] = -INFINITY, ss[hl] = 0.f;
  }
  // one more entry of head hl with logit sc and row pieces xv (expf: spp.h f3v says why).  kDrop: an entry with
  // keep = false counts in (mm, ss) like any other and leaves acc alone
  template <bool kDrop = false>
  __device__ __forceinline__ void take(int hl, float sc, const f4 (&xv)[NQ], [[maybe_unused]] bool keep = true) {
#pragma clang fp contract(off)
    if (sc > mm[hl]) {
      const float r = expf(mm[hl] - sc);  // (m = -inf: r = 0, and s, acc are 0)
#pragma unroll
      for (int q = hl * CPH; q < (hl + 1) * CPH; ++q) {
        acc[q].x *= r; acc[q].y *= r; acc[q].z *= r; acc[q].w *= r;
      }
      ss[hl] *= r;
      mm[hl] = sc;
    }
    const float w = expf(sc - mm[hl]);
    ss[hl] += w;
    if constexpr (kDrop)
      if (!keep) return;
#pragma unroll
    for (int q = hl * CPH; q < (hl + 1) * CPH; ++q) {
      acc[q] = {fmaf(w, xv[q].x, acc[q].x), fmaf(w, xv[q].y, acc[q].y), fmaf(w, xv[q].z, acc[q].z),
                fmaf(w, xv[q].w, acc[q].w)};
    }
  }
  // the state of the entries behind this one's (graph_gat.hip's merge with expf).  *this is finite (it began with the
  // self loop); o may be empty: then o.m = -inf, f2 = 0 and f1 = 1, and nothing changes
  __device__ __forceinline__ void merge(const State& o) {
#pragma clang fp contract(off)
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) {
      const float m = fmaxf(mm[hl], o.mm[hl]);
      const float f1 = expf(mm[hl] - m), f2 = expf(o.mm[hl] - m);
      ss[hl] = fmaf(o.ss[hl], f2, ss[hl] * f1);
#pragma unroll
      for (int q = hl * CPH; q < (hl + 1) * CPH; ++q)
        acc[q] = {fmaf(f2, o.acc[q].x, acc[q].x * f1), fmaf(f2, o.acc[q].y, acc[q].y * f1),
                  fmaf(f2, o.acc[q].z, acc[q].z * f1), fmaf(f2, o.acc[q].w, acc[q].w * f1)};
      mm[hl] = m;
    }
  }
  // piece q of the result: acc / s, as a product by the reciprocal; kDrop: by scale / s, scale = 1 / (1 - p)
  template <bool kDrop = false>
  __device__ __forceinline__ f4 result(int q, [[maybe_unused]] float scale = 1.f) const {
#pragma clang fp contract(off)
    const float inv = (kDrop ? scale : 1.f) / ss[q / CPH];
    return {acc[q].x * inv, acc[q].y * inv, acc[q].z * inv, acc[q].w * inv};
  }
};

// adds every value of v over the lanes of a head's segment, widest step first; all lanes end with the same bits
template <int N>
__device__ __forceinline__ void butterfly(float (&v)[N], int seg_log2) {
#pragma clang fp contract(off)
  for (int d = (1 << seg_log2) >> 1; d >= 1; d >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], d, kWave);
}

// kDrop: what a lane needs to draw the keep bits of its heads (act_keep.hip.h attn_keep_head): the call's threshold and
// seed, the head count, and the global head behind each of the lane's HL local ones
template <int HL>
struct Drop {
  ActArgs a;
  int H;
  int head[HL];
};

// the self loop's state of a target whose SOURCE row is xl_row: m = e_tt, s = 1, acc = x_l[t]
template <typename Tin, int NQ, int CPH>
__device__ __forceinline__ void self_state(State<NQ, CPH>& st, const Lane<NQ, CPH>& L, const Tin* xl_row) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) st.acc[q] = load4(xl_row + L.col0(q));
  L.partial(st.acc, st.mm);
#pragma unroll
  for (int hl = 0; hl < State<NQ, CPH>::HL; ++hl) st.ss[hl] = 1.f;
  butterfly(st.mm, L.seg_log2);
}

// st continued over target t's entries col[b .. e) in CSR order, every entry equal to t skipped.  NB neighbours per
// round: ids, then rows, then partial dots, then ONE butterfly whose steps carry all NB * HL values (one dependent
// reduction per entry was the slow version).  x_rows >= 0: an entry outside [0, x_rows) is node 0 in every respect;
// x_rows < 0: the ids are taken as they are (an MFG hop's).  b, e and t are the same for all lanes of the group.
// kDrop: CSR entry k is softmax entry k of the keep rule (a skipped diagonal entry still owns its index); every lane
// draws for its own heads, dr->head, and the draws are issued with the rows' loads, ahead of the butterfly.
template <bool kDrop = false, typename Tin, int NQ, int CPH>
__device__ __forceinline__ void walk(State<NQ, CPH>& st, const Lane<NQ, CPH>& L, const Tin* xl, int64_t xl_stride,
                                     const int64_t* __restrict__ col, int64_t b, int64_t e, int64_t t, int64_t x_rows,
                                     [[maybe_unused]] const Drop<NQ / CPH>* dr = nullptr) {
  constexpr int HL = NQ / CPH, NB = Lane<NQ, CPH>::NB;
  for (int64_t k0 = b; k0 < e; k0 += NB) {
    int64_t j[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      j[u] = col[k0 + u < e ? k0 + u : e - 1];  // clamped, unpredicated
      if (x_rows >= 0 && (uint64_t)j[u] >= (uint64_t)x_rows) j[u] = 0;
    }
    f4 xv[NB][NQ];
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
      for (int q = 0; q < NQ; ++q) xv[u][q] = load4(xl + j[u] * xl_stride + L.col0(q));
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
    for (int u = 0; u < NB; ++u) {
      float one[HL];
      L.partial(xv[u], one);
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) pd[u * HL + hl] = one[hl];
    }
    butterfly(pd, L.seg_log2);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (k0 + u >= e || j[u] == t) continue;  // set_diag drops existing diagonal entries
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) {
        if constexpr (kDrop) st.template take<true>(hl, pd[u * HL + hl], xv[u], keep[u * HL + hl]);
        else st.take(hl, pd[u * HL + hl], xv[u]);
      }
    }
  }
}

// ---- host ----
static inline int log2_of(int64_t v) {
  int l = 0;
  while ((1ll << l) < v) ++l;
  return l;
}
static inline bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// The shapes the kernels are built for, refused in the order and the words include/spp.h documents for every GATv2 and
// TransformerConv entry, training and graph alike.  Two helpers: the training entries check their element code between
// the head count and C.
static inline spp_status check_heads(const char* who, int32_t heads) {
  SPP_REQUIRE(heads == 1 || heads == 2 || heads == 4 || heads == 8, "%s: heads must be 1, 2, 4 or 8 (got %d)", who,
              (int)heads);
  return SPP_OK;
}
static inline spp_status check_channels(const char* who, int64_t heads, int64_t C) {
  SPP_REQUIRE(C > 0 && C % 4 == 0, "%s: needs C > 0 and C %% 4 == 0 (got %lld)", who, (long long)C);
  SPP_REQUIRE(pow2(C / 4), "%s: built for C / 4 a power of two (got C = %lld)", who, (long long)C);
  SPP_REQUIRE(C <= 1024 && heads * C <= 1024, "%s: needs D = heads * C <= 1024", who);
  return SPP_OK;
}

// the launch geometry of D = heads * C columns (heads in {1, 2, 4, 8}, C / 4 a power of two, D <= 1024)
struct Shape {
  int lpr_log2, seg_log2, g_log2, nq, cph;
};
static inline Shape shape_of(int64_t heads, int64_t C) {
  const int64_t G = C / 4, P = heads * G;
  Shape s;
  s.lpr_log2 = lanes_log2(P);
  const int64_t lpr = 1ll << s.lpr_log2;
  s.nq = (int)(P / lpr), s.cph = (int)std::max<int64_t>(1, G / lpr);
  s.seg_log2 = log2_of(std::min<int64_t>(G, lpr)), s.g_log2 = log2_of(G);
  return s;
}

template <int N> using IC = std::integral_constant<int, N>;
// fn(IC<NQ>{}, IC<CPH>{}): the forward's chunks per lane and chunks per head
template <class Fn>
static void with_fwd_shape(int nq, int cph, Fn&& fn) {
  switch (nq * 8 + cph) {
    case 1 * 8 + 1: fn(IC<1>{}, IC<1>{}); break;
    case 2 * 8 + 1: fn(IC<2>{}, IC<1>{}); break;
    case 2 * 8 + 2: fn(IC<2>{}, IC<2>{}); break;
    case 4 * 8 + 1: fn(IC<4>{}, IC<1>{}); break;
    case 4 * 8 + 2: fn(IC<4>{}, IC<2>{}); break;
    default: fn(IC<4>{}, IC<4>{}); break;
  }
}
// fn(IC<NS>{}, IC<SPH>{}): the backward's steps per lane and steps per head (NS / SPH <= 8 heads)
template <class Fn>
static void with_bwd_shape(int ns, int sph, Fn&& fn) {
  switch (ns * 32 + sph) {
    case 1 * 32 + 1: fn(IC<1>{}, IC<1>{}); break;
    case 2 * 32 + 1: fn(IC<2>{}, IC<1>{}); break;
    case 2 * 32 + 2: fn(IC<2>{}, IC<2>{}); break;
    case 4 * 32 + 1: fn(IC<4>{}, IC<1>{}); break;
    case 4 * 32 + 2: fn(IC<4>{}, IC<2>{}); break;
    case 4 * 32 + 4: fn(IC<4>{}, IC<4>{}); break;
    case 8 * 32 + 1: fn(IC<8>{}, IC<1>{}); break;
    case 8 * 32 + 2: fn(IC<8>{}, IC<2>{}); break;
    case 8 * 32 + 4: fn(IC<8>{}, IC<4>{}); break;
    case 8 * 32 + 8: fn(IC<8>{}, IC<8>{}); break;
    case 16 * 32 + 2: fn(IC<16>{}, IC<2>{}); break;
    case 16 * 32 + 4: fn(IC<16>{}, IC<4>{}); break;
    case 16 * 32 + 8: fn(IC<16>{}, IC<8>{}); break;
    default: fn(IC<16>{}, IC<16>{}); break;
  }
}

}  // namespace gatv2
}  // namespace spp
