// f3: GAT training over an MFG hop -- the full-width pair (k_gat_fwd / k_gat_bwd, attention over projected rows) and
// the aggregate-then-project family (k_gat_mh_*, templated on the head count, with attention dropout) behind every
// spp_gat_* entry of include/spp.h.  Moved out of aggregate.hip, kernels unchanged; the transposed hop of the gather
// backward is transpose_hop.hip.h's, the keep rule of the attention dropout act_keep.hip.h's.
#include "act_keep.hip.h"
#include "elem_io.hip.h"
#include "gatv2_core.hip.h"  // check_heads: the head counts of every attention entry, one rule and one message
#include "transpose_hop.hip.h"

#include <algorithm>
#include <type_traits>

// ================================================================================================
// GATConv(heads=1) message passing over an MFG hop (reference: driver/models.py:195-231 uses
// torch_geometric.nn.GATConv(bias=False, heads=1) on ((x, x_target), adj_t)):
//     e_ij  = leaky_relu(a_src[j] + a_dst[i], slope)     for j in row i without its diagonal entry, plus j = i
//             (GATConv adds self loops with set_diag: exactly one (i, i) entry per target)
//     out_i = sum_j softmax_j(e_ij) * h[j,:]
// One pass over the neighbour rows with a running maximum (the rescaling trick of online softmax).
// ================================================================================================
namespace spp {

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

__global__ __launch_bounds__(kAggNT) void k_gat_fwd(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                    int64_t T, const float* __restrict__ h, int64_t F,
                                                    const float* __restrict__ a_src, const float* __restrict__ a_dst,
                                                    float slope, int lpr_log2, float* __restrict__ out,
                                                    float* __restrict__ row_max, float* __restrict__ row_sum) {
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kAggNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  const float ad = a_dst[t];
  // every lane of the group walks the same edges, so the softmax statistics need no exchange
  float m = lrelu(a_src[t] + ad, slope);  // the self loop
  float ssum = 1.f;
  for (int64_t c0 = lane; c0 < F || c0 == lane; c0 += lpr) {  // at least one sweep even if F < lpr
    const bool has = c0 < F;
    float acc = has ? h[t * F + c0] : 0.f;
    float mm = lrelu(a_src[t] + ad, slope), ss = 1.f;
    for (int64_t k = b; k < e; ++k) {
      const int64_t j = col[k];
      if (j == t) continue;  // set_diag drops existing diagonal entries
      const float sc = lrelu(a_src[j] + ad, slope);
      if (sc > mm) {
        const float r = __expf(mm - sc);
        acc *= r;
        ss *= r;
        mm = sc;
      }
      const float w = __expf(sc - mm);
      ss += w;
      if (has) acc += w * h[j * F + c0];
    }
    if (has) out[t * F + c0] = acc / ss;
    m = mm;
    ssum = ss;
  }
  if (lane == 0) {
    row_max[t] = m;
    row_sum[t] = ssum;
  }
}

// grad_h[j,:] += a_ij * g_i;  grad_e_ij = a_ij * (g_i . h_j - g_i . out_i) * lrelu'(raw);  grad_a_src[j] += grad_e_ij;
// grad_a_dst[i] = sum_j grad_e_ij.  One wavefront-sized group per target reduces the dot products.
__global__ __launch_bounds__(kAggNT) void k_gat_bwd(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                    int64_t T, const float* __restrict__ h, int64_t F,
                                                    const float* __restrict__ a_src, const float* __restrict__ a_dst,
                                                    float slope, const float* __restrict__ out,
                                                    const float* __restrict__ row_max, const float* __restrict__ row_sum,
                                                    const float* __restrict__ g, float* __restrict__ grad_h,
                                                    float* __restrict__ grad_a_src, float* __restrict__ grad_a_dst) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t t = ((int64_t)blockIdx.x * kAggNT + threadIdx.x) / kWave;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  const float ad = a_dst[t], m = row_max[t], inv_s = 1.f / row_sum[t];
  float go = 0.f;  // g_i . out_i
  for (int64_t c = lane; c < F; c += kWave) go += g[t * F + c] * out[t * F + c];
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) go += __shfl_xor(go, d, kWave);
  float gad = 0.f;
  for (int64_t k = b - 1; k < e; ++k) {  // k == b-1 stands for the self loop
    const int64_t j = (k < b) ? t : col[k];
    if (k >= b && j == t) continue;
    const float raw = a_src[j] + ad;
    const float a = __expf(lrelu(raw, slope) - m) * inv_s;
    float gh = 0.f;  // g_i . h_j
    for (int64_t c = lane; c < F; c += kWave) {
      const float gv = g[t * F + c];
      gh += gv * h[j * F + c];
      unsafeAtomicAdd(grad_h + j * F + c, a * gv);
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) gh += __shfl_xor(gh, d, kWave);
    const float ge = a * (gh - go) * (raw > 0.f ? 1.f : slope);
    gad += ge;
    if (lane == 0) unsafeAtomicAdd(grad_a_src + j, ge);
  }
  if (lane == 0) grad_a_dst[t] = gad;
}

// ================================================================================================
// GATConv, aggregate-then-project form.  GATConv computes h = W x for every SOURCE row and then
//   out_i = sum_j alpha_ij h_j,   alpha_ij = softmax_j(leaky_relu(att_src . h_j + att_dst . h_i)).
// Both uses of h are linear in x:  att_src . (W x_j) = x_j . (W^T att_src)  and  sum_j alpha_ij W x_j =
// W (sum_j alpha_ij x_j).  So the attention logits come from two K-vectors v_src = W^T att_src and
// v_dst = W^T att_dst, the aggregation runs over the RAW rows (128-wide fp16 in layer 1 instead of
// 256-wide fp32) and only the T aggregated target rows are projected: layer 1 of the papers-scale batch
// drops from a 947 k-row GEMM (62 GFLOP, and as much again for its weight gradient) to a 164 k-row one.
//
// With PyG's `heads` = H, W [H*C, K] is H blocks W_h of C rows;  v_src^h = W_h^T att_src[h],  v_dst^h = W_h^T att_dst[h]
// (V_src, V_dst: [H, K]).  Per head h:
//   a_src[j,h] = x_j . v_src^h,  a_dst[i,h] = x_i . v_dst^h,  alpha^h = softmax over row i of leaky_relu(a_src + a_dst),
//   z[i,h,:] = sum_j alpha_ij^h x_j    (RAW rows, K wide)  -> out_i^h = W_h z[i,h,:].
// Every kernel below is templated on H (1, 2, 4 or 8; heads = 1 is the H = 1 instance, not code of its own) and walks
// the edges ONCE for all heads: one load of the row chunk and one load of the H logits per edge, shared by the heads;
// what grows with H are the registers (H softmax states and accumulators) and z ([T, H, K]).
// Layouts: a_src [S, H], a_dst [T, H], V [H, K], z and grad_z [T, H, K], row_max / row_sum [T, H], alpha_e [E, H],
// alpha_self [T, H]; all fp32, row-major.  Per head, the order of operations does not depend on H.
// ================================================================================================
__device__ __forceinline__ f4 load4v(const float* p) { return load4(p); }

// o[h] = p[h], h < H, in 16-byte (H % 4 == 0), 8-byte (H == 2) or scalar (H == 1) loads: p is 4 * min(H, 4)-byte aligned
template <int H>
__device__ __forceinline__ void load_heads(const float* p, float (&o)[H]) {
  if constexpr (H % 4 == 0) {
#pragma unroll
    for (int q = 0; q < H; q += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + q);
      o[q] = v.x; o[q + 1] = v.y; o[q + 2] = v.z; o[q + 3] = v.w;
    }
  } else if constexpr (H == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    o[0] = v.x; o[1] = v.y;
  } else {
    o[0] = *p;
  }
}
template <int H>
__device__ __forceinline__ void store_heads(float* p, const float (&v)[H]) {
  if constexpr (H % 4 == 0) {
#pragma unroll
    for (int q = 0; q < H; q += 4) *reinterpret_cast<float4*>(p + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
  } else if constexpr (H == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  } else {
    p[0] = v[0];
  }
}

// a_src[j,h] = x_j . v_src^h  (all S rows);  a_dst[j,h] = x_j . v_dst^h  (the first T rows: the targets)
// A group of lpr lanes takes kDotRows consecutive rows; their loads are issued back to back (row index clamped,
// not predicated: with one row per group and a predicate the kernel had ONE load in flight per lane and ran
// at a third of the HBM rate).  2H dot products per row; H = 8 takes half as many rows per group (2H accumulators
// per row).
constexpr int kDotRows = 8;
template <int H>
constexpr int mh_dot_rows() { return H <= 4 ? kDotRows : kDotRows / 2; }
template <typename Tin, int H>
__global__ __launch_bounds__(kAggNT) void k_gat_mh_rowdot(const Tin* __restrict__ x, int64_t x_stride, int64_t S, int64_t T,
                                                          int64_t K, const float* __restrict__ v_src,
                                                          const float* __restrict__ v_dst, int lpr_log2,
                                                          float* __restrict__ a_src, float* __restrict__ a_dst) {
  constexpr int R = mh_dot_rows<H>();
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t j0 = (((int64_t)blockIdx.x * kAggNT + threadIdx.x) >> lpr_log2) * R;
  if (j0 >= S) return;  // whole groups leave together (the shuffles below stay inside a group)
  float ds[R][H], dd[R][H];
#pragma unroll
  for (int u = 0; u < R; ++u)
#pragma unroll
    for (int h = 0; h < H; ++h) ds[u][h] = dd[u][h] = 0.f;
  for (int64_t c = (int64_t)lane * 4; c < K; c += (int64_t)lpr * 4) {
    f4 xv[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {  // clamped, unpredicated: all R loads in flight
      const int64_t j = j0 + u < S ? j0 + u : S - 1;
      xv[u] = load4(x + j * x_stride + c);
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const f4 vs = load4v(v_src + h * K + c), vd = load4v(v_dst + h * K + c);
#pragma unroll
      for (int u = 0; u < R; ++u) {
        ds[u][h] += xv[u].x * vs.x + xv[u].y * vs.y + xv[u].z * vs.z + xv[u].w * vs.w;
        dd[u][h] += xv[u].x * vd.x + xv[u].y * vd.y + xv[u].z * vd.z + xv[u].w * vd.w;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < R; ++u)
#pragma unroll
    for (int h = 0; h < H; ++h)
      for (int d = lpr >> 1; d >= 1; d >>= 1) {  // the lpr lanes of a row are consecutive lanes of one wavefront
        ds[u][h] += __shfl_xor(ds[u][h], d, kWave);
        dd[u][h] += __shfl_xor(dd[u][h], d, kWave);
      }
  if (lane == 0) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int64_t j = j0 + u;
      if (j < S) {
        store_heads<H>(a_src + j * H, ds[u]);
        if (j < T) store_heads<H>(a_dst + j * H, dd[u]);
      }
    }
  }
}

// out_src[h,c] += sum_j w_src[j,h] x[j,c] over all rows;  out_dst[h,c] += sum_{j<T} w_dst[j,h] x[j,c]
// (out zeroed by the caller).  The 2H column sums of a workgroup leave through one LDS buffer, one after the other;
// H = 1 has room for both of its sums (32 KiB) and takes a single barrier round.
// (1024 threads and 4096 rows per workgroup: every workgroup ends in K atomics per head onto the SAME addresses, and
// with 256-thread / 1024-row workgroups those 924 x 256 same-address adds were most of the single-head kernel's time)
constexpr int kColsumNT = 1024;
template <typename Tin, int H>
__global__ __launch_bounds__(kColsumNT) void k_gat_mh_colsum(const Tin* __restrict__ x, int64_t x_stride, int64_t S,
                                                             int64_t T, int64_t K, const float* __restrict__ w_src,
                                                             const float* __restrict__ w_dst, int64_t rows_per_wg,
                                                             float* __restrict__ out_src, float* __restrict__ out_dst) {
  constexpr int kPer = H == 1 ? 2 : 1;          // column sums per barrier round
  __shared__ float red[kPer][kColsumNT][4];
  constexpr int kU = H <= 2 ? 4 : 2;            // independent rows in flight, no predicate on a load (8 at H = 1: slower)
  const int groups = (int)(K / 4);              // threads that share a row (K/4 <= kColsumNT)
  const int cg = threadIdx.x % groups;          // this thread's 4 columns
  const int rsub = threadIdx.x / groups, rstep = kColsumNT / groups;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = r0 + rows_per_wg < S ? r0 + rows_per_wg : S;
  f4 as[H], ad[H];
#pragma unroll
  for (int h = 0; h < H; ++h) as[h] = ad[h] = f4{0.f, 0.f, 0.f, 0.f};
  auto add = [](f4& a, float w, const f4& v) { a.x += w * v.x; a.y += w * v.y; a.z += w * v.z; a.w += w * v.w; };
  if (rsub < rstep) {
    int64_t j = r0 + rsub;
    const int64_t tlast = T > 0 ? T - 1 : 0;
    const float* __restrict__ wdp = T > 0 ? w_dst : w_src;  // (w_dst may be NULL without targets)
    for (; j + (kU - 1) * rstep < r1; j += kU * rstep) {
      f4 xv[kU];
      float ws[kU][H], wd[kU][H];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t ju = j + u * rstep;
        xv[u] = load4(x + ju * x_stride + (int64_t)cg * 4);
        load_heads<H>(w_src + ju * H, ws[u]);
        load_heads<H>(wdp + (ju < T ? ju : tlast) * H, wd[u]);
        if (ju >= T)
#pragma unroll
          for (int h = 0; h < H; ++h) wd[u][h] = 0.f;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u)
#pragma unroll
        for (int h = 0; h < H; ++h) {
          add(as[h], ws[u][h], xv[u]);
          add(ad[h], wd[u][h], xv[u]);
        }
    }
    for (; j < r1; j += rstep) {
      const f4 xv = load4(x + j * x_stride + (int64_t)cg * 4);
      float ws[H];
      load_heads<H>(w_src + j * H, ws);
#pragma unroll
      for (int h = 0; h < H; ++h) add(as[h], ws[h], xv);
      if (j < T) {
        float wd[H];
        load_heads<H>(w_dst + j * H, wd);
#pragma unroll
        for (int h = 0; h < H; ++h) add(ad[h], wd[h], xv);
      }
    }
  }
#pragma unroll
  for (int o = 0; o < 2 * H; o += kPer) {
#pragma unroll
    for (int p = 0; p < kPer; ++p) {
      const f4 v = o + p < H ? as[o + p] : ad[o + p - H];
      float* r = red[p][threadIdx.x];
      r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    }
    __syncthreads();
    if (threadIdx.x < groups) {  // one thread per column group sums the row sub-lanes, then one atomic per column
      float s4[kPer][4] = {};
      for (int r = 0; r < rstep; ++r)
#pragma unroll
        for (int p = 0; p < kPer; ++p)
          for (int q = 0; q < 4; ++q) s4[p][q] += red[p][r * groups + threadIdx.x][q];
#pragma unroll
      for (int p = 0; p < kPer; ++p) {
        if (o + p >= H && r0 >= T) continue;  // no target among this workgroup's rows
        float* out = o + p < H ? out_src + (o + p) * K : out_dst + (o + p - H) * K;
        for (int q = 0; q < 4; ++q) unsafeAtomicAdd(out + threadIdx.x * 4 + q, s4[p][q]);
      }
    }
    if (o + kPer < 2 * H) __syncthreads();
  }
}

// z[i,h,:] = sum_j alpha_ij^h x_j over row i (its diagonal entry dropped) plus the self loop; x rows fp16, bf16 or fp32,
// 4 columns per lane, online softmax (every lane of a row's group walks the same edges) with H softmax states and
// accumulators; per edge one load of the H logits and one of the row chunk, shared by the heads.
// kDrop (attention dropout, spp.h f3t): z[i,h,:] = sum_j q_ij^h alpha_ij^h x_j, q = keep / (1 - p) per (entry, head)
// from attn_keep_heads (entry k for CSR entry k, E + t for t's self loop).  The softmax runs over ALL entries (row_max
// and row_sum are the kDrop = false values); only the accumulator skips a dropped entry.  Every lane of a row's group
// hashes for itself: the walk has no cross-lane step to hand a draw over in, and the hashes overlap the loads' latency.
template <typename Tin, int H, bool kDrop>
__global__ __launch_bounds__(kAggNT) void k_gat_mh_agg_fwd(const int64_t* __restrict__ rowptr,
                                                           const int64_t* __restrict__ col, int64_t T,
                                                           const Tin* __restrict__ x, int64_t x_stride, int64_t K,
                                                           const float* __restrict__ a_src,
                                                           const float* __restrict__ a_dst, float slope, int lpr_log2,
                                                           float* __restrict__ z, float* __restrict__ row_max,
                                                           float* __restrict__ row_sum, ActArgs drop) {
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t t = ((int64_t)blockIdx.x * kAggNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  float ad[H], self[H];
  load_heads<H>(a_dst + t * H, ad);
  load_heads<H>(a_src + t * H, self);
#pragma unroll
  for (int h = 0; h < H; ++h) self[h] = lrelu(self[h] + ad[h], slope);
  [[maybe_unused]] bool kself[H];
  if constexpr (kDrop) attn_keep_heads<H>((uint64_t)(rowptr[T] + t), drop, kself);  // E = rowptr[T]
  for (int64_t c = (int64_t)lane * 4; c < K || c == (int64_t)lane * 4; c += (int64_t)lpr * 4) {
    const bool has = c < K;
    const f4 xt = has ? load4(x + t * x_stride + c) : f4{0.f, 0.f, 0.f, 0.f};
    f4 acc[H];
    float mm[H], ss[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      acc[h] = xt;
      if constexpr (kDrop)
        if (!kself[h]) acc[h] = f4{0.f, 0.f, 0.f, 0.f};
      mm[h] = self[h];
      ss[h] = 1.f;
    }
    // kNb neighbours per round: their ids, then their logits and rows, each issued back to back (clamped
    // indices, no predicated load); the online softmax then runs over registers.  One neighbour at a time
    // was two dependent round trips per edge.
    constexpr int kNb = 4;
    const int64_t cc = has ? c : 0;
    for (int64_t k0 = b; k0 < e; k0 += kNb) {
      int64_t j[kNb];
#pragma unroll
      for (int u = 0; u < kNb; ++u) j[u] = col[k0 + u < e ? k0 + u : e - 1];
      float as[kNb][H];
      f4 xv[kNb];
#pragma unroll
      for (int u = 0; u < kNb; ++u) {
        load_heads<H>(a_src + j[u] * H, as[u]);
        xv[u] = load4(x + j[u] * x_stride + cc);
      }
#pragma unroll
      for (int u = 0; u < kNb; ++u) {
        if (k0 + u >= e || j[u] == t) continue;  // set_diag drops existing diagonal entries
        [[maybe_unused]] bool keep[H];
        if constexpr (kDrop) attn_keep_heads<H>((uint64_t)(k0 + u), drop, keep);
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float sc = lrelu(as[u][h] + ad[h], slope);
          if (sc > mm[h]) {
            const float r = __expf(mm[h] - sc);
            acc[h].x *= r; acc[h].y *= r; acc[h].z *= r; acc[h].w *= r;
            ss[h] *= r;
            mm[h] = sc;
          }
          const float w = __expf(sc - mm[h]);
          ss[h] += w;
          if constexpr (kDrop)
            if (!keep[h]) continue;
          acc[h].x += w * xv[u].x; acc[h].y += w * xv[u].y; acc[h].z += w * xv[u].z; acc[h].w += w * xv[u].w;
        }
      }
    }
    if (has) {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float inv = (kDrop ? drop.scale : 1.f) / ss[h];
        *reinterpret_cast<float4*>(z + (t * H + h) * K + c) =
            make_float4(acc[h].x * inv, acc[h].y * inv, acc[h].z * inv, acc[h].w * inv);
      }
    }
    if (lane == 0 && c == 0) {
      store_heads<H>(row_max + t * H, mm);
      store_heads<H>(row_sum + t * H, ss);
    }
  }
}

// One wavefront per target i (lpt = min(64, K rounded up to a power of two) lanes; K/4 for kVec).  Per head
// go^h = g_i^h . z_i^h,  gh^h = g_i^h . x_j,  ge^h = alpha_ij^h (gh^h - go^h) lrelu'(raw);  grad_a_src[j,h] += ge^h,
// grad_a_dst[i,h] = sum_j ge^h, and grad_x[j,:] += sum_h alpha_ij^h g_i^h  (only when grad_x != NULL: the first layer's
// input needs no gradient, which saves E x K atomics): the heads are summed first, so there is ONE fp32 atomic per
// column per edge whatever H is.
// kVec: 4 columns per lane (no input gradient wanted: only dot products, 8/16-byte loads);
// otherwise one column per lane and step, c = lane + lpt * i: consecutive lanes touch consecutive columns, so a group's
// loads and -- what matters -- its fp32 atomics are contiguous 4 * lpt-byte segments (the atomic units run at full
// rate on contiguous 256-byte wave instructions and ~17x slower on scattered ones).
// alpha_e / alpha_self (optional): the attention weights of every CSR entry (0 for a dropped diagonal entry) and of
// every target's self loop -- what the input gradient by GATHER over the transposed hop needs (k_gat_mh_gx_gather).
// kDrop (attention dropout, the forward's (p, seed)): go is taken on the saved DROPPED z, so sum_k alpha_ik q_ik gh_ik = go
// and ge^h = alpha (q gh - go) lrelu'(raw) -- a dropped entry still sends -alpha go to its logits;  grad_x takes q alpha,
// and alpha_e / alpha_self hold q alpha (what k_gat_mh_gx_gather multiplies by); ge uses the plain alpha.
template <typename Tin, int H, bool kVec, bool kDrop>
__global__ __launch_bounds__(kAggNT) void k_gat_mh_agg_bwd(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t T, const Tin* __restrict__ x,
    int64_t x_stride, int64_t K, const float* __restrict__ a_src, const float* __restrict__ a_dst, float slope,
    const float* __restrict__ z, const float* __restrict__ row_max, const float* __restrict__ row_sum,
    const float* __restrict__ g, int lpt_log2, float* __restrict__ grad_x, float* __restrict__ grad_a_src,
    float* __restrict__ grad_a_dst, float* __restrict__ alpha_e, float* __restrict__ alpha_self, ActArgs drop) {
  const int lpt = 1 << lpt_log2;
  const int lane = threadIdx.x & (lpt - 1);
  const int64_t t = ((int64_t)blockIdx.x * kAggNT + threadIdx.x) >> lpt_log2;
  const bool live = t < T;
  const int64_t b = live ? rowptr[t] : 0, e = live ? rowptr[t + 1] : -1;
  [[maybe_unused]] const int64_t E = kDrop ? rowptr[T] : 0;  // the self loops' draws come after the E entries'
  float ad[H], m[H], inv_s[H];
#pragma unroll
  for (int h = 0; h < H; ++h) ad[h] = m[h] = inv_s[h] = 0.f;
  if (live) {
    load_heads<H>(a_dst + t * H, ad);
    load_heads<H>(row_max + t * H, m);
    load_heads<H>(row_sum + t * H, inv_s);
#pragma unroll
    for (int h = 0; h < H; ++h) inv_s[h] = 1.f / inv_s[h];
  }
  auto group_sum = [&](float v) {
    for (int d = lpt >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
  };
  const float* __restrict__ gt = g + (live ? t : 0) * H * K;  // target t's [H, K] block of grad_z (and of z)
  const float* __restrict__ zt = z + (live ? t : 0) * H * K;
  float go[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    go[h] = 0.f;
    if (live) {
      if (kVec) {
        for (int64_t c = (int64_t)lane * 4; c < K; c += (int64_t)lpt * 4) {
          const f4 gv = load4(gt + h * K + c), zv = load4(zt + h * K + c);
          go[h] += gv.x * zv.x + gv.y * zv.y + gv.z * zv.z + gv.w * zv.w;
        }
      } else {
        for (int64_t c = lane; c < K; c += lpt) go[h] += gt[h * K + c] * zt[h * K + c];
      }
    }
    go[h] = group_sum(go[h]);
  }
  // the targets sharing a wavefront have different degrees: every group runs to the longest row of its
  // wavefront so that the shuffles stay convergent
  int64_t n = live ? e - b + 1 : 0;
  for (int d = lpt; d < kWave; d <<= 1) {
    const int64_t o = __shfl_xor((long long)n, d, kWave);
    n = o > n ? o : n;
  }
  float gad[H];
#pragma unroll
  for (int h = 0; h < H; ++h) gad[h] = 0.f;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = b - 1 + i;  // k == b-1 stands for the self loop
    const bool on = live && k < e;
    const int64_t j = !on ? 0 : ((k < b) ? t : col[k]);
    const bool use = on && !(k >= b && j == t);  // set_diag drops existing diagonal entries
    float gh[H], a[H], raw[H];
    [[maybe_unused]] float q[H];  // kDrop: keep / (1 - p)
#pragma unroll
    for (int h = 0; h < H; ++h) gh[h] = a[h] = raw[h] = 0.f;
    if constexpr (kDrop) {
#pragma unroll
      for (int h = 0; h < H; ++h) q[h] = 0.f;
    }
    if (use) {
      load_heads<H>(a_src + j * H, raw);
      if constexpr (kDrop) {
        bool keep[H];
        attn_keep_heads<H>((uint64_t)(k < b ? E + t : k), drop, keep);
#pragma unroll
        for (int h = 0; h < H; ++h) q[h] = keep[h] ? drop.scale : 0.f;
      }
      if (kVec) {  // before the logits are used: their load and the rows' are in flight together
        for (int64_t c = (int64_t)lane * 4; c < K; c += (int64_t)lpt * 4) {
          const f4 xv = load4(x + j * x_stride + c);
#pragma unroll
          for (int h = 0; h < H; ++h) {
            const f4 gv = load4(gt + h * K + c);
            gh[h] += gv.x * xv.x + gv.y * xv.y + gv.z * xv.z + gv.w * xv.w;
          }
        }
      }
#pragma unroll
      for (int h = 0; h < H; ++h) {
        raw[h] += ad[h];
        a[h] = __expf(lrelu(raw[h], slope) - m[h]) * inv_s[h];
      }
      if (!kVec) {
        for (int64_t c = lane; c < K; c += lpt) {
          const float xv = load1(x + j * x_stride + c);
          float gx = 0.f;
#pragma unroll
          for (int h = 0; h < H; ++h) {
            const float gv = gt[h * K + c];
            gh[h] += gv * xv;
            gx += (kDrop ? q[h] * a[h] : a[h]) * gv;
          }
          unsafeAtomicAdd(grad_x + j * K + c, gx);
        }
      }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) gh[h] = group_sum(gh[h]);
    if (alpha_e && on && lane == 0) {  // 0: dropped entry
      if constexpr (kDrop) {
        float qa[H];
#pragma unroll
        for (int h = 0; h < H; ++h) qa[h] = q[h] * a[h];
        store_heads<H>(k < b ? alpha_self + t * H : alpha_e + k * H, qa);
      } else {
        store_heads<H>(k < b ? alpha_self + t * H : alpha_e + k * H, a);
      }
    }
    if (use) {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float ge = a[h] * ((kDrop ? q[h] * gh[h] : gh[h]) - go[h]) * (raw[h] > 0.f ? 1.f : slope);
        gad[h] += ge;
        if (lane == 0) unsafeAtomicAdd(grad_a_src + j * H + h, ge);
      }
    }
  }
  if (live && lane == 0) store_heads<H>(grad_a_dst + t * H, gad);
}

// Input gradient of the layer by GATHER (no fp32 atomics, no zero fill, no separate rank-1 passes):
//   grad_x[s,:] = sum over the targets t of s: sum_h alpha_ts^h grad_z[t,h,:]
//   (+ the self loop's sum_h alpha_ss^h grad_z[s,h,:], s < T) + sum_h grad_a_src[s,h] v_src^h (+ grad_a_dst[s,h] v_dst^h, s < T)
//   -- a_src = x V_src^T, a_dst = x[:T] V_dst^T.  Every term is added to the accumulator on its own, in this order.
template <int H>
__global__ __launch_bounds__(kAggNT) void k_gat_mh_gx_gather(
    const int32_t* __restrict__ start, const int32_t* __restrict__ ttgt, const int32_t* __restrict__ tedge,
    const float* __restrict__ alpha_e, const float* __restrict__ alpha_self, int64_t T, int64_t S,
    const float* __restrict__ g, int64_t K, int lpr_log2, const float* __restrict__ grad_a_src,
    const float* __restrict__ grad_a_dst, const float* __restrict__ v_src, const float* __restrict__ v_dst,
    float* __restrict__ grad_x) {
  const int lpr = 1 << lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t srow = ((int64_t)blockIdx.x * kAggNT + threadIdx.x) >> lpr_log2;
  if (srow >= S) return;
  const int32_t b = start[srow], e = start[srow + 1];
  const bool tgt = srow < T;
  float gas[H], gad[H], aself[H];
  load_heads<H>(grad_a_src + srow * H, gas);
#pragma unroll
  for (int h = 0; h < H; ++h) gad[h] = aself[h] = 0.f;
  if (tgt) {
    load_heads<H>(grad_a_dst + srow * H, gad);
    load_heads<H>(alpha_self + srow * H, aself);
  }
  auto add = [](float4& a, float w, const float4& v) { a.x += w * v.x; a.y += w * v.y; a.z += w * v.z; a.w += w * v.w; };
  const int64_t HK = H * K;
  for (int64_t c = (int64_t)lane * 4; c < K; c += (int64_t)lpr * 4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int h = 0; h < H; ++h) add(acc, gas[h], *reinterpret_cast<const float4*>(v_src + h * K + c));
    if (tgt) {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        add(acc, gad[h], *reinterpret_cast<const float4*>(v_dst + h * K + c));
        add(acc, aself[h], *reinterpret_cast<const float4*>(g + srow * HK + h * K + c));
      }
    }
    int32_t k = b;
    for (; k + 1 < e; k += 2) {  // two independent targets in flight
      const int32_t t0 = ttgt[k], t1 = ttgt[k + 1];
      float w0[H], w1[H];
      load_heads<H>(alpha_e + (int64_t)tedge[k] * H, w0);
      load_heads<H>(alpha_e + (int64_t)tedge[k + 1] * H, w1);
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float4 v0 = *reinterpret_cast<const float4*>(g + (int64_t)t0 * HK + h * K + c);
        const float4 v1 = *reinterpret_cast<const float4*>(g + (int64_t)t1 * HK + h * K + c);
        add(acc, w0[h], v0);
        add(acc, w1[h], v1);
      }
    }
    if (k < e) {
      const int32_t t0 = ttgt[k];
      float w0[H];
      load_heads<H>(alpha_e + (int64_t)tedge[k] * H, w0);
#pragma unroll
      for (int h = 0; h < H; ++h) add(acc, w0[h], *reinterpret_cast<const float4*>(g + (int64_t)t0 * HK + h * K + c));
    }
    *reinterpret_cast<float4*>(grad_x + srow * K + c) = acc;
  }
}

// keep[entry, h] (0 / 1) of the E + T softmax entries, by the device function the aggregate kernels call
template <int H>
__global__ __launch_bounds__(kAggNT) void k_gat_mh_attn_keep(int64_t n, ActArgs drop, uint8_t* __restrict__ keep_out) {
  const int64_t entry = (int64_t)blockIdx.x * kAggNT + threadIdx.x;
  if (entry >= n) return;
  bool keep[H];
  attn_keep_heads<H>((uint64_t)entry, drop, keep);
#pragma unroll
  for (int h = 0; h < H; ++h) keep_out[entry * H + h] = keep[h] ? 1 : 0;
}

}  // namespace spp

using namespace spp;

extern "C" spp_status spp_gat_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                      const float* h_dev, int64_t F, const float* a_src_dev, const float* a_dst_dev,
                                      float negative_slope, float* out_dev, float* row_max_dev, float* row_sum_dev,
                                      void* stream) {
  SPP_REQUIRE(num_targets >= 0 && F >= 0, "spp_gat_forward: negative size");
  if (num_targets == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(rowptr_dev && h_dev && a_src_dev && a_dst_dev && out_dev && row_max_dev && row_sum_dev,
              "spp_gat_forward: NULL buffer");
  const int lpr_log2 = lanes_log2(F);
  const unsigned grid = (unsigned)ceil_div(num_targets << lpr_log2, kAggNT);
  hipLaunchKernelGGL(k_gat_fwd, dim3(grid), dim3(kAggNT), 0, as_stream(stream), rowptr_dev, col_dev, num_targets, h_dev,
                     F, a_src_dev, a_dst_dev, negative_slope, lpr_log2, out_dev, row_max_dev, row_sum_dev);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" spp_status spp_gat_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                       const float* h_dev, int64_t F, const float* a_src_dev, const float* a_dst_dev,
                                       float negative_slope, const float* out_dev, const float* row_max_dev,
                                       const float* row_sum_dev, const float* grad_out_dev, float* grad_h_dev,
                                       float* grad_a_src_dev, float* grad_a_dst_dev, void* stream) {
  SPP_REQUIRE(num_targets >= 0 && F >= 0, "spp_gat_backward: negative size");
  if (num_targets == 0 || F == 0) return SPP_OK;
  SPP_REQUIRE(rowptr_dev && h_dev && a_src_dev && a_dst_dev && out_dev && row_max_dev && row_sum_dev && grad_out_dev &&
                  grad_h_dev && grad_a_src_dev && grad_a_dst_dev,
              "spp_gat_backward: NULL buffer");
  const unsigned grid = (unsigned)ceil_div(num_targets * kWave, kAggNT);
  hipLaunchKernelGGL(k_gat_bwd, dim3(grid), dim3(kAggNT), 0, as_stream(stream), rowptr_dev, col_dev, num_targets, h_dev,
                     F, a_src_dev, a_dst_dev, negative_slope, out_dev, row_max_dev, row_sum_dev, grad_out_dev,
                     grad_h_dev, grad_a_src_dev, grad_a_dst_dev);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// ---- the aggregate-then-project GAT entries (include/spp.h: spp_gat_mh_* and, as their heads = 1 spelling, the
// spp_gat_logits / spp_gat_aggregate_* entries that predate the head count) ----
// fn(std::integral_constant<int, H>{}) for heads = H in {1, 2, 4, 8} (checked by gat_check)
template <class Fn>
static void with_heads(int32_t heads, Fn&& fn) {
  switch (heads) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    default: fn(std::integral_constant<int, 8>{}); break;
  }
}
static bool al16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
// the per-head arrays are read and written H floats at a time (load_heads): 4, 8 and 16-byte accesses at H = 1, 2, >= 4
static bool al_heads(const void* p, int32_t heads) {
  return reinterpret_cast<uintptr_t>(p) % (4 * std::min<int32_t>(heads, 4)) == 0;
}

// One hop's arguments as the host code passes them: every exported entry fills the fields its signature has, by name
// (the others stay 0 / NULL), and calls the one static implementation of its operation, which reads fields.  Host side
// only: the kernels take scalars and pointers.  A buffer is const here whichever entry it came from; the launch that
// WRITES one (the logits: a_src, a_dst; the forward: z, row_max, row_sum; the backward: grad_a_src, grad_a_dst) hands
// it over through out() -- the exported signature of that entry declares it writable.
struct GatHop {
  const char* who;  // the exported entry, for the errors
  const int64_t *rowptr, *col;
  int64_t T, S, E;
  const void* x;  // [S, K] rows of x_elem, x_stride elements apart; the targets are its first T rows
  int32_t x_elem;
  int64_t x_stride, K;
  int32_t heads;
  const float *a_src, *a_dst;  // [S, H], [T, H]
  float slope;
  const float *z, *row_max, *row_sum;  // [T, H, K], [T, H], [T, H]
  const float* grad_z;
  float* grad_x;                          // [S, K]; NULL in the atomic form: not wanted
  const float *grad_a_src, *grad_a_dst;  // [S, H], [T, H]
  const float *v_src, *v_dst;            // [H, K]
  float *grad_v_src, *grad_v_dst;
  void* workspace;
  int64_t workspace_bytes;
  void* stream;
  AttnDrop drop;  // spp_gat_mh_*_drop (spp.h f3t): checked right after gat_check, before the sizes
};
static float* out(const float* p) { return const_cast<float*>(p); }

// The head count, and x: x_elem is the element code of its rows (0 fp32, 1 fp16, 2 bf16); the softmax statistics, z and
// all gradients stay fp32.  Every entry runs these checks before anything else.
static spp_status gat_check(const GatHop& h) {
  SPP_TRY(gatv2::check_heads(h.who, h.heads));
  SPP_REQUIRE(elem_ok(h.x_elem), "%s: unknown element code %d", h.who, (int)h.x_elem);
  const int64_t esz = elem_bytes(h.x_elem);
  SPP_REQUIRE(h.K > 0 && h.K % 4 == 0 && h.K / 4 <= spp::kAggNT && h.x_stride >= h.K &&
                  (h.x_stride * esz) % (4 * esz) == 0 && reinterpret_cast<uintptr_t>(h.x) % (4 * esz) == 0,
              "%s: needs K %% 4 == 0, K <= %d and rows aligned to 4 elements", h.who, 4 * spp::kAggNT);
  return SPP_OK;
}

static spp_status gat_logits(const GatHop& h) {
  SPP_TRY(gat_check(h));
  SPP_REQUIRE(h.S >= h.T && h.T >= 0, "%s: bad sizes", h.who);
  if (h.S == 0) return SPP_OK;
  SPP_REQUIRE(h.x && h.v_src && h.v_dst && h.a_src && (h.a_dst || h.T == 0) && al16(h.v_src) && al16(h.v_dst) &&
                  al_heads(h.a_src, h.heads) && al_heads(h.a_dst, h.heads),
              "%s: NULL or unaligned buffer", h.who);
  const int lpr_log2 = lanes_log2(h.K / 4);
  with_elem(h.x_elem, [&](auto tin) {
    with_heads(h.heads, [&](auto hh) {
      using Tin = typename decltype(tin)::type;
      constexpr int H = decltype(hh)::value;
      const unsigned grid = (unsigned)ceil_div(ceil_div(h.S, mh_dot_rows<H>()) << lpr_log2, kAggNT);
      hipLaunchKernelGGL((k_gat_mh_rowdot<Tin, H>), dim3(grid), dim3(kAggNT), 0, as_stream(h.stream),
                         static_cast<const Tin*>(h.x), h.x_stride, h.S, h.T, h.K, h.v_src, h.v_dst, lpr_log2,
                         out(h.a_src), out(h.a_dst));
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

static spp_status gat_logits_backward(const GatHop& h) {
  SPP_TRY(gat_check(h));
  SPP_REQUIRE(h.S >= h.T && h.T >= 0, "%s: bad sizes", h.who);
  SPP_REQUIRE(h.grad_v_src && h.grad_v_dst, "%s: NULL output", h.who);
  SPP_REQUIRE(h.S == 0 || (h.x && h.grad_a_src && (h.grad_a_dst || h.T == 0) && al_heads(h.grad_a_src, h.heads) &&
                           al_heads(h.grad_a_dst, h.heads)),
              "%s: NULL or unaligned input", h.who);
  hipStream_t st = as_stream(h.stream);
  SPP_HIP_TRY(hipMemsetAsync(h.grad_v_src, 0, sizeof(float) * (size_t)(h.heads * h.K), st));
  SPP_HIP_TRY(hipMemsetAsync(h.grad_v_dst, 0, sizeof(float) * (size_t)(h.heads * h.K), st));
  if (h.S == 0) return SPP_OK;
  // every workgroup ends in atomics onto the SAME 2 H K addresses: about one workgroup per CU, between 1024 and 4096
  // rows each
  const int64_t rows_per_wg = std::max<int64_t>(1024, std::min<int64_t>(4096, ceil_div(h.S, 256)));
  const unsigned grid = (unsigned)ceil_div(h.S, rows_per_wg);
  with_elem(h.x_elem, [&](auto tin) {
    with_heads(h.heads, [&](auto hh) {
      using Tin = typename decltype(tin)::type;
      hipLaunchKernelGGL((k_gat_mh_colsum<Tin, decltype(hh)::value>), dim3(grid), dim3(kColsumNT), 0, st,
                         static_cast<const Tin*>(h.x), h.x_stride, h.S, h.T, h.K, h.grad_a_src, h.grad_a_dst,
                         rows_per_wg, h.grad_v_src, h.grad_v_dst);
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

static spp_status gat_aggregate_forward(const GatHop& h) {
  SPP_TRY(gat_check(h));
  SPP_TRY(attn_drop_check(h.drop, h.who));
  SPP_REQUIRE(h.T >= 0, "%s: negative size", h.who);
  if (h.T == 0) return SPP_OK;
  SPP_REQUIRE(h.rowptr && h.x && h.a_src && h.a_dst && h.z && h.row_max && h.row_sum && al16(h.z) &&
                  al_heads(h.a_src, h.heads) && al_heads(h.a_dst, h.heads) && al_heads(h.row_max, h.heads) &&
                  al_heads(h.row_sum, h.heads),
              "%s: NULL or unaligned buffer", h.who);
  const int lpr_log2 = lanes_log2(h.K / 4);
  const unsigned grid = (unsigned)ceil_div(h.T << lpr_log2, kAggNT);
  const ActArgs da = h.drop.args();
  with_elem(h.x_elem, [&](auto tin) {
    with_heads(h.heads, [&](auto hh) {
      with_drop(h.drop.on(), [&](auto drop) {
        using Tin = typename decltype(tin)::type;
        hipLaunchKernelGGL((k_gat_mh_agg_fwd<Tin, decltype(hh)::value, decltype(drop)::value>), dim3(grid),
                           dim3(kAggNT), 0, as_stream(h.stream), h.rowptr, h.col, h.T, static_cast<const Tin*>(h.x),
                           h.x_stride, h.K, h.a_src, h.a_dst, h.slope, lpr_log2, out(h.z), out(h.row_max),
                           out(h.row_sum), da);
      });
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// the launch of k_gat_mh_agg_bwd (arguments checked by the caller); grad_x == NULL: the vector form.  alpha_e /
// alpha_self: the gather form's attention weights in its workspace, else NULL
static spp_status gat_backward_launch(const GatHop& h, float* grad_x, float* alpha_e, float* alpha_self) {
  const bool vec = grad_x == nullptr;
  const ActArgs da = h.drop.args();
  const int lpt_log2 = lanes_log2(vec ? h.K / 4 : h.K);
  const unsigned grid = (unsigned)ceil_div(h.T << lpt_log2, kAggNT);
  with_elem_vec(h.x_elem, vec, [&](auto tin, auto v) {
    with_heads(h.heads, [&](auto hh) {
      with_drop(h.drop.on(), [&](auto drop) {
        using Tin = typename decltype(tin)::type;
        hipLaunchKernelGGL((k_gat_mh_agg_bwd<Tin, decltype(hh)::value, decltype(v)::value, decltype(drop)::value>),
                           dim3(grid), dim3(kAggNT), 0, as_stream(h.stream), h.rowptr, h.col, h.T,
                           static_cast<const Tin*>(h.x), h.x_stride, h.K, h.a_src, h.a_dst, h.slope, h.z, h.row_max,
                           h.row_sum, h.grad_z, lpt_log2, grad_x, out(h.grad_a_src), out(h.grad_a_dst), alpha_e,
                           alpha_self, da);
      });
    });
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

static bool gat_backward_bufs_ok(const GatHop& h) {
  return h.rowptr && h.x && h.a_src && h.a_dst && h.z && h.row_max && h.row_sum && h.grad_z && h.grad_a_src &&
         h.grad_a_dst && al16(h.z) && al16(h.grad_z) && al_heads(h.a_src, h.heads) && al_heads(h.a_dst, h.heads) &&
         al_heads(h.row_max, h.heads) && al_heads(h.row_sum, h.heads) && al_heads(h.grad_a_src, h.heads) &&
         al_heads(h.grad_a_dst, h.heads);
}

static spp_status gat_aggregate_backward(const GatHop& h) {
  SPP_TRY(gat_check(h));
  SPP_TRY(attn_drop_check(h.drop, h.who));
  SPP_REQUIRE(h.T >= 0, "%s: negative size", h.who);
  if (h.T == 0) return SPP_OK;
  SPP_REQUIRE(gat_backward_bufs_ok(h), "%s: NULL or unaligned buffer", h.who);
  return gat_backward_launch(h, h.grad_x, nullptr, nullptr);
}

extern "C" int64_t spp_gat_mh_aggregate_backward_gather_workspace_bytes(int64_t num_targets, int64_t num_sources,
                                                                        int64_t num_edges, int32_t heads) {
  if (heads != 1 && heads != 2 && heads != 4 && heads != 8) return SPP_ERR_INVALID;
  // alpha_e [E, H] | alpha_self [T, H] | the transposed hop with edge ids   (each 16-byte aligned)
  return align16(4 * heads * num_edges) + align16(4 * heads * num_targets) +
         transpose_hop_bytes(num_targets, num_sources, num_edges, true);
}

// gat_aggregate_backward with the input gradient by GATHER over the transposed hop: grad_x [S, K] is written
// completely, including the rank-1 terms of the logits (grad_a_src[s,h] v_src^h, grad_a_dst[s,h] v_dst^h for s < T)
// that the atomic form leaves to the caller.  grad_a_src [S, H] is zeroed by the caller as before.
static spp_status gat_aggregate_backward_gather(const GatHop& h) {
  SPP_TRY(gat_check(h));
  SPP_TRY(attn_drop_check(h.drop, h.who));
  SPP_REQUIRE(h.T >= 0 && h.S >= h.T && h.E >= 0, "%s: bad sizes", h.who);
  if (h.S == 0) return SPP_OK;
  SPP_REQUIRE(h.S < (1ll << 31) && h.E < (1ll << 31), "%s: 32-bit indices", h.who);
  SPP_REQUIRE(h.T == 0 || gat_backward_bufs_ok(h), "%s: NULL or unaligned buffer", h.who);
  SPP_REQUIRE(h.rowptr && h.v_src && h.v_dst && h.grad_x && h.grad_a_src && h.workspace && al16(h.v_src) &&
                  al16(h.v_dst) && al16(h.grad_x) && al_heads(h.grad_a_src, h.heads) && al16(h.workspace),
              "%s: NULL or unaligned buffer (v, grad_x and the workspace: 16 bytes)", h.who);
  SPP_REQUIRE(h.workspace_bytes >= spp_gat_mh_aggregate_backward_gather_workspace_bytes(h.T, h.S, h.E, h.heads),
              "%s: workspace too small", h.who);
  hipStream_t st = as_stream(h.stream);
  float* alpha_e = static_cast<float*>(h.workspace);
  float* alpha_self = alpha_e + align16(4 * h.heads * h.E) / 4;
  const int64_t alpha_bytes = align16(4 * h.heads * h.E) + align16(4 * h.heads * h.T);
  // the attention weights of every entry and head + grad_a_src / grad_a_dst (no input gradient by atomics)
  if (h.T > 0) SPP_TRY(gat_backward_launch(h, nullptr, alpha_e, alpha_self));
  TransposedHop hop;
  SPP_TRY(transpose_hop(h.rowptr, h.col, h.T, h.S, h.E, true, static_cast<char*>(h.workspace) + alpha_bytes,
                        h.workspace_bytes - alpha_bytes, st, &hop));
  const int lpr_log2 = lanes_log2(h.K / 4);
  const unsigned grid = (unsigned)ceil_div(h.S << lpr_log2, kAggNT);
  with_heads(h.heads, [&](auto hh) {
    hipLaunchKernelGGL((k_gat_mh_gx_gather<decltype(hh)::value>), dim3(grid), dim3(kAggNT), 0, st, hop.start, hop.tcol,
                       hop.tedge, alpha_e, alpha_self, h.T, h.S, h.grad_z, h.K, lpr_log2, h.grad_a_src, h.grad_a_dst,
                       h.v_src, h.v_dst, h.grad_x);
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// ---- the exported spellings: with the head count (spp_gat_mh_*), with heads fixed at 1 (the entries that predate it)
// and with attention dropout (spp_gat_mh_*_drop, spp.h f3t: (p, training, seed) after `stream`) ----
extern "C" spp_status spp_gat_mh_logits(const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t num_sources,
                                        int64_t num_targets, int64_t K, int32_t heads, const float* v_src_dev,
                                        const float* v_dst_dev, float* a_src_dev, float* a_dst_dev, void* stream) {
  return gat_logits({.who = "spp_gat_mh_logits", .T = num_targets, .S = num_sources, .x = x_dev, .x_elem = x_elem,
                     .x_stride = x_stride_elems, .K = K, .heads = heads, .a_src = a_src_dev, .a_dst = a_dst_dev,
                     .v_src = v_src_dev, .v_dst = v_dst_dev, .stream = stream});
}

extern "C" spp_status spp_gat_logits(const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t num_sources,
                                     int64_t num_targets, int64_t K, const float* v_src_dev, const float* v_dst_dev,
                                     float* a_src_dev, float* a_dst_dev, void* stream) {
  return gat_logits({.who = "spp_gat_logits", .T = num_targets, .S = num_sources, .x = x_dev, .x_elem = x_elem,
                     .x_stride = x_stride_elems, .K = K, .heads = 1, .a_src = a_src_dev, .a_dst = a_dst_dev,
                     .v_src = v_src_dev, .v_dst = v_dst_dev, .stream = stream});
}

extern "C" spp_status spp_gat_mh_logits_backward(const void* x_dev, int32_t x_elem, int64_t x_stride_elems,
                                                 int64_t num_sources, int64_t num_targets, int64_t K, int32_t heads,
                                                 const float* grad_a_src_dev, const float* grad_a_dst_dev,
                                                 float* grad_v_src_dev, float* grad_v_dst_dev, void* stream) {
  return gat_logits_backward({.who = "spp_gat_mh_logits_backward", .T = num_targets, .S = num_sources, .x = x_dev,
                              .x_elem = x_elem, .x_stride = x_stride_elems, .K = K, .heads = heads,
                              .grad_a_src = grad_a_src_dev, .grad_a_dst = grad_a_dst_dev, .grad_v_src = grad_v_src_dev,
                              .grad_v_dst = grad_v_dst_dev, .stream = stream});
}

extern "C" spp_status spp_gat_logits_backward(const void* x_dev, int32_t x_elem, int64_t x_stride_elems,
                                              int64_t num_sources, int64_t num_targets, int64_t K,
                                              const float* grad_a_src_dev, const float* grad_a_dst_dev,
                                              float* grad_v_src_dev, float* grad_v_dst_dev, void* stream) {
  return gat_logits_backward({.who = "spp_gat_logits_backward", .T = num_targets, .S = num_sources, .x = x_dev,
                              .x_elem = x_elem, .x_stride = x_stride_elems, .K = K, .heads = 1,
                              .grad_a_src = grad_a_src_dev, .grad_a_dst = grad_a_dst_dev, .grad_v_src = grad_v_src_dev,
                              .grad_v_dst = grad_v_dst_dev, .stream = stream});
}

extern "C" spp_status spp_gat_mh_aggregate_forward(const int64_t* rowptr_dev, const int64_t* col_dev,
                                                   int64_t num_targets, const void* x_dev, int32_t x_elem,
                                                   int64_t x_stride_elems, int64_t K, int32_t heads,
                                                   const float* a_src_dev, const float* a_dst_dev, float negative_slope,
                                                   float* z_dev, float* row_max_dev, float* row_sum_dev, void* stream) {
  return gat_aggregate_forward({.who = "spp_gat_mh_aggregate_forward", .rowptr = rowptr_dev, .col = col_dev,
                                .T = num_targets, .x = x_dev, .x_elem = x_elem, .x_stride = x_stride_elems, .K = K,
                                .heads = heads, .a_src = a_src_dev, .a_dst = a_dst_dev, .slope = negative_slope,
                                .z = z_dev, .row_max = row_max_dev, .row_sum = row_sum_dev, .stream = stream});
}

extern "C" spp_status spp_gat_aggregate_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                                const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K,
                                                const float* a_src_dev, const float* a_dst_dev, float negative_slope,
                                                float* z_dev, float* row_max_dev, float* row_sum_dev, void* stream) {
  return gat_aggregate_forward({.who = "spp_gat_aggregate_forward", .rowptr = rowptr_dev, .col = col_dev,
                                .T = num_targets, .x = x_dev, .x_elem = x_elem, .x_stride = x_stride_elems, .K = K,
                                .heads = 1, .a_src = a_src_dev, .a_dst = a_dst_dev, .slope = negative_slope,
                                .z = z_dev, .row_max = row_max_dev, .row_sum = row_sum_dev, .stream = stream});
}

extern "C" spp_status spp_gat_mh_aggregate_forward_drop(const int64_t* rowptr_dev, const int64_t* col_dev,
                                                        int64_t num_targets, const void* x_dev, int32_t x_elem,
                                                        int64_t x_stride_elems, int64_t K, int32_t heads,
                                                        const float* a_src_dev, const float* a_dst_dev,
                                                        float negative_slope, float* z_dev, float* row_max_dev,
                                                        float* row_sum_dev, void* stream, float p, int32_t training,
                                                        uint64_t seed) {
  return gat_aggregate_forward({.who = "spp_gat_mh_aggregate_forward_drop", .rowptr = rowptr_dev, .col = col_dev,
                                .T = num_targets, .x = x_dev, .x_elem = x_elem, .x_stride = x_stride_elems, .K = K,
                                .heads = heads, .a_src = a_src_dev, .a_dst = a_dst_dev, .slope = negative_slope,
                                .z = z_dev, .row_max = row_max_dev, .row_sum = row_sum_dev, .stream = stream,
                                .drop = {true, p, training, seed}});
}

extern "C" spp_status spp_gat_mh_aggregate_backward(const int64_t* rowptr_dev, const int64_t* col_dev,
                                                    int64_t num_targets, const void* x_dev, int32_t x_elem,
                                                    int64_t x_stride_elems, int64_t K, int32_t heads,
                                                    const float* a_src_dev, const float* a_dst_dev,
                                                    float negative_slope, const float* z_dev, const float* row_max_dev,
                                                    const float* row_sum_dev, const float* grad_z_dev, float* grad_x_dev,
                                                    float* grad_a_src_dev, float* grad_a_dst_dev, void* stream) {
  return gat_aggregate_backward(
      {.who = "spp_gat_mh_aggregate_backward", .rowptr = rowptr_dev, .col = col_dev, .T = num_targets, .x = x_dev,
       .x_elem = x_elem, .x_stride = x_stride_elems, .K = K, .heads = heads, .a_src = a_src_dev, .a_dst = a_dst_dev,
       .slope = negative_slope, .z = z_dev, .row_max = row_max_dev, .row_sum = row_sum_dev, .grad_z = grad_z_dev,
       .grad_x = grad_x_dev, .grad_a_src = grad_a_src_dev, .grad_a_dst = grad_a_dst_dev, .stream = stream});
}

extern "C" spp_status spp_gat_aggregate_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                                 const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K,
                                                 const float* a_src_dev, const float* a_dst_dev, float negative_slope,
                                                 const float* z_dev, const float* row_max_dev, const float* row_sum_dev,
                                                 const float* grad_z_dev, float* grad_x_dev, float* grad_a_src_dev,
                                                 float* grad_a_dst_dev, void* stream) {
  return gat_aggregate_backward(
      {.who = "spp_gat_aggregate_backward", .rowptr = rowptr_dev, .col = col_dev, .T = num_targets, .x = x_dev,
       .x_elem = x_elem, .x_stride = x_stride_elems, .K = K, .heads = 1, .a_src = a_src_dev, .a_dst = a_dst_dev,
       .slope = negative_slope, .z = z_dev, .row_max = row_max_dev, .row_sum = row_sum_dev, .grad_z = grad_z_dev,
       .grad_x = grad_x_dev, .grad_a_src = grad_a_src_dev, .grad_a_dst = grad_a_dst_dev, .stream = stream});
}

extern "C" spp_status spp_gat_mh_aggregate_backward_drop(
    const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets, const void* x_dev, int32_t x_elem,
    int64_t x_stride_elems, int64_t K, int32_t heads, const float* a_src_dev, const float* a_dst_dev,
    float negative_slope, const float* z_dev, const float* row_max_dev, const float* row_sum_dev,
    const float* grad_z_dev, float* grad_x_dev, float* grad_a_src_dev, float* grad_a_dst_dev, void* stream, float p,
    int32_t training, uint64_t seed) {
  return gat_aggregate_backward(
      {.who = "spp_gat_mh_aggregate_backward_drop", .rowptr = rowptr_dev, .col = col_dev, .T = num_targets, .x = x_dev,
       .x_elem = x_elem, .x_stride = x_stride_elems, .K = K, .heads = heads, .a_src = a_src_dev, .a_dst = a_dst_dev,
       .slope = negative_slope, .z = z_dev, .row_max = row_max_dev, .row_sum = row_sum_dev, .grad_z = grad_z_dev,
       .grad_x = grad_x_dev, .grad_a_src = grad_a_src_dev, .grad_a_dst = grad_a_dst_dev, .stream = stream,
       .drop = {true, p, training, seed}});
}

extern "C" int64_t spp_gat_aggregate_backward_gather_workspace_bytes(int64_t num_targets, int64_t num_sources,
                                                                     int64_t num_edges) {
  return spp_gat_mh_aggregate_backward_gather_workspace_bytes(num_targets, num_sources, num_edges, 1);
}

extern "C" spp_status spp_gat_mh_aggregate_backward_gather(
    const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets, int64_t num_sources, int64_t num_edges,
    const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K, int32_t heads, const float* a_src_dev,
    const float* a_dst_dev, float negative_slope, const float* z_dev, const float* row_max_dev,
    const float* row_sum_dev, const float* grad_z_dev, const float* v_src_dev, const float* v_dst_dev,
    float* grad_x_dev, float* grad_a_src_dev, float* grad_a_dst_dev, void* workspace_dev, int64_t workspace_bytes,
    void* stream) {
  return gat_aggregate_backward_gather(
      {.who = "spp_gat_mh_aggregate_backward_gather", .rowptr = rowptr_dev, .col = col_dev, .T = num_targets,
       .S = num_sources, .E = num_edges, .x = x_dev, .x_elem = x_elem, .x_stride = x_stride_elems, .K = K,
       .heads = heads, .a_src = a_src_dev, .a_dst = a_dst_dev, .slope = negative_slope, .z = z_dev,
       .row_max = row_max_dev, .row_sum = row_sum_dev, .grad_z = grad_z_dev, .grad_x = grad_x_dev,
       .grad_a_src = grad_a_src_dev, .grad_a_dst = grad_a_dst_dev, .v_src = v_src_dev, .v_dst = v_dst_dev,
       .workspace = workspace_dev, .workspace_bytes = workspace_bytes, .stream = stream});
}

extern "C" spp_status spp_gat_aggregate_backward_gather(
    const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets, int64_t num_sources, int64_t num_edges,
    const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K, const float* a_src_dev,
    const float* a_dst_dev, float negative_slope, const float* z_dev, const float* row_max_dev,
    const float* row_sum_dev, const float* grad_z_dev, const float* v_src_dev, const float* v_dst_dev,
    float* grad_x_dev, float* grad_a_src_dev, float* grad_a_dst_dev, void* workspace_dev, int64_t workspace_bytes,
    void* stream) {
  return gat_aggregate_backward_gather(
      {.who = "spp_gat_aggregate_backward_gather", .rowptr = rowptr_dev, .col = col_dev, .T = num_targets,
       .S = num_sources, .E = num_edges, .x = x_dev, .x_elem = x_elem, .x_stride = x_stride_elems, .K = K, .heads = 1,
       .a_src = a_src_dev, .a_dst = a_dst_dev, .slope = negative_slope, .z = z_dev, .row_max = row_max_dev,
       .row_sum = row_sum_dev, .grad_z = grad_z_dev, .grad_x = grad_x_dev, .grad_a_src = grad_a_src_dev,
       .grad_a_dst = grad_a_dst_dev, .v_src = v_src_dev, .v_dst = v_dst_dev, .workspace = workspace_dev,
       .workspace_bytes = workspace_bytes, .stream = stream});
}

extern "C" spp_status spp_gat_mh_aggregate_backward_gather_drop(
    const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets, int64_t num_sources, int64_t num_edges,
    const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K, int32_t heads, const float* a_src_dev,
    const float* a_dst_dev, float negative_slope, const float* z_dev, const float* row_max_dev,
    const float* row_sum_dev, const float* grad_z_dev, const float* v_src_dev, const float* v_dst_dev,
    float* grad_x_dev, float* grad_a_src_dev, float* grad_a_dst_dev, void* workspace_dev, int64_t workspace_bytes,
    void* stream, float p, int32_t training, uint64_t seed) {
  return gat_aggregate_backward_gather(
      {.who = "spp_gat_mh_aggregate_backward_gather_drop", .rowptr = rowptr_dev, .col = col_dev, .T = num_targets,
       .S = num_sources, .E = num_edges, .x = x_dev, .x_elem = x_elem, .x_stride = x_stride_elems, .K = K,
       .heads = heads, .a_src = a_src_dev, .a_dst = a_dst_dev, .slope = negative_slope, .z = z_dev,
       .row_max = row_max_dev, .row_sum = row_sum_dev, .grad_z = grad_z_dev, .grad_x = grad_x_dev,
       .grad_a_src = grad_a_src_dev, .grad_a_dst = grad_a_dst_dev, .v_src = v_src_dev, .v_dst = v_dst_dev,
       .workspace = workspace_dev, .workspace_bytes = workspace_bytes, .stream = stream,
       .drop = {true, p, training, seed}});
}

// the mask the _drop entries apply, written out: keep [(E + T), H]
extern "C" spp_status spp_gat_mh_attn_keep(int64_t num_edges, int64_t num_targets, int32_t heads, float p, uint64_t seed,
                                           uint8_t* keep_dev, void* stream) {
  const char* who = "spp_gat_mh_attn_keep";
  SPP_REQUIRE(num_edges >= 0 && num_targets >= 0, "%s: negative size", who);
  SPP_TRY(gatv2::check_heads(who, heads));
  SPP_REQUIRE(p >= 0.f && p < 1.f, "%s: attention dropout needs 0 <= p < 1", who);
  const int64_t n = num_edges + num_targets;
  SPP_REQUIRE(n < (1ll << 31) * (int64_t)kAggNT, "%s: size out of range", who);
  if (n == 0) return SPP_OK;
  SPP_REQUIRE(keep_dev, "%s: NULL buffer", who);
  const ActArgs da = act_args(p, 1, seed);
  with_heads(heads, [&](auto hh) {
    hipLaunchKernelGGL((k_gat_mh_attn_keep<decltype(hh)::value>), dim3((unsigned)ceil_div(n, kAggNT)), dim3(kAggNT), 0,
                       as_stream(stream), n, da, keep_dev);
  });
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
