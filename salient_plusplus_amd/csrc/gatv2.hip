// f3v: GATv2Conv ("dynamic attention", Brody et al.) training over an MFG hop: the forward / backward pair behind
// spp_gatv2_forward / spp_gatv2_backward of include/spp.h.
//     x_l [S, H, C] = lin_l(x),   x_r [T, H, C] = lin_r(x_target)     (projected by the caller; x_r may alias x_l)
//     e_ij^h     = sum_c att[h,c] * leaky_relu(x_l[j,h,c] + x_r[i,h,c], slope)
//     out[i,h,:] = sum_j softmax_j(e_ij^h) * x_l[j,h,:]
// over row i without its diagonal entries (col == i) plus one self loop (i, i) whose message is SOURCE row i: the set_diag
// convention of gat.hip.  The nonlinearity sits between the projection and att, so GAT's aggregate-first trick
// (att . (W x_j) = x_j . (W^T att)) does not apply: every edge's logit is a C-wide dot product per head, reduced across
// lanes, and the hot loops below are their own.  What they keep from gat.hip: the per-head online softmax in the order
// self loop, then CSR; several neighbours' loads in flight per round; one fp32 atomic per column per edge on contiguous
// wave-wide segments for grad_xl; element I/O and the entry checks of elem_io.hip.h.
// Built for C / 4 a power of two (the per-head reduction is an xor butterfly over aligned lane segments); with H in
// {1, 2, 4, 8} D = H * C is then a power of two as well, 4 <= D <= 1024.
#include "attn_train.hip.h"

namespace spp {

using namespace gatv2;

// Forward.  The lane mapping, the logit, the online softmax and the walk over a row are gatv2_core.hip.h's (shared with
// the long-row kernels of graph_gatv2.hip): lpr lanes per target, 4 columns per lane and chunk, NB neighbours in flight,
// one butterfly per round.  The targets are the first T rows of x_l.  No atomics: the same bits in every run.
// kDrop (attention dropout, spp.h f3x): out[i,h,:] = sum_j q_ij^h alpha_ij^h x_l[j,h,:], q = keep / (1 - p) per (entry,
// head) by the keep rule of f3t (entry k for CSR entry k, E + t for t's self loop, E = rowptr[T]).  The softmax runs
// over ALL entries -- row_max and row_sum are the kDrop = false bits -- and only acc skips a dropped entry, the self
// loop's x_l[t] included.  The lane's head hl is global head ((hl * CPH) * lpr + lane) >> g_log2; every lane hashes for
// the heads it holds (the lanes of a head's segment draw the same bits).
template <typename Tin, int NQ, int CPH, bool kDrop>
__global__ __launch_bounds__(kAttnNT) void k_gatv2_fwd(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t T, const Tin* xl, int64_t xl_stride,
    const Tin* xr, int64_t xr_stride, const float* __restrict__ att, float slope, int lpr_log2, int seg_log2,
    int g_log2, int H, float* __restrict__ out, float* __restrict__ row_max, float* __restrict__ row_sum, ActArgs drop) {
  constexpr int HL = NQ / CPH;
  Lane<NQ, CPH> L;
  L.slope = slope, L.lpr = 1 << lpr_log2, L.lane = threadIdx.x & (L.lpr - 1), L.seg_log2 = seg_log2;
  const int64_t t = ((int64_t)blockIdx.x * kAttnNT + threadIdx.x) >> lpr_log2;
  if (t >= T) return;  // whole groups leave together (the shuffles below stay inside a group)
  L.load(att, xr + t * xr_stride);
  State<NQ, CPH> st;
  self_state(st, L, xl + t * xl_stride);  // the self loop's message: source row t
  if constexpr (kDrop) {
    Drop<HL> dr;
    fwd_drop_heads<CPH>(dr, drop, H, L.lpr, L.lane, g_log2);
    const uint64_t self = (uint64_t)(rowptr[T] + t);  // the self loops' draws come after the E = rowptr[T] entries'
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) {
      if (attn_keep_head(self, H, dr.head[hl], drop)) continue;
#pragma unroll
      for (int q = hl * CPH; q < (hl + 1) * CPH; ++q) st.acc[q] = {0.f, 0.f, 0.f, 0.f};
    }
    walk<true>(st, L, xl, xl_stride, col, rowptr[t], rowptr[t + 1], t, (int64_t)-1, &dr);
  } else {
    walk(st, L, xl, xl_stride, col, rowptr[t], rowptr[t + 1], t, (int64_t)-1);
  }
  fwd_store<kDrop, false>(st, t, L.lpr, L.lane, g_log2, H, drop.scale, out, row_max, row_sum);
}

// Backward.  ONE column per lane and step, c = lane + lpt * i, i < NS, lpt = min(64, D) lanes per target: a group's
// loads and -- what matters -- its fp32 atomics on grad_xl are contiguous 4 * lpt-byte segments (gat.hip,
// k_gat_mh_agg_bwd: the atomic units run at full rate on contiguous 256-byte wave instructions and ~17x slower on
// scattered ones); one atomic per column per edge.  A head is C consecutive columns: C <= lpt lanes of one step
// (SPH = 1) or SPH = C / 64 whole steps; a lane takes part in HL = NS / SPH heads.  Per entry the logit e^h (recomputed;
// alpha = expf(e - row_max) / row_sum, no [E, H] array) and gh^h = g_i . x_l[j] are reduced by one butterfly.
// A group walks tpg consecutive targets; its lanes keep the grad_att sums of their columns in registers over all of
// them, and a workgroup adds them up (across the groups of a wavefront by shuffles, across wavefronts through LDS) before
// its D atomics on grad_att (k_gat_mh_colsum's rule: every workgroup ends on the SAME addresses).
// lrelu'(0) = slope (v > 0 ? 1 : slope).
// kDrop (attention dropout, the forward's (p, seed)): go is taken on the saved DROPPED out, so sum_j q alpha gh = go and
// ge = alpha (q gh - go) is the softmax gradient again -- a dropped entry (q = 0) still sends -alpha go to its logit --
// and grad_xl[j] takes q alpha g_i + ge att d.  q = keep ? 1 / (1 - p) : 0 per (entry, head), the forward's draws: the
// lane's head hl is global head (lane + lpt * hl * SPH) >> c_log2, and every lane hashes for the heads it holds.
template <typename Tin, int NS, int SPH, bool kDrop>
__global__ __launch_bounds__(kAttnNT) void k_gatv2_bwd(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t T, const Tin* xl, int64_t xl_stride,
    const Tin* xr, int64_t xr_stride, const float* __restrict__ att, float slope, int lpt_log2, int seg_log2,
    int c_log2, int H, const float* __restrict__ out, const float* __restrict__ row_max,
    const float* __restrict__ row_sum, const float* __restrict__ g, int64_t tpg, float* __restrict__ grad_xl,
    float* __restrict__ grad_xr, float* __restrict__ grad_att, ActArgs drop) {
  constexpr int HL = NS / SPH;
  __shared__ float red[kAttnNT / kWave][NS][kWave];
  const int lpt = 1 << lpt_log2;
  const int lane = threadIdx.x & (lpt - 1);
  const int64_t D = (int64_t)NS * lpt;
  const int64_t gid = ((int64_t)blockIdx.x * kAttnNT + threadIdx.x) >> lpt_log2;
  const int64_t t0 = gid * tpg < T ? gid * tpg : T;
  const int64_t t1 = t0 + tpg < T ? t0 + tpg : T;
  float av[NS], ga[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    av[i] = att[lane + lpt * i];
    ga[i] = 0.f;
  }
  [[maybe_unused]] const int64_t E = kDrop ? rowptr[T] : 0;  // the self loops' draws come after the E entries'
  [[maybe_unused]] int head[HL];
  if constexpr (kDrop) {
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) head[hl] = (lane + lpt * hl * SPH) >> c_log2;
  }
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t b = rowptr[t], e = rowptr[t + 1];
    float gv[NS], rv[NS], gr[NS], go[HL], m[HL], inv_s[HL];
#pragma unroll
    for (int hl = 0; hl < HL; ++hl) {
      const int head = (lane + lpt * hl * SPH) >> c_log2;
      m[hl] = row_max[t * H + head];
      inv_s[hl] = 1.f / row_sum[t * H + head];
      go[hl] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int64_t c = lane + lpt * i;
      gv[i] = g[t * D + c];
      rv[i] = load1(xr + t * xr_stride + c);
      gr[i] = 0.f;
      go[i / SPH] += gv[i] * out[t * D + c];
    }
    for (int d = (1 << seg_log2) >> 1; d >= 1; d >>= 1)
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) go[hl] += __shfl_xor(go[hl], d, kWave);
    for (int64_t k = b - 1; k < e; ++k) {  // k == b - 1 stands for the self loop
      const int64_t j = k < b ? t : col[k];
      if (k >= b && j == t) continue;  // set_diag drops existing diagonal entries
      float xv[NS], pe[HL], gh[HL];
#pragma unroll
      for (int i = 0; i < NS; ++i) xv[i] = load1(xl + j * xl_stride + lane + lpt * i);
      [[maybe_unused]] float q[HL];  // kDrop: keep / (1 - p)
      if constexpr (kDrop) {
#pragma unroll
        for (int hl = 0; hl < HL; ++hl)
          q[hl] = attn_keep_head((uint64_t)(k < b ? E + t : k), H, head[hl], drop) ? drop.scale : 0.f;
      }
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) pe[hl] = gh[hl] = 0.f;
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        pe[i / SPH] += av[i] * lrelu(xv[i] + rv[i], slope);
        gh[i / SPH] += gv[i] * xv[i];
      }
      for (int d = (1 << seg_log2) >> 1; d >= 1; d >>= 1)
#pragma unroll
        for (int hl = 0; hl < HL; ++hl) {
          pe[hl] += __shfl_xor(pe[hl], d, kWave);
          gh[hl] += __shfl_xor(gh[hl], d, kWave);
        }
      float a[HL], ge[HL];
#pragma unroll
      for (int hl = 0; hl < HL; ++hl) {
        a[hl] = expf(pe[hl] - m[hl]) * inv_s[hl];
        ge[hl] = a[hl] * ((kDrop ? q[hl] * gh[hl] : gh[hl]) - go[hl]);
        if constexpr (kDrop) a[hl] *= q[hl];  // from here on a is the message's weight q alpha
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const float pre = xv[i] + rv[i];
        const float tt = ge[i / SPH] * av[i] * (pre > 0.f ? 1.f : slope);
        gr[i] += tt;
        ga[i] += ge[i / SPH] * lrelu(pre, slope);
        if (grad_xl) unsafeAtomicAdd(grad_xl + j * D + lane + lpt * i, a[i / SPH] * gv[i] + tt);
      }
    }
    bwd_store_row(grad_xr, t, lane, lpt, gr);
  }
  // grad_att: the groups of a wavefront hold the same columns (lpt < 64), then the wavefronts of the workgroup
  const int wl = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    float v = ga[i];
    for (int d = lpt; d < kWave; d <<= 1) v += __shfl_xor(v, d, kWave);
    red[wave][i][wl] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < lpt) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < kAttnNT / kWave; ++w) s += red[w][i][threadIdx.x];
      unsafeAtomicAdd(grad_att + threadIdx.x + lpt * i, s);
    }
  }
}

}  // namespace spp

using namespace spp;
using namespace spp::gatv2;

// The row checks of both entries, after attn_train.hip.h's shape check and the T == 0 decision, in the order include/spp.h
// documents: strides, NULL buffers, alignment.  Nothing here touches the device.
static spp_status gatv2_check_rows(const spp_gatv2_desc* d, const char* who) {
  const int64_t D = d->heads * d->C, esz = elem_bytes(d->x_elem);
  SPP_REQUIRE(d->x_l_stride_elems >= D && d->x_r_stride_elems >= D && d->x_l_stride_elems % 4 == 0 &&
                  d->x_r_stride_elems % 4 == 0,
              "%s: a row stride is smaller than D or not a multiple of 4 elements", who);
  SPP_REQUIRE(d->rowptr_dev && d->x_l_dev && d->x_r_dev && d->att_dev && d->out_dev && d->row_max_dev && d->row_sum_dev,
              "%s: NULL buffer", who);
  SPP_REQUIRE(aligned_to(d->x_l_dev, 4 * esz) && aligned_to(d->x_r_dev, 4 * esz) && aligned_to(d->att_dev, 16) &&
                  aligned_to(d->out_dev, 16) && aligned_to(d->row_max_dev, 4) && aligned_to(d->row_sum_dev, 4) &&
                  aligned_to(d->rowptr_dev, 8) && aligned_to(d->col_dev, 8),
              "%s: misaligned buffer (rows: 4 elements; att, out: 16 bytes)", who);
  return SPP_OK;
}

// attn_entry checks the _drop entries' AttnDrop (spp.h f3x) right after the shape, before the T == 0 return and the rows
static spp_status gatv2_forward(const spp_gatv2_desc* d, void* stream, const char* who, const AttnDrop& dr) {
  return attn_entry(d, who, dr, [&] { return gatv2_check_rows(d, who); }, [&] {
    dispatch_fwd(d->x_elem, d->heads, d->C, dr.on(), [&](auto tin, auto q, auto c, auto drop, const Shape& sh) {
      using Tin = typename decltype(tin)::type;
      hipLaunchKernelGGL((k_gatv2_fwd<Tin, decltype(q)::value, decltype(c)::value, decltype(drop)::value>),
                         dim3(grid_of(d->num_targets, sh.lpr_log2)), dim3(kAttnNT), 0, as_stream(stream), d->rowptr_dev,
                         d->col_dev, d->num_targets, static_cast<const Tin*>(d->x_l_dev), d->x_l_stride_elems,
                         static_cast<const Tin*>(d->x_r_dev), d->x_r_stride_elems, d->att_dev, d->negative_slope,
                         sh.lpr_log2, sh.seg_log2, sh.g_log2, (int)d->heads, d->out_dev, d->row_max_dev, d->row_sum_dev,
                         dr.args());
    });
  });
}

// grad_att is checked first and zeroed whatever T is: with T == 0 it is the whole answer
static spp_status gatv2_backward(const spp_gatv2_desc* d, void* stream, const char* who, const AttnDrop& dr) {
  hipStream_t st = as_stream(stream);
  auto rows = [&]() -> spp_status {
    SPP_TRY(gatv2_check_rows(d, who));
    SPP_REQUIRE(d->grad_out_dev && d->grad_x_r_dev, "%s: NULL buffer", who);
    SPP_REQUIRE(aligned_to(d->grad_out_dev, 16) && aligned_to(d->grad_x_r_dev, 16) && aligned_to(d->grad_x_l_dev, 16),
                "%s: misaligned buffer (grad_out, grad_x_l, grad_x_r: 16 bytes)", who);
    return SPP_OK;
  };
  auto launch = [&] {
    dispatch_bwd(d->x_elem, d->heads, d->C, dr.on(), [&](auto tin, auto n, auto s, auto drop, const BwdShape& sh) {
      using Tin = typename decltype(tin)::type;
      // every workgroup ends in D atomics onto the same addresses: about 1024 workgroups, whatever T is
      const int64_t T = d->num_targets, gpb = kAttnNT >> sh.lpt_log2;
      const int64_t tpg = std::max<int64_t>(1, ceil_div(T, 1024 * gpb));
      hipLaunchKernelGGL((k_gatv2_bwd<Tin, decltype(n)::value, decltype(s)::value, decltype(drop)::value>),
                         dim3((unsigned)ceil_div(ceil_div(T, tpg), gpb)), dim3(kAttnNT), 0, st, d->rowptr_dev,
                         d->col_dev, T, static_cast<const Tin*>(d->x_l_dev), d->x_l_stride_elems,
                         static_cast<const Tin*>(d->x_r_dev), d->x_r_stride_elems, d->att_dev, d->negative_slope,
                         sh.lpt_log2, sh.seg_log2, sh.c_log2, (int)d->heads, d->out_dev, d->row_max_dev, d->row_sum_dev,
                         d->grad_out_dev, tpg, d->grad_x_l_dev, d->grad_x_r_dev, d->grad_att_dev, dr.args());
    });
  };
  return attn_entry(
      d, who, dr, rows, launch,
      [&]() -> spp_status {
        SPP_REQUIRE(d->grad_att_dev && aligned_to(d->grad_att_dev, 16), "%s: NULL or misaligned grad_att", who);
        return SPP_OK;
      },
      [&]() -> spp_status {
        SPP_HIP_TRY(hipMemsetAsync(d->grad_att_dev, 0, sizeof(float) * (size_t)(d->heads * d->C), st));
        return SPP_OK;
      });
}

SPP_ATTN_ENTRIES(spp_gatv2_forward, spp_gatv2_forward_drop, spp_gatv2_desc, gatv2_forward)
SPP_ATTN_ENTRIES(spp_gatv2_backward, spp_gatv2_backward_drop, spp_gatv2_desc, gatv2_backward)
