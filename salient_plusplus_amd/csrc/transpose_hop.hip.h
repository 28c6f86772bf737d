// The transposed hop (sources -> targets) that the gather backwards share (aggregate.hip: the operand's and the sum's;
// gat.hip: GAT's; aggregate_weighted.hip: the weighted sum's): its kernels, its workspace layout and the count / scan /
// fill that builds it.  Moved out of aggregate.hip unchanged, but for the kernels' `static`: each of the three
// translation units holds its own copy of them (and of hipcub's scan).
#pragma once

#include "spp_internal.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace spp {

constexpr int kAggNT = 256;

// ---- backward of the fused operand by GATHER over the transposed hop ----------------------------
// 42 M fp32 atomics (163 k edges x 256 columns) run at the chip's atomic rate (~325 G/s: 140 us); the
// transposed adjacency (sources -> targets) costs three small integer passes per step and turns the
// backward into the same gather-reduce as the forward.
static __global__ __launch_bounds__(kAggNT) void k_tr_count(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                     int64_t T, int32_t* __restrict__ cnt, float* __restrict__ inv) {
  const int64_t t = (int64_t)blockIdx.x * kAggNT + threadIdx.x;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  inv[t] = 1.0f / (float)(e > b ? e - b : 1);
  for (int64_t k = b; k < e; ++k) atomicAdd(&cnt[col[k]], 1);
}

// tcol[pos] = t and tedge[pos] = k, the entry's CSR position, for every entry (t, s) of the hop, pos in source s's
// segment -- in the order the atomics on the source's cursor arrive, which changes from run to run as soon as the
// targets fill more than one wavefront: k_tr_order puts every segment into one order
static __global__ __launch_bounds__(kAggNT) void k_tr_fill(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                    int64_t T, const int32_t* __restrict__ start,
                                                    int32_t* __restrict__ cursor, int32_t* __restrict__ tcol,
                                                    int32_t* __restrict__ tedge) {
  const int64_t t = (int64_t)blockIdx.x * kAggNT + threadIdx.x;
  if (t >= T) return;
  const int64_t b = rowptr[t], e = rowptr[t + 1];
  for (int64_t k = b; k < e; ++k) {
    const int64_t s = col[k];
    const int32_t pos = start[s] + atomicAdd(&cursor[s], 1);
    tcol[pos] = (int32_t)t;
    tedge[pos] = (int32_t)k;
  }
}

// Every segment of the filled hop in ascending CSR position (so in ascending target): one thread per entry; the entry ids
// of a segment are distinct, so an entry's place is the number of smaller ids in its segment.  A gather over a segment
// then adds its terms in the same order in every run.  (Work: the sum of the squared in-degrees, read from one cached
// segment per wavefront group; the in-degrees of a sampled hop are small.)  tedge == NULL: only tcol is wanted.
static __global__ __launch_bounds__(kAggNT) void k_tr_order(const int64_t* __restrict__ col, const int32_t* __restrict__ start,
                                                     const int32_t* __restrict__ tcol_in,
                                                     const int32_t* __restrict__ tedge_in, int64_t E, int64_t S,
                                                     int32_t* __restrict__ tcol, int32_t* __restrict__ tedge) {
  const int64_t p = (int64_t)blockIdx.x * kAggNT + threadIdx.x;
  if (p >= E || p >= start[S]) return;  // start[S]: the entries rowptr holds, all that k_tr_fill wrote
  const int32_t k = tedge_in[p];
  const int64_t s = col[k];
  const int32_t b = start[s], e = start[s + 1];
  int32_t rank = 0;
  for (int32_t q = b; q < e; ++q) rank += tedge_in[q] < k ? 1 : 0;
  tcol[b + rank] = tcol_in[p];
  if (tedge) tedge[b + rank] = k;
}

static int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// The workspace of transpose_hop: cnt/cursor [S+1] | start [S+1] | tcol [E] | tedge [E] (edge_ids) | inv [T] |
// the filled, unordered tcol [E] and tedge [E] | scan temporaries   (each 16-byte aligned)
static int64_t transpose_hop_bytes(int64_t T, int64_t S, int64_t E, bool edge_ids) {
  size_t scan_tmp = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (const int32_t*)nullptr, (int32_t*)nullptr, (int)(S + 1));
  return align16(4 * (S + 1)) * 2 + align16(4 * E) * (edge_ids ? 4 : 3) + align16(4 * T) + align16((int64_t)scan_tmp) + 64;
}

struct TransposedHop {
  const int32_t *start, *tcol, *tedge;
  const float* inv;
};

// The transposed hop (sources -> targets) in a transpose_hop_bytes workspace: source s's targets are
// tcol[start[s] .. start[s+1]), with edge_ids tedge[] holds the CSR entry of each, inv[t] = 1 / max(deg t, 1).
// Each segment is in ascending CSR position, the same in every run.  Count, scan, fill, order; the callers have checked
// the sizes.
static spp_status transpose_hop(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                int64_t num_sources, int64_t num_edges, bool edge_ids, void* workspace_dev,
                                int64_t workspace_bytes, hipStream_t st, TransposedHop* hop) {
  char* w = static_cast<char*>(workspace_dev);
  auto take = [&](int64_t bytes) { int32_t* p = reinterpret_cast<int32_t*>(w); w += align16(bytes); return p; };
  int32_t* cnt = take(4 * (num_sources + 1));
  int32_t* start = take(4 * (num_sources + 1));
  int32_t* tcol = take(4 * num_edges);
  int32_t* tedge = edge_ids ? take(4 * num_edges) : nullptr;
  float* inv = reinterpret_cast<float*>(take(4 * num_targets));
  int32_t* tcol_filled = take(4 * num_edges);
  int32_t* tedge_filled = take(4 * num_edges);
  size_t scan_tmp = (size_t)(workspace_bytes - (w - static_cast<char*>(workspace_dev)));
  SPP_HIP_TRY(hipMemsetAsync(cnt, 0, 4 * (size_t)(num_sources + 1), st));
  const unsigned gt = (unsigned)std::max<int64_t>(1, ceil_div(num_targets, kAggNT));
  if (num_targets > 0)
    hipLaunchKernelGGL(k_tr_count, dim3(gt), dim3(kAggNT), 0, st, rowptr_dev, col_dev, num_targets, cnt, inv);
  SPP_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(w, scan_tmp, cnt, start, (int)(num_sources + 1), st));
  SPP_HIP_TRY(hipMemsetAsync(cnt, 0, 4 * (size_t)(num_sources + 1), st));
  if (num_targets > 0 && num_edges > 0) {
    hipLaunchKernelGGL(k_tr_fill, dim3(gt), dim3(kAggNT), 0, st, rowptr_dev, col_dev, num_targets, start, cnt,
                       tcol_filled, tedge_filled);
    hipLaunchKernelGGL(k_tr_order, dim3((unsigned)ceil_div(num_edges, kAggNT)), dim3(kAggNT), 0, st, col_dev, start,
                       tcol_filled, tedge_filled, num_edges, num_sources, tcol, tedge);
  }
  *hop = {start, tcol, tedge, inv};
  return SPP_OK;
}

}  // namespace spp
