// f3m: the tail every model's exact inference shares -- the class a row of logits predicts and its negative
// log-likelihood -- as ONE pass over the GEMM tile that holds the logits, so that no [rows, classes] matrix of
// log-probabilities is ever written (reference: the test loop of driver/main.py, `out.argmax(dim=-1)` and
// `F.nll_loss(out, y)` on log_softmax'ed logits):
//     pred[i] = argmax_c z[i,c]                          torch's rules: smallest index on ties, the first NaN wins
//     m       = max_c z[i,c]
//     nll[i]  = log(sum_c exp(z[i,c] - m)) - (z[i,y] - m)            0.0f without a label in [0, C)
// (include/spp.h, spp_classify_rows, states the contract.)
//
// Shape (resinc_epilogue.hip's): a row is cut into PIECES of kW columns (16 bytes: 4 fp32 or 8 bf16); lpr lanes (a power
// of two, at most 64: the first that covers the row's pieces) own one row, lane l the pieces l, l + lpr, ... -- a row of
// more than lpr pieces is walked in rounds.  A workgroup's 256 / lpr lane groups take kUnroll rows each.  Which lane owns
// which column, the order in which a lane meets its columns and the xor-shuffle trees over the group's lanes follow from
// (C, dtype) alone, and every fp32 operation is a named intrinsic (no contraction): a row's two results are the same
// bits wherever the row stands in the call and however it is loaded.  The load forms differ in nothing else: V columns
// per load instruction, the largest power of two <= kW that the base address, the row stride and C are multiples of
// (V = kW: 16-byte loads; V = 1: one element each), so that a load lies inside the row or outside it as a whole and
// no load needs a branch: one outside is redirected to the row's first columns and its values are never used.
// One round (C <= lpr * kW): a row's logits are read once into registers and both reductions run from there.  More
// rounds: the maximum is taken in a first walk and the sum in a second one, which finds the row (a few KB) in the cache.
// The four rows of a lane group go through every step together -- their loads are issued back to back, the label's
// dependent loads (id, label, the label's logit) one kind at a time, and the four xor trees step in one loop -- so a
// wave has four independent chains in flight through the shuffles.
// No atomics, no LDS, no workspace, every offset 64-bit.
#include "elem_io.hip.h"

#include <limits>

namespace spp {
namespace classify {

constexpr int kNT = 256;
constexpr int kUnroll = 4;            // rows per lane group
constexpr int kNoIndex = 0x7fffffff;  // loses every tie: no column has it (C < 2^31)

template <typename T> constexpr int piece_width() { return 16 / (int)sizeof(T); }

// V columns from p (aligned to V elements) into o.v[k ..], converted to fp32 exactly
template <int V, int W>
__device__ __forceinline__ void load_cols(const float* p, PieceN<W>& o, int k) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    o.v[k] = q.x, o.v[k + 1] = q.y, o.v[k + 2] = q.z, o.v[k + 3] = q.w;
  } else if constexpr (V == 2) {
    const float2 q = *reinterpret_cast<const float2*>(p);
    o.v[k] = q.x, o.v[k + 1] = q.y;
  } else {
    o.v[k] = *p;
  }
}
template <int V, int W>
__device__ __forceinline__ void load_cols(const bf16* p, PieceN<W>& o, int k) {
  if constexpr (V == 8) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    o.v[k] = bf16_lo(q.x), o.v[k + 1] = bf16_hi(q.x), o.v[k + 2] = bf16_lo(q.y), o.v[k + 3] = bf16_hi(q.y);
    o.v[k + 4] = bf16_lo(q.z), o.v[k + 5] = bf16_hi(q.z), o.v[k + 6] = bf16_lo(q.w), o.v[k + 7] = bf16_hi(q.w);
  } else if constexpr (V == 4) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    o.v[k] = bf16_lo(q.x), o.v[k + 1] = bf16_hi(q.x), o.v[k + 2] = bf16_lo(q.y), o.v[k + 3] = bf16_hi(q.y);
  } else if constexpr (V == 2) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
    o.v[k] = bf16_lo(q), o.v[k + 1] = bf16_hi(q);
  } else {
    o.v[k] = bf16_lo(*reinterpret_cast<const uint16_t*>(p));
  }
}

// the first `valid` (0 .. W, a multiple of V: V divides C) columns of the piece at column c0 of `row`.  No branch: a
// chunk of V columns past them is loaded from the row's first V columns instead (C >= V) and its slots are never used.
template <typename T, int V>
__device__ __forceinline__ PieceN<piece_width<T>()> load_piece(const T* row, int64_t c0, int valid) {
  constexpr int W = piece_width<T>();
  PieceN<W> o;
#pragma unroll
  for (int k = 0; k < W; k += V) load_cols<V, W>(row + (k + V <= valid ? c0 + k : 0), o, k);
  return o;
}

// how many of the W columns from c0 on the row has (0 when the piece lies past its end)
template <int W>
__device__ __forceinline__ int valid_cols(int64_t c0, int64_t C) {
  const int64_t left = C - c0;
  return left >= W ? W : left > 0 ? (int)left : 0;
}

// ---- the contract's arithmetic; the three forms of a kernel share every line of it ---------------------------------
struct Best {
  float v;
  int i;
};

// torch's order: a NaN is above everything, and of two equals (two NaNs included) the smaller index wins.  A total
// order on (value, index) pairs, so the maximum does not depend on the order of the comparisons: exact by construction.
__device__ __forceinline__ bool beats(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  const bool above = (an & !bn) | (av > bv), same = (an & bn) | (av == bv);  // (a comparison with a NaN is false)
  return above | (same & (ai < bi));
}
// A lane meets its columns in ascending order, so inside a lane the index decides nothing: a later column wins only if
// it is strictly above, or the first NaN.  !(v <= b.v) is "above or NaN"; a column past the row's end counts as -inf,
// which that never takes.  (The lane starts at (-inf, its first column): a row of -inf predicts its first column.)
template <int W>
__device__ __forceinline__ void max_piece(Best& b, const PieceN<W>& p, int c0, int valid) {
  const float ninf = -std::numeric_limits<float>::infinity();
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const float v = k < valid ? p.v[k] : ninf;
    const bool w = !(v <= b.v) && b.v == b.v;
    b.v = w ? v : b.v, b.i = w ? c0 + k : b.i;
  }
}
// the group's maximum in every lane; the kUnroll rows' trees step together, so their shuffles overlap
__device__ __forceinline__ void max_groups(Best (&b)[kUnroll], int lpr) {
  for (int off = 1; off < lpr; off <<= 1) {
    float ov[kUnroll];
    int oi[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) ov[u] = __shfl_xor(b[u].v, off), oi[u] = __shfl_xor(b[u].i, off);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const bool w = beats(ov[u], oi[u], b[u].v, b[u].i);
      b[u].v = w ? ov[u] : b[u].v, b[u].i = w ? oi[u] : b[u].i;
    }
  }
}

// exp(z - m): one subtraction, one product with log2(e), the hardware's 2^x
__device__ __forceinline__ float exp_term(float z, float m) {
  return __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(z, m), 1.44269504088896340736f));
}
template <int W>
__device__ __forceinline__ void sum_piece(float& s, const PieceN<W>& p, float m, int valid) {
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const float t = __fadd_rn(s, exp_term(p.v[k], m));
    s = k < valid ? t : s;
  }
}
__device__ __forceinline__ void sum_groups(float (&s)[kUnroll], int lpr) {
  for (int off = 1; off < lpr; off <<= 1) {
    float o[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) o[u] = __shfl_xor(s[u], off);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) s[u] = __fadd_rn(s[u], o[u]);  // (a + b == b + a: every lane agrees)
  }
}
__device__ __forceinline__ float nll_of(float s, float zy, float m, bool has) {
  return has ? __fsub_rn(logf(s), __fsub_rn(zy, m)) : 0.f;
}

template <typename T>
__device__ __forceinline__ float load_one(const T* p) {
  PieceN<1> o;
  load_cols<1, 1>(p, o, 0);
  return o.v[0];
}

struct Args {
  const int64_t* y;    // NULL: no labels
  const int64_t* ids;  // NULL: the slab y_row0 .. y_row0 + n
  int64_t row0, y_rows;
  int64_t n, C, z_stride;
  int64_t* pred;  // NULL: not wanted
  float* nll;     // NULL: not wanted
  int lpr_log2;
};

// the labels of the rows i[] as columns of z, or -1: an id outside [0, y_rows) and a label outside [0, C) are "none".
// The loads of a kind are issued together: the ids of a list under one scalar branch, then the labels.
__device__ __forceinline__ void labels_of(const Args& a, const int64_t (&i)[kUnroll], int64_t (&yc)[kUnroll]) {
  int64_t r[kUnroll];
  if (a.ids) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) r[u] = a.ids[i[u]];
  } else {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) r[u] = a.row0 + i[u];
  }
  bool inside[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) inside[u] = (uint64_t)r[u] < (uint64_t)a.y_rows;
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) yc[u] = a.y[inside[u] ? r[u] : 0];  // (y_rows >= 1: the entry checked)
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) yc[u] = (inside[u] & ((uint64_t)yc[u] < (uint64_t)a.C)) ? yc[u] : -1;
}

template <typename T, int V, bool kOneRound>
__global__ __launch_bounds__(kNT) void k_classify_rows(const T* __restrict__ z, Args a) {
  constexpr int W = piece_width<T>();
  const int lpr = 1 << a.lpr_log2, gpb = kNT >> a.lpr_log2;
  const int g = threadIdx.x >> a.lpr_log2, l = threadIdx.x & (lpr - 1);
  const int64_t base = (int64_t)blockIdx.x * gpb * kUnroll;
  const int64_t C = a.C, pieces = (C + W - 1) / W;
  const float ninf = -std::numeric_limits<float>::infinity();
  int64_t i[kUnroll];
  bool ok[kUnroll];
  const T* row[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int64_t iu = base + (int64_t)u * gpb + g;
    ok[u] = iu < a.n;
    i[u] = ok[u] ? iu : a.n - 1;  // (clamped: loaded, never stored; every lane stays in the shuffles)
    row[u] = z + i[u] * a.z_stride;
  }
  // one round: the rows' pieces, loaded once and kept; issued ahead of the labels' dependent loads
  const int c0 = l * W, valid = valid_cols<W>(c0, C);
  PieceN<W> p[kUnroll];
  if constexpr (kOneRound) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) p[u] = load_piece<T, V>(row[u], c0, valid);
  }
  int64_t yc[kUnroll];
  float zy[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) yc[u] = -1, zy[u] = 0.f;
  if (a.nll) {  // (a kernel argument: one scalar branch)
    if (a.y) labels_of(a, i, yc);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) zy[u] = load_one(row[u] + (yc[u] >= 0 ? yc[u] : 0));
  }
  Best b[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) b[u] = Best{ninf, (int64_t)c0 < C ? c0 : kNoIndex};  // (no column: wins no tie)
  if constexpr (kOneRound) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) max_piece<W>(b[u], p[u], c0, valid);
  } else {
    for (int64_t p0 = 0; p0 < pieces; p0 += lpr) {  // (workgroup-uniform bounds; the four rows' pieces in flight)
      const int64_t c = (p0 + l) * W;
      const int v = valid_cols<W>(c, C);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) p[u] = load_piece<T, V>(row[u], c, v);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) max_piece<W>(b[u], p[u], (int)c, v);  // (c past 2^31: v is 0, c unused)
    }
  }
  max_groups(b, lpr);
  if (a.pred && l == 0) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (ok[u]) a.pred[i[u]] = b[u].i;
  }
  if (!a.nll) return;
  float s[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) s[u] = 0.f;
  if constexpr (kOneRound) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) sum_piece<W>(s[u], p[u], b[u].v, valid);
  } else {
    for (int64_t p0 = 0; p0 < pieces; p0 += lpr) {  // (the second walk: the rows are in the cache)
      const int64_t c = (p0 + l) * W;
      const int v = valid_cols<W>(c, C);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) p[u] = load_piece<T, V>(row[u], c, v);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) sum_piece<W>(s[u], p[u], b[u].v, v);
    }
  }
  sum_groups(s, lpr);
  if (l == 0) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (ok[u]) a.nll[i[u]] = nll_of(s[u], zy[u], b[u].v, yc[u] >= 0);
  }
}

}  // namespace classify
}  // namespace spp

using namespace spp;
using namespace spp::classify;

extern "C" spp_status spp_classify_rows(const spp_classify_desc* desc, void* stream) {
  const char* who = "spp_classify_rows";
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_classify_desc& d = *desc;
  SPP_REQUIRE(d.z_dev, "%s: NULL buffer (z_dev)", who);
  SPP_REQUIRE(d.pred_dev || d.nll_dev, "%s: nothing to write (pred_dev and nll_dev are both NULL)", who);
  SPP_REQUIRE(d.z_elem == SPP_ELEM_F32 || d.z_elem == SPP_ELEM_BF16, "%s: unknown or unsupported element code (z_elem %d)",
              who, (int)d.z_elem);
  const int64_t n = d.n, C = d.C;
  SPP_REQUIRE(C >= 1 && C < (1ll << 31), "%s: C = %lld must be in [1, 2^31)", who, (long long)C);
  SPP_REQUIRE(n >= 0, "%s: negative n (%lld)", who, (long long)n);
  SPP_REQUIRE(d.z_stride_elems >= 0, "%s: negative row stride (z %lld)", who, (long long)d.z_stride_elems);
  const int64_t z_stride = d.z_stride_elems ? d.z_stride_elems : C;
  SPP_REQUIRE(z_stride >= C, "%s: a row stride smaller than the row (C = %lld)", who, (long long)C);
  const bool lab = d.y_dev != nullptr, by_ids = d.row_ids_dev != nullptr, by_slab = d.y_row0 >= 0;
  SPP_REQUIRE(!(by_ids && by_slab), "%s: address the labels as a slab (y_row0 >= 0) or as a list (row_ids_dev), not both", who);
  SPP_REQUIRE(!lab || by_ids || by_slab, "%s: labels need their rows: a slab (y_row0 >= 0) or a list (row_ids_dev)", who);
  SPP_REQUIRE(!lab || d.y_rows >= 0, "%s: negative y_rows (%lld)", who, (long long)d.y_rows);
  if (n == 0) return SPP_OK;
  const bool use_y = lab && d.y_rows >= 1;  // (labels of no rows: every row is unlabelled)
  const int esize = (int)elem_bytes(d.z_elem), W = 16 / esize;
  const int64_t pieces = ceil_div(C, (int64_t)W);
  const int lpr_log2 = lanes_log2(pieces);
  const bool one_round = pieces <= (1ll << lpr_log2);
  int V = W;  // columns per load: what the base, the stride and the row are multiples of
  while (V > 1 && (!aligned_to(d.z_dev, V * esize) || z_stride % V != 0 || C % V != 0))
    V >>= 1;
  const int64_t grid = ceil_div(n, (int64_t)(kNT >> lpr_log2) * kUnroll);
  SPP_REQUIRE(grid < (1ll << 31), "%s: too many rows for one launch (n %lld)", who, (long long)n);
  Args a{};
  a.y = use_y ? d.y_dev : nullptr, a.ids = by_ids ? d.row_ids_dev : nullptr, a.row0 = by_slab ? d.y_row0 : 0;
  a.y_rows = use_y ? d.y_rows : 0, a.n = n, a.C = C, a.z_stride = z_stride, a.pred = d.pred_dev, a.nll = d.nll_dev;
  a.lpr_log2 = lpr_log2;
  hipStream_t st = as_stream(stream);
  auto launch = [&](auto t, auto v) {
    using T = typename decltype(t)::type;
    constexpr int Vc = decltype(v)::value;
    if constexpr (Vc <= piece_width<T>()) {
      if (one_round)
        hipLaunchKernelGGL((k_classify_rows<T, Vc, true>), dim3((unsigned)grid), dim3(kNT), 0, st,
                           static_cast<const T*>(d.z_dev), a);
      else
        hipLaunchKernelGGL((k_classify_rows<T, Vc, false>), dim3((unsigned)grid), dim3(kNT), 0, st,
                           static_cast<const T*>(d.z_dev), a);
    }
  };
  auto by_v = [&](auto t) {
    switch (V) {
      case 8: launch(t, std::integral_constant<int, 8>{}); break;
      case 4: launch(t, std::integral_constant<int, 4>{}); break;
      case 2: launch(t, std::integral_constant<int, 2>{}); break;
      default: launch(t, std::integral_constant<int, 1>{}); break;
    }
  };
  d.z_elem == SPP_ELEM_BF16 ? by_v(Type<bf16>{}) : by_v(Type<float>{});
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}
