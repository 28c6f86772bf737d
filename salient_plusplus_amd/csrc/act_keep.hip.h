// The keep / drop rule of every dropout this library applies (aggregate.hip: k_relu_dropout_*, the activated operand;
// bn_act.hip: the BatchNorm tail; gat.hip, gatv2.hip: the attention dropout), from a counter-based generator: element i of the call with `seed` is kept iff
// hash(seed, i) < (1 - p) * 2^32.  One 64-bit hash serves two elements; the n % 4 elements at the end of an array take
// a hash of their own (the tail of k_relu_dropout_fwd).
#pragma once

#include "elem_io.hip.h"

namespace spp {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
struct ActArgs {
  uint32_t keep_thr;
  float scale;
  uint64_t seed;
  int32_t training;
};

// keep / drop of the four elements 4*i4 .. 4*i4+3 of a dense array
struct Keep4 {
  bool x, y, z, w;
};
__device__ __forceinline__ Keep4 keep4(int64_t i4, const ActArgs& a) {
  const uint64_t r0 = mix64(a.seed + 2ull * (uint64_t)i4 * 0x9E3779B97F4A7C15ull);
  const uint64_t r1 = mix64(a.seed + (2ull * (uint64_t)i4 + 1ull) * 0x9E3779B97F4A7C15ull);
  return {(uint32_t)r0 < a.keep_thr, (uint32_t)(r0 >> 32) < a.keep_thr, (uint32_t)r1 < a.keep_thr,
          (uint32_t)(r1 >> 32) < a.keep_thr};
}
// keep / drop of element i of a dense array of n: the same answer keep4 gives for i < n - n % 4, the tail's hash after
__device__ __forceinline__ bool keep1(int64_t i, int64_t n, const ActArgs& a) {
  if (i >= n - (n & 3)) return (uint32_t)mix64(a.seed + (uint64_t)i * 0xD1B54A32D192ED03ull) < a.keep_thr;
  const uint64_t r = mix64(a.seed + (uint64_t)(i >> 1) * 0x9E3779B97F4A7C15ull);
  return (uint32_t)(i & 1 ? r >> 32 : r) < a.keep_thr;
}

// the activation of the four elements 4*i4 .. 4*i4+3 of a dense array, exactly as k_relu_dropout_fwd computes it
__device__ __forceinline__ f4 relu_dropout4(f4 v, int64_t i4, const ActArgs& a) {
  if (!a.training) return {fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
  const uint64_t r0 = mix64(a.seed + 2ull * (uint64_t)i4 * 0x9E3779B97F4A7C15ull);
  const uint64_t r1 = mix64(a.seed + (2ull * (uint64_t)i4 + 1ull) * 0x9E3779B97F4A7C15ull);
  f4 o;
  o.x = (v.x > 0.f && (uint32_t)r0 < a.keep_thr) ? v.x * a.scale : 0.f;
  o.y = (v.y > 0.f && (uint32_t)(r0 >> 32) < a.keep_thr) ? v.y * a.scale : 0.f;
  o.z = (v.z > 0.f && (uint32_t)r1 < a.keep_thr) ? v.z * a.scale : 0.f;
  o.w = (v.w > 0.f && (uint32_t)(r1 >> 32) < a.keep_thr) ? v.w * a.scale : 0.f;
  return o;
}

// Attention dropout (GATConv's dropout=, spp.h f3t): keep / drop of the H heads of softmax entry `entry` -- CSR entry k
// is entry k, target t's self loop is entry E + t -- draw index i = entry * H + h, the low (i even) or high (i odd) half
// of mix64(seed + (i >> 1) * 0x9E3779B97F4A7C15): one hash serves two heads, and at H = 1 two neighbouring entries.
template <int H>
__device__ __forceinline__ void attn_keep_heads(uint64_t entry, const ActArgs& a, bool (&keep)[H]) {
  if constexpr (H == 1) {
    const uint64_t r = mix64(a.seed + (entry >> 1) * 0x9E3779B97F4A7C15ull);
    keep[0] = (uint32_t)(entry & 1 ? r >> 32 : r) < a.keep_thr;
  } else {
    const uint64_t base = a.seed + entry * (uint64_t)(H / 2) * 0x9E3779B97F4A7C15ull;  // (i >> 1) = entry * H/2 + h/2
#pragma unroll
    for (int q = 0; q < H / 2; ++q) {
      const uint64_t r = mix64(base + (uint64_t)q * 0x9E3779B97F4A7C15ull);
      keep[2 * q] = (uint32_t)r < a.keep_thr;
      keep[2 * q + 1] = (uint32_t)(r >> 32) < a.keep_thr;
    }
  }
}

// The same draw for ONE head h of H (spp.h f3x): for kernels whose lanes serve only some of the heads (gatv2.hip), so a
// lane hashes for the heads it holds and no others.  attn_keep_heads<H>(entry, a, keep)[h] for every H, entry and h.
__device__ __forceinline__ bool attn_keep_head(uint64_t entry, int H, int h, const ActArgs& a) {
  const uint64_t i = entry * (uint64_t)H + (uint64_t)h;
  const uint64_t r = mix64(a.seed + (i >> 1) * 0x9E3779B97F4A7C15ull);
  return (uint32_t)(i & 1 ? r >> 32 : r) < a.keep_thr;
}

static inline ActArgs act_args(float p, int32_t training, uint64_t seed) {
  const double keep = 1.0 - (double)p;
  ActArgs a{};
  a.keep_thr = keep >= 1.0 ? 0xffffffffu : (uint32_t)(keep * 4294967296.0);
  a.scale = (float)(1.0 / keep);
  a.seed = seed;
  a.training = training ? 1 : 0;
  return a;
}

// The attention dropout arguments of a _drop entry (spp.h f3t, f3x, f4a: (p, training, seed) after `stream`), host side;
// the entries without dropout pass AttnDrop{}.  training = 0 or p = 0 runs the kDrop = false kernels, which never read
// the block (it then carries p = 0).
struct AttnDrop {
  bool given = false;
  float p = 0.f;
  int32_t training = 0;
  uint64_t seed = 0;
  bool on() const { return given && training && p > 0.f; }
  ActArgs args() const { return act_args(on() ? p : 0.f, training, seed); }
};
// every entry runs this right after its shape checks, before its sizes and buffers, in eval mode too
static inline spp_status attn_drop_check(const AttnDrop& dr, const char* who) {
  SPP_REQUIRE(!dr.given || (dr.p >= 0.f && dr.p < 1.f), "%s: attention dropout needs 0 <= p < 1", who);
  return SPP_OK;
}
// fn(std::bool_constant<kDrop>{})
template <class Fn>
static void with_drop(bool on, Fn&& fn) {
  if (on) fn(std::true_type{}); else fn(std::false_type{});
}

}  // namespace spp
