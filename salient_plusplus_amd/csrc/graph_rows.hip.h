// What the kernels over rows of the resident graph share (graph_aggregate.hip: sums; graph_gat.hip: attention): the
// targets of a call and its long-row list on the device, the owner lookup of a row-partitioned matrix, and on the host
// the checks of a parts descriptor and of everything the two families' entries refuse alike.
#pragma once

#include "elem_io.hip.h"

#include <algorithm>

namespace spp {
namespace graph_rows {

constexpr int kNT = 256;
constexpr int64_t kWorkspaceHeader = 16;      // the counter (8 bytes) and padding; the list follows
constexpr unsigned kLongGrid = 16384;         // workgroups of the long-row launch (they stride over the list)
constexpr int64_t kGraphChunk = 64;           // C of the sums' contract (graph_aggregate.hip, graph_agg_weighted.hip)

// ---- device: what both families' Args begin and end with ----
// the graph, the targets of the call and the geometry of x and out
struct Targets {
  const int64_t* rowptr;
  const int64_t* col;
  const int64_t* ids;   // NULL: the slab row0 .. row0 + T
  int64_t row0, T;
  int64_t x_stride, x_rows, F;
  int64_t out_stride;
  __device__ __forceinline__ int64_t target(int64_t i) const { return ids ? ids[i] : row0 + i; }
};
// The caller's workspace: a counter the entry zeroes and the OUTPUT indices of the long rows.  The first launch appends
// (one atomic a row; the list's order varies from run to run, the result of a row does not depend on it), the second
// strides over the list.
struct LongRows {
  unsigned long long* counter;
  int64_t* list;
  __device__ __forceinline__ void append(int64_t i) const { list[atomicAdd(counter, 1ull)] = i; }
  __device__ __forceinline__ int64_t count() const { return (int64_t)*counter; }
};

// ---- device: the owner of a global row of a row-partitioned matrix ----
// The matrix as up to kMaxParts row ranges, each in an allocation of its own (a rank's partition, mapped into this
// process): entry p of a table holds the first global row of the p-th NON-EMPTY part and, per matrix, its base moved
// back by that many rows (part_table), so that row g of every part is base + g * stride; the entries behind the last
// part start at INT64_MAX (no row reaches them).  The launch passes the tables by value.  Indexing that argument block
// with a per-lane owner would make the compiler keep a private copy of it in scratch, and walking
// it entry by entry with scalar loads puts two dependent scalar-load waits per entry in front of every row fetch
// (measured: 2.1-2.3 times the time of one matrix).  So thread 0 copies the tables into LDS once per workgroup, with
// compile-time indices, and a lane finds the owner by a branch-free binary search there: four dependent 8-byte LDS
// reads, then one for each base, no loop, and the searches of the four rows in flight overlap.
constexpr int kMaxParts = SPP_GRAPH_AGG_MAX_PARTS;
static_assert(kMaxParts == 16, "part_owner searches exactly 16 entries");
template <int NB>  // NB matrices share the row ranges: one base table each
struct PartTable {
  int64_t first[kMaxParts];
  const void* base[NB][kMaxParts];
};
// The LDS copy itself stays with each row source (PartRows of graph_aggregate.hip and of graph_gat.hip): one loop of
// thread 0 over first[] and its base tables, one barrier.  (With the arrays declared in one shared helper instead, the
// attention's long kernels came out with other LDS offsets and registers; where they are, every kernel is unchanged.)
// the last entry with first <= g (first[0] = 0), for g inside [0, rows); first points into LDS
__device__ __forceinline__ int part_owner(const int64_t* first, int64_t g) {
  int p = g >= first[8] ? 8 : 0;
  p += g >= first[p + 4] ? 4 : 0;
  p += g >= first[p + 2] ? 2 : 0;
  p += g >= first[p + 1] ? 1 : 0;
  return p;
}

// ---- host ----
inline int64_t workspace_bytes(int64_t num_targets) { return kWorkspaceHeader + 8 * std::max<int64_t>(num_targets, 0); }

// the non-empty parts of a parts descriptor in order, with one or two base addresses each
struct Parts {
  int n;
  int64_t first[kMaxParts];
  const void* base[2][kMaxParts];
};

// validates a parts descriptor and compacts it to its non-empty parts; name1 == NULL: one base array
inline spp_status check_parts(const char* who, int32_t num_parts, const int64_t* part_offsets, const void* const* base0,
                              const char* name0, const void* const* base1, const char* name1, Parts* parts) {
  SPP_REQUIRE(num_parts >= 1 && num_parts <= kMaxParts, "%s: num_parts %d outside 1..%d", who, (int)num_parts, kMaxParts);
  SPP_REQUIRE(part_offsets[0] == 0, "%s: part_offsets[0] must be 0, got %lld", who, (long long)part_offsets[0]);
  *parts = Parts{};
  for (int p = 0; p < num_parts; ++p) {
    const long long b = part_offsets[p], e = part_offsets[p + 1];
    SPP_REQUIRE(e >= b, "%s: part_offsets decrease at part %d (%lld after %lld)", who, p, e, b);
    if (e == b) continue;  // an empty part owns no row: its bases may be NULL
    SPP_REQUIRE(base0[p], "%s: part %d holds the rows [%lld, %lld) and its %s is NULL", who, p, b, e, name0);
    SPP_REQUIRE(!name1 || base1[p], "%s: part %d holds the rows [%lld, %lld) and its %s is NULL", who, p, b, e, name1);
    parts->first[parts->n] = b, parts->base[0][parts->n] = base0[p], parts->base[1][parts->n] = name1 ? base1[p] : nullptr;
    ++parts->n;
  }
  return SPP_OK;
}

// The device tables of `parts`: each non-empty part's bases moved back by its first row (never dereferenced below that
// row; integer arithmetic, the address may lie before the allocation), and INT64_MAX as the first row of the entries
// behind the last part (never the owner).  row_bytes[b]: the bytes of a row of matrix b.
template <int NB>
inline PartTable<NB> part_table(const Parts& parts, const int64_t (&row_bytes)[NB]) {
  PartTable<NB> t{};
  for (int p = 0; p < kMaxParts; ++p) t.first[p] = p < parts.n ? parts.first[p] : INT64_MAX;
  for (int b = 0; b < NB; ++b)
    for (int p = 0; p < parts.n; ++p)
      t.base[b][p] = reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(parts.base[b][p]) -
                                                   (uintptr_t)parts.first[p] * (uintptr_t)row_bytes[b]);
  return t;
}

// the descriptor fields both families share
struct Common {
  int32_t x_elem, out_elem;
  const int64_t* rowptr;
  const int64_t* col;
  int64_t x_stride, x_rows, F, row0;
  const int64_t* ids;
  int64_t T;
  void* out;
  int64_t out_stride;
};

// what a launch needs from the checks
struct Launch {
  bool empty;  // T == 0 or F == 0: nothing to enqueue
  bool vec;
  int lpr_log2;
  unsigned grid, long_grid;
  Targets targets;
  LongRows long_rows;
};

// The checks both families' forward() make, in one order.  out_width: the columns of an output row; vec_cols: the
// columns that must be a multiple of 4 for the vector form (F, or the columns of a head); x_bases: the base of x or
// of each non-empty part; others: the entry's further buffers are there.  The vector form moves four columns per
// lane: rows of x that do not allow it (with parts: the rows of any of them) are read one column per lane instead; an
// output that does not is refused (the caller allocates it).  fp8_rows: the entry reads e4m3 rows in place (f3o, the
// _fp8 entries of graph_aggregate.hip: x_elem is SPP_ELEM_FP8_E4M3, an element is a byte); everywhere else they are refused.
// ws_fn, stride_name: the entry's own workspace function and row-stride field, as its messages name them.
inline spp_status check_common(const char* who, const Common& d, int64_t out_width, int64_t vec_cols,
                               const void* const* x_bases, int n_bases, bool others, void* workspace_dev,
                               int64_t workspace_bytes_given, Launch* l, bool fp8_rows = false,
                               const char* ws_fn = "spp_graph_agg_ / spp_graph_gat_workspace_bytes",
                               const char* stride_name = "x_stride_elems") {
  SPP_REQUIRE((fp8_rows || d.x_elem != SPP_ELEM_FP8_E4M3) && d.out_elem != SPP_ELEM_FP8_E4M3,
              "%s: fp8 rows are not read or written here (x_elem %d, out_elem %d; dequantise the table first)", who,
              (int)d.x_elem, (int)d.out_elem);
  SPP_REQUIRE((fp8_rows ? d.x_elem == SPP_ELEM_FP8_E4M3 : elem_ok(d.x_elem)) && f32_bf16_ok(d.out_elem),
              "%s: unknown or unsupported element code (x_elem %d, out_elem %d)", who, (int)d.x_elem, (int)d.out_elem);
  const bool by_ids = d.ids != nullptr, by_slab = d.row0 >= 0;
  SPP_REQUIRE(by_ids != by_slab, "%s: give the targets as a slab (target_row0 >= 0) or as a list (target_ids_dev), %s", who,
              by_ids ? "not both" : "one of them");
  const int64_t T = d.T, F = d.F;
  SPP_REQUIRE(T >= 0 && F >= 0 && d.x_rows >= 0, "%s: negative size (num_targets, F or x_rows)", who);
  SPP_REQUIRE(by_ids || (d.row0 <= d.x_rows && T <= d.x_rows - d.row0),
              "%s: the slab [%lld, %lld) (target_row0, num_targets) leaves the graph's %lld rows", who, (long long)d.row0,
              (long long)(d.row0 + T), (long long)d.x_rows);
  const int64_t out_stride = d.out_stride > 0 ? d.out_stride : out_width;
  SPP_REQUIRE(out_stride >= out_width, "%s: output stride (out_stride_elems) smaller than the output row", who);
  SPP_REQUIRE(workspace_dev && aligned_to(workspace_dev, 16) && workspace_bytes_given >= workspace_bytes(T),
              "%s: needs a 16-byte aligned workspace of %lld bytes (%s(num_targets))", who,
              (long long)workspace_bytes(T), ws_fn);
  *l = Launch{};
  l->empty = T == 0 || F == 0;
  if (l->empty) return SPP_OK;
  bool x_there = true, x_aligned = true;
  for (int p = 0; p < n_bases; ++p)
    x_there = x_there && x_bases[p], x_aligned = x_aligned && aligned_to(x_bases[p], 4 * elem_bytes(d.x_elem));
  SPP_REQUIRE(d.rowptr && d.col && x_there && others && d.out && d.x_rows > 0, "%s: NULL buffer or empty graph", who);
  SPP_REQUIRE(d.x_stride >= F, "%s: row stride (%s) smaller than the row", who, stride_name);
  l->vec = vec_cols % 4 == 0 && d.x_stride % 4 == 0 && x_aligned;
  SPP_REQUIRE(!l->vec || (out_stride % 4 == 0 && aligned_to(d.out, 4 * elem_bytes(d.out_elem))),
              "%s: the vector form (4 columns a lane) needs out_dev aligned to 4 elements (base and stride)", who);
  l->lpr_log2 = lanes_log2(l->vec ? F / 4 : F);
  const int64_t grid = ceil_div(T << l->lpr_log2, kNT);
  SPP_REQUIRE(grid < (1ll << 31), "%s: too many targets for one launch (num_targets %lld)", who, (long long)T);
  l->grid = (unsigned)grid, l->long_grid = (unsigned)std::min<int64_t>(T, kLongGrid);
  l->targets = Targets{d.rowptr, d.col, d.ids, by_ids ? 0 : d.row0, T, d.x_stride, d.x_rows, F, out_stride};
  l->long_rows.counter = static_cast<unsigned long long*>(workspace_dev);
  l->long_rows.list = reinterpret_cast<int64_t*>(static_cast<char*>(workspace_dev) + kWorkspaceHeader);
  return SPP_OK;
}

}  // namespace graph_rows
}  // namespace spp
