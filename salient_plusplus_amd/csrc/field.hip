// f3n: the receptive field of a few nodes as a compact, relabelled graph -- the two kernels that touch the resident
// graph's rows when exact inference scores `nodes` over the nodes within L-1 hops of them only (inference.py,
// ReceptiveFields).  The field's nodes carry slots (depth by depth, ascending id within a depth; the numbering is made
// between the launches, by a compaction of the flags, and no atomic decides it):
//   spp_field_mark   flag[j] = 1 for every entry j of a frontier node's row that has no slot yet.  Plain byte stores:
//                    every writer of a flag stores the same value, so the result does not depend on who wins.
//   spp_field_rows   fcol[frowptr[i] + k] = slot[col[rowptr[ids[i]] + k]]: the node's whole row in CSR order, relabelled
//                    (multi-edges and self-loops stay, the degree is unchanged).
// Rows are as uneven as the graph's, so both take graph_aggregate.hip's two-launch shape: kLanes lanes finish every row
// of at most kFieldChunk entries, the lanes of a longer row append its index to the LongRows list in the caller's
// workspace (graph_rows.hip.h), and a second launch gives each listed row a workgroup.  Every offset is 64-bit.
#include "graph_rows.hip.h"

namespace spp {
namespace field {

using namespace graph_rows;

constexpr int64_t kFieldChunk = 64;  // the cut: a longer row is a workgroup's
constexpr int kLanesLog2 = 3;        // lanes that share a short row (8 consecutive entries of col per step: one 64-byte line)
constexpr int kLanes = 1 << kLanesLog2;

struct Args {
  const int64_t* rowptr;
  const int64_t* col;
  int64_t N;
  const int64_t* ids;  // the frontier (mark) or the field's rows by slot (rows)
  int64_t n;
  const int32_t* slot;
  uint8_t* flag;            // mark
  const int64_t* frowptr;   // rows
  int64_t* fcol;            // rows
  int64_t fcol_len;         // rows
  LongRows long_rows;
};

// entries [b, e) of col, one per lane of a group of `lanes` with stride `lanes`
struct Mark {
  static __device__ __forceinline__ int64_t room(const Args&, int64_t, int64_t deg) { return deg; }
  static __device__ __forceinline__ void entries(const Args& a, int64_t, int64_t b, int64_t e, int lane, int lanes) {
    for (int64_t k = b + lane; k < e; k += lanes) {
      const int64_t j = a.col[k];
      if ((uint64_t)j < (uint64_t)a.N && a.slot[j] < 0) a.flag[j] = 1;
    }
  }
};
// A row of the field is the node's own: frowptr is the prefix sum of the same degrees.  One that disagrees is the
// caller's error; the copy then stays inside [frowptr[i], frowptr[i + 1]) and inside fcol.
struct Rows {
  static __device__ __forceinline__ int64_t room(const Args& a, int64_t i, int64_t deg) {
    const int64_t o = a.frowptr[i], len = a.frowptr[i + 1] - o;
    return (o < 0 || o > a.fcol_len) ? 0 : std::min<int64_t>(std::min<int64_t>(deg, len), a.fcol_len - o);
  }
  static __device__ __forceinline__ void entries(const Args& a, int64_t i, int64_t b, int64_t e, int lane, int lanes) {
    const int64_t o = a.frowptr[i];
    for (int64_t k = b + lane; k < e; k += lanes) {
      const int64_t j = a.col[k];
      a.fcol[o + (k - b)] = (uint64_t)j < (uint64_t)a.N ? (int64_t)a.slot[j] : -1;  // (-1: not in the field)
    }
  }
};

// the row of ids[i]: its first entry and its length (0 for an id outside the graph: an empty row, no fault)
template <typename Op>
__device__ __forceinline__ int64_t row_of(const Args& a, int64_t i, int64_t* b) {
  const int64_t t = a.ids[i];
  const bool in_graph = (uint64_t)t < (uint64_t)a.N;
  *b = in_graph ? a.rowptr[t] : 0;
  return in_graph ? std::max<int64_t>(Op::room(a, i, a.rowptr[t + 1] - *b), 0) : 0;
}

template <typename Op>
__global__ __launch_bounds__(kNT) void k_field_short(Args a) {
  const int lane = threadIdx.x & (kLanes - 1);
  const int64_t i = ((int64_t)blockIdx.x * kNT + threadIdx.x) >> kLanesLog2;
  if (i >= a.n) return;
  int64_t b;
  const int64_t deg = row_of<Op>(a, i, &b);
  if (deg > kFieldChunk) {  // a long row: k_field_long's
    if (lane == 0) a.long_rows.append(i);
    return;
  }
  Op::entries(a, i, b, b + deg, lane, kLanes);
}

template <typename Op>
__global__ __launch_bounds__(kNT) void k_field_long(Args a) {
  const int64_t n = a.long_rows.count();
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t i = a.long_rows.list[r];
    int64_t b;
    const int64_t deg = row_of<Op>(a, i, &b);
    Op::entries(a, i, b, b + deg, threadIdx.x, kNT);
  }
}

}  // namespace field
}  // namespace spp

using namespace spp;
using namespace spp::field;

extern "C" int64_t spp_field_chunk(void) { return kFieldChunk; }

extern "C" int64_t spp_field_workspace_bytes(int64_t num_ids) { return workspace_bytes(num_ids); }

namespace {

// what both entries check and launch; rows: spp_field_rows
template <typename Op>
spp_status run(const char* who, const spp_field_desc* desc, bool rows, void* workspace_dev, int64_t workspace_bytes_given,
               void* stream) {
  SPP_REQUIRE(desc, "%s: NULL descriptor", who);
  const spp_field_desc& d = *desc;
  SPP_REQUIRE(d.num_nodes >= 0 && d.num_ids >= 0 && d.fcol_len >= 0, "%s: negative size (num_nodes, num_ids or fcol_len)",
              who);
  SPP_REQUIRE(workspace_dev && aligned_to(workspace_dev, 16) && workspace_bytes_given >= workspace_bytes(d.num_ids),
              "%s: needs a 16-byte aligned workspace of %lld bytes (spp_field_workspace_bytes(num_ids))", who,
              (long long)workspace_bytes(d.num_ids));
  if (d.num_ids == 0) return SPP_OK;
  SPP_REQUIRE(d.rowptr_dev && d.col_dev && d.ids_dev && d.slot_dev && d.num_nodes > 0, "%s: NULL buffer or empty graph", who);
  if (rows)
    SPP_REQUIRE(d.frowptr_dev && (d.fcol_dev || d.fcol_len == 0), "%s: NULL buffer (frowptr_dev or fcol_dev)", who);
  else
    SPP_REQUIRE(d.flag_dev, "%s: NULL buffer (flag_dev)", who);
  const int64_t grid = ceil_div(d.num_ids << kLanesLog2, kNT);
  SPP_REQUIRE(grid < (1ll << 31), "%s: too many rows for one launch (num_ids %lld)", who, (long long)d.num_ids);
  Args a{d.rowptr_dev, d.col_dev, d.num_nodes, d.ids_dev, d.num_ids, d.slot_dev, d.flag_dev, d.frowptr_dev, d.fcol_dev,
         d.fcol_len, LongRows{}};
  a.long_rows.counter = static_cast<unsigned long long*>(workspace_dev);
  a.long_rows.list = reinterpret_cast<int64_t*>(static_cast<char*>(workspace_dev) + kWorkspaceHeader);
  hipStream_t st = as_stream(stream);
  SPP_HIP_TRY(hipMemsetAsync(workspace_dev, 0, kWorkspaceHeader, st));
  hipLaunchKernelGGL((k_field_short<Op>), dim3((unsigned)grid), dim3(kNT), 0, st, a);
  hipLaunchKernelGGL((k_field_long<Op>), dim3((unsigned)std::min<int64_t>(d.num_ids, kLongGrid)), dim3(kNT), 0, st, a);
  SPP_HIP_TRY(hipGetLastError());
  return SPP_OK;
}

}  // namespace

extern "C" spp_status spp_field_mark(const spp_field_desc* desc, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  return run<Mark>("spp_field_mark", desc, false, workspace_dev, workspace_bytes, stream);
}

extern "C" spp_status spp_field_rows(const spp_field_desc* desc, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  return run<Rows>("spp_field_rows", desc, true, workspace_dev, workspace_bytes, stream);
}
