/*
 * include/spp.h -- C ABI of the MI355X-native mini-batch GNN data path
 * (libspp_hip.so), the drop-in boundary beneath SALIENT++'s `fast_sampler`
 * module (reference: fast_sampler/fast_sampler.cpp:1280-1396 is the pybind11
 * surface this replaces).
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures: device buffers are `void*`
 *     or typed pointers to HBM, streams are passed as `void*` (a hipStream_t),
 *     0 / NULL means the null stream;
 *   - every buffer is CALLER-OWNED unless stated otherwise; sampler/session
 *     objects own only their internal workspace;
 *   - every function returns SPP_OK (0) or a negative spp_status; the message
 *     is available from spp_last_error() (thread-local);
 *   - all functions are asynchronous w.r.t. the device unless documented as
 *     blocking (spp_sampler_wait, spp_session_next);
 *   - node ids are < 2^31 (the reference narrows to int32 inside sampling,
 *     fast_sampler.cpp:196-199) and tensors at the boundary are int64, as
 *     PyG / torch_sparse expect.
 */
#ifndef SPP_H
#define SPP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPP_ABI_VERSION 6
#define SPP_MAX_HOPS 8
#define SPP_MAX_PARTS 64

typedef int spp_status;
enum {
  SPP_OK = 0,
  SPP_ERR_INVALID = -1,   /* bad argument (TORCH_CHECK equivalents -> RuntimeError upstream) */
  SPP_ERR_HIP = -2,       /* HIP runtime error */
  SPP_ERR_CAPACITY = -3,  /* a batch exceeded the workspace the sampler was created for */
  SPP_ERR_STATE = -4      /* call sequence error (e.g. export before wait) */
};

int spp_abi_version(void);
const char* spp_last_error(void);
/* number of visible HIP devices, or <0 when no device / runtime (the product path fails loudly) */
int spp_device_count(void);

/* Live timing of the HBM-bound kernels with HIP events recorded on the launching stream
 * (bench.py's roofline leg).  spp_profile_enable(n) clears and starts recording: n = 1 times
 * every launch, n > 1 every n-th launch of a kind (two timing events around a ~100 us kernel cost ~7 us
 * of idle hardware queue each time: timing EVERY per-batch delivery slowed the pipeline by 5 %), 0 stops.
 * spp_profile_read is BLOCKING and returns the summed duration, launch count and processed
 * units (rows) of the TIMED launches of one kernel kind. */
#define SPP_PROF_GATHER 0     /* k_gather_rows   (serial_index)              */
#define SPP_PROF_ASSEMBLE 1   /* k_assemble      (distributed final assembly) */
#define SPP_PROF_CHAIN 2      /* one sampling chain of a group of batches, first launch to last, on its sampling stream
                                 (units = batches of the group; every chain is timed whatever n is: two events per
                                 ~0.6 ms chain; sample_adj x hops, sample_cpu.hpp:25-143 / fast_sampler.cpp:191-227) */
#define SPP_PROF_KINDS 3
void spp_profile_enable(int on);
spp_status spp_profile_read(int kind, double* total_ms, int64_t* launches, int64_t* units);

/* Run-time tuning knobs (measurement aid and the hook of embedders that pace the data path themselves).
 * "gather_wg_per_cu": workgroups per compute unit a row gather / delivery launch may put on the chip (default 16, or
 * SPP_GATHER_WG_PER_CU); value <= 0 only reads.
 * "gather_span": 1 (default; SPP_GATHER_SPAN=0) = rows of 16k + 8 bytes (200-byte rows of 100 fp16 features) out of a
 * table whose base and row stride are multiples of 16 bytes (>= the row + 8) into a 16-byte-aligned destination are moved
 * with 16-byte accesses (the loads read up to 8 bytes of the row's padding; never written); 0 = the 8-byte form;
 * value < 0 only reads.  Returns the previous value, or a negative spp_status. */
int spp_tune(const char* key, int value);

/* Asynchronously detected data errors.  The reference's CPU code does not range-check row indices
 * (fast_sampler.cpp:253-256 copies in[idx[i]] blindly); here a kernel that meets an index outside
 * its table clamps it to a valid row (no fault) and raises a bit in a per-device word in pinned host
 * memory, so a peer's bucketing bug surfaces as an error instead of wrong features.  The word is
 * read without any device synchronisation (a bit becomes visible once the offending kernel has run);
 * spp_session_next reports it as SPP_ERR_STATE, other callers poll it with spp_async_errors. */
#define SPP_AERR_GATHER_INDEX 1   /* spp_gather_rows*: idx[i] outside [0, src_rows)                       */
#define SPP_AERR_SERVE_ID 2       /* native exchange: a peer requested a row this rank does not own      */
#define SPP_AERR_ASSEMBLE 4       /* feature assembly: a source row outside its table                    */
/* returns the error mask of `device` (>= 0) or a negative spp_status; clear != 0 resets it */
int spp_async_errors(int device, int clear);

/* ------------------------------------------------------------------------- *
 * a1  std::mt19937 stream (fast_sampler/sample_cpu.hpp:11, seeding
 *     fast_sampler.cpp:994 `gen.seed(range.second*17+5)`): writes raw 32-bit
 *     outputs number skip .. skip+n-1 of mt19937(seed) to out_dev.
 * ------------------------------------------------------------------------- */
spp_status spp_mt19937_fill(uint32_t seed, int64_t skip, int64_t n, uint32_t* out_dev, void* stream);
/* seed of the batch whose idx range ends at `stop` (fast_sampler.cpp:994) */
uint32_t spp_batch_seed(int32_t stop);

/* ------------------------------------------------------------------------- *
 * a5  serial_index (fast_sampler.cpp:238-279):
 *       dst[i, :] = src[idx[i], :]  for i < min(n_idx, n_out)
 *     src is row-major [src_rows, row_bytes]; idx_elem_bytes is 8 (int64, the
 *     reference's dtype) or 4 (int32).  Rows i >= n_idx of dst are left
 *     untouched (the reference leaves them uninitialised).
 * ------------------------------------------------------------------------- */
spp_status spp_gather_rows(const void* src_dev, int64_t src_rows, int64_t row_bytes,
                           const void* idx_dev, int idx_elem_bytes, int64_t n_idx, int64_t n_out,
                           void* dst_dev, void* stream);
/* Same, for a source table whose rows are src_stride_bytes apart (>= row_bytes; 0 = dense).  The
 * resident feature table is kept with rows padded to the 128-B HBM fetch granule: a 200-B row then
 * costs 2 granules instead of 2.56 on average.  dst stays dense.
 * READABLE EXTENT: the table must hold src_rows * src_stride_bytes readable bytes (not just (src_rows - 1) * stride +
 * row_bytes): for rows of 16k + 8 bytes out of a 16-byte-aligned table with a 16-byte-multiple stride >= row_bytes + 8
 * the gather moves 16-byte pieces and the last piece of a row reads 8 bytes of that row's padding (never written;
 * spp_tune("gather_span", 0) keeps the 8-byte form, which reads row_bytes per row exactly).  The same holds for
 * spp_exchange_cfg.x_local_dev and the table of spp_session_export. */
spp_status spp_gather_rows_strided(const void* src_dev, int64_t src_rows, int64_t row_bytes,
                                   int64_t src_stride_bytes, const void* idx_dev, int idx_elem_bytes,
                                   int64_t n_idx, int64_t n_out, void* dst_dev, void* stream);

/* to_row_major (fast_sampler.cpp:281-308): column-major [rows, cols] -> row-major */
spp_status spp_to_row_major(const void* src_dev, int64_t rows, int64_t cols, int elem_bytes,
                            void* dst_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * a2-a4  On-GPU multi-hop neighbour sampler: sample_adj (sample_cpu.hpp:25-143)
 *        driven by multilayer_sample (fast_sampler.cpp:191-236).
 *        Bit-exact MFG (n_id, per-hop rowptr/col) vs the CPU algorithm for the
 *        same (seeds, fanouts, graph, rng seed).
 * ------------------------------------------------------------------------- */
typedef struct spp_sampler spp_sampler;

/* Optional ownership bucketing of the batch's node list, fused into the sampling chain (worker
 * distributed branch, fast_sampler.cpp:1017-1272): with num_parts > 0 every sampled batch also
 * carries the per-owner id lists, the VIP-cache hits and perm_partition_to_mfg, and their sizes
 * arrive with the counts -- no extra launch sequence and no host synchronisation per batch. */
typedef struct spp_partition_cfg {
  int32_t num_parts;                    /* P; 0 = bucketing off                                  */
  int32_t rank;                         /* this process's partition                              */
  int64_t offsets[SPP_MAX_PARTS + 1];   /* RangePartitionBook offsets (range_partition_book.cpp:38-55) */
  int32_t use_cache;                    /* Config.use_cache (fast_sampler.cpp:1108)               */
  const int32_t* cache_map_dev;         /* int32[cache_map_len]: node -> cache row, -1 = miss
                                           (spp_cache_build_map); read while batches are in flight */
  int64_t cache_map_len;
} spp_partition_cfg;

/* Which form of the sampling chain a sampler runs.  Every form computes the SAME batches (sample_cpu.hpp:25-143,
 * fast_sampler.cpp:191-227, :994) -- the forms differ in derived tables and kernel variants only.  By default the
 * library chooses by itself (sizes, free HBM); these fields pin a choice, and spp_sampler_get_info reports what
 * was chosen.  Convention for the int32 switches: 0 = automatic (the rule stated; the environment variable named
 * is honoured, read once at spp_sampler_create), > 0 = on, < 0 = off.  A zero-filled record is "all automatic". */
typedef struct spp_sampler_opts {
  int32_t col32;            /* int32 copy of `col` (SPP_COL32; auto: on).  Off: the kernels read the int64 array        */
  int32_t deg_tags;         /* degree tags in the spare top bits of the int32 entries (SPP_DEG_TAGS; auto: on when
                               ids leave >= 3 bits spare; used by a sampler only when every later fanout < the cap)     */
  int32_t row_stubs;        /* 128-byte row-stub table (SPP_ROW_STUBS; auto: when it takes <= 1/8 of the free HBM)      */
  int32_t rng_arena;        /* mt19937 streams of a whole epoch generated once and kept (auto: when the arena fits
                               rng_arena_mb and, without an explicit budget, 1/4 of the free HBM); off: per group
                               into the slots' ping-pong buffers (k_rng_fill)                                          */
  int64_t rng_arena_mb;     /* budget of that arena in MiB (0: SPP_RNG_ARENA_MB, default 16384)                         */
  int32_t fuse_scatter;     /* bucket scatter folded into the pick kernel (SPP_FUSE_SCATTER; auto = 1: where a pick
                               workgroup's edges give bucket runs of >= 8 pairs; 2: wherever the kernel can; off: never) */
  int32_t flag_tiled;       /* flag pass over the scatter's tiles (SPP_FLAG_TILED; auto: on)                            */
  int32_t rows_coalesced;   /* rows' per-edge arrays staged through LDS for fanouts <= 28 (SPP_ROWS_COALESCED; auto: on) */
  int32_t dedup_preread;    /* candidates pre-read the LDS table before their compare-and-swap (SPP_DEDUP_PREREAD;
                               auto: off)                                                                              */
  int64_t fuse_max_edges;   /* a hop of more edges per batch is never fused (0: SPP_FUSE_MAX_EDGES, default 262144)     */
  int64_t initial_edge_cap; /* all-neighbour hops (fanout < 0): starting capacity of the per-edge scratch, grown on
                               demand (0: min(nnz, 4 Mi))                                                              */
  int64_t reserved[4];      /* zero                                                                                    */
} spp_sampler_opts;

typedef struct spp_sampler_cfg {
  const int64_t* rowptr_dev;   /* int64[num_nodes+1], HBM resident           */
  const int64_t* col_dev;      /* int64[nnz], HBM resident                   */
  int64_t num_nodes;
  int64_t nnz;
  int32_t num_hops;            /* len(sizes) <= SPP_MAX_HOPS                 */
  int64_t sizes[SPP_MAX_HOPS]; /* fanouts, e.g. {15,10,5}; <0 = all neighbours */
  int64_t max_batch;           /* max number of seeds in one batch           */
  int32_t num_slots;           /* independent batches that may be in flight  */
  int32_t device;              /* HIP device ordinal                         */
  int32_t replace;             /* 1: sample WITH replacement (sample_cpu.hpp:74-82; only the free
                                  sample_adj exposes it, multilayer_sample passes false) */
  spp_partition_cfg part;      /* part.num_parts = 0: plain (single-GPU) batches */
  int64_t graph_generation;    /* The tables derived from (rowptr_dev, col_dev) -- the degree-tagged int32 neighbour
                                  array and the row stubs -- are shared by the samplers created over the same arrays AND
                                  the same generation.  A caller that rewrites the graph in place, or frees it and may get
                                  another graph of equal size at the same address, passes a new value (0 is fine for a
                                  graph that never changes). */
  spp_sampler_opts opts;       /* chain variants (zero-filled = automatic) */
} spp_sampler_cfg;

/* What a sampler actually runs -- the outcome of spp_sampler_opts' automatic rules -- and what its one-off tables
 * cost.  The per-hop arrays are in PROCESSING order (hop 0 = the seeds' neighbours). */
typedef struct spp_sampler_info {
  int32_t col32;               /* 1: the kernels read the int32 neighbour array                                        */
  int32_t deg_tags;            /* 1: degree pass from the nodes' tags (implies col32 and row_stubs)                    */
  int32_t row_stubs;           /* 1: row-stub table in use                                                             */
  int32_t rng_arena;           /* 1: epoch arena, 0: per-group generation, -1: no Session has decided yet              */
  int32_t idbits, tag_cap;     /* bits of a node id inside an int32 entry (32: untagged), largest degree a tag holds   */
  int32_t num_hops;
  int32_t dedup_buckets_log2;  /* finest bucket count of the radix-partitioned dedup                                   */
  int32_t dedup_table_slots;   /* LDS table of k_bucket_dedup                                                          */
  int32_t generic[SPP_MAX_HOPS];        /* edge-parallel path (fanout < 0 or > 32)                                     */
  int32_t fused_pick[SPP_MAX_HOPS];     /* k_hop_pick<kFuse> (no k_bucket_scatter launch)                              */
  int32_t flag_tiled[SPP_MAX_HOPS];     /* k_hop_flag_tiled                                                            */
  int32_t rows_coalesced[SPP_MAX_HOPS]; /* k_hop_rows_coalesced                                                        */
  int32_t bucket_log2[SPP_MAX_HOPS];    /* buckets of the hop                                                          */
  /* one-off set-up work: wall-clock milliseconds THIS sampler spent building a table (0 when it found the table of
   * an earlier sampler over the same graph, or has none) and the tables' sizes in bytes */
  double col32_ms, row_stubs_ms, rng_arena_ms;
  int64_t col32_bytes, row_stubs_bytes, rng_arena_bytes;
  int64_t rng_arena_batches;   /* streams the arena holds                                                              */
} spp_sampler_info;

/* counts of one sampled batch; hops in OUTPUT order (outermost first, after the
 * std::reverse at fast_sampler.cpp:224) */
typedef struct spp_mfg_counts {
  int64_t num_nodes;              /* U = len(n_id)                           */
  int64_t num_seeds;
  int32_t num_hops;
  int64_t T[SPP_MAX_HOPS];        /* target rows of hop                      */
  int64_t S[SPP_MAX_HOPS];        /* source nodes of hop                     */
  int64_t E[SPP_MAX_HOPS];        /* sampled edges of hop                    */
  int64_t draws;                  /* RNG outputs consumed                    */
  /* with spp_partition_cfg.num_parts = P > 0: [0,P) nodes owned by partition m (cache hits
   * excluded when use_cache), [P] cache hits, [P+1] reserved (host-resident local rows: always 0,
   * every local row lives in HBM); else zeros */
  int64_t part_counts[SPP_MAX_PARTS + 2];
} spp_mfg_counts;

/* caller-owned, exact-size destination buffers for one batch's MFG */
typedef struct spp_mfg_out {
  int64_t* n_id;                  /* int64[U]                                */
  int64_t* rowptr[SPP_MAX_HOPS];  /* int64[T_h+1], output order              */
  int64_t* col[SPP_MAX_HOPS];     /* int64[E_h],   output order              */
  /* bucketing outputs (NULL = skip; ignored when the sampler has no spp_partition_cfg):          */
  int64_t* parts;                 /* int64[sum part_counts[0..P)]: global node ids grouped by owner,
                                     MFG order inside a group (fast_sampler.cpp:1063-1068)        */
  int64_t* cached;                /* int64[part_counts[P]]: cache rows of the hits (:1256)         */
  int64_t* perm;                  /* int64[U]: perm_partition_to_mfg (:1085, :1246-1252)           */
  /* Row references (opt-in; spp_session_export / spp_session_export_group with x_out_dev == NULL): instead of
   * writing the batch's feature matrix the delivery writes WHERE every row lives, for a consumer whose first layer
   * reads the rows exactly once (spp_sage_operand_forward_rows) -- x = cat(...)[perm] (transferers.py:472-486) is
   * neither written nor read back.  row_addr[j] = device address of the feature row of MFG node j: in the local
   * partition (or the one resident table of a single-GPU session), in the VIP cache, in a peer's partition (P2P
   * transport), or -- RCCL transport -- in x_remote, into which the rows received for THIS batch are copied (dense
   * rows, peer-major, request order: U - part_counts[rank] - part_counts[P] of them); the group's receive buffer is
   * free again when the launch completes, so nothing outlives the delivery but caller-owned memory and the
   * resident tables. */
  int64_t* row_addr;              /* int64[U], or NULL                                             */
  void* x_remote;                 /* [remote rows, row_bytes] dense, or NULL (nothing remote / P2P) */
} spp_mfg_out;

/* rowptr_dev / col_dev must stay valid AND unchanged for the sampler's lifetime: an int32 copy of the
 * neighbour array and a row-stub table (degree, row start and first neighbours of every node in one
 * 128-byte record; SPP_ROW_STUBS=0 disables it, it is skipped when HBM is short) are derived from them
 * once and shared by the samplers created over the same arrays and graph_generation
 * (spp_sampler_workspace_bytes includes them and the mt19937 arena).  The cache map of a spp_partition_cfg may
 * be rewritten between Sessions (its membership bits are rebuilt by spp_session_create). */
spp_status spp_sampler_create(const spp_sampler_cfg* cfg, spp_sampler** out);
void spp_sampler_destroy(spp_sampler* s);
/* bytes of HBM workspace held by the sampler (all slots) */
int64_t spp_sampler_workspace_bytes(const spp_sampler* s);
/* A persistent HIP stream owned by the sampler that the consumer may use for spp_session_export /
 * spp_sampler_export / spp_sampler_gather (as a hipStream_t).  Using it keeps the per-batch delivery
 * kernel on a hardware queue of its own; any other stream works too. */
void* spp_sampler_deliver_stream(spp_sampler* s);
/* the configuration the sampler was created with */
spp_status spp_sampler_get_cfg(const spp_sampler* s, spp_sampler_cfg* out);
/* the chain variants it runs and the cost of its one-off tables (BLOCKING when the epoch arena is still being
 * generated: rng_arena_ms is that launch's duration) */
spp_status spp_sampler_get_info(spp_sampler* s, spp_sampler_info* out);

/* Enqueue the sampling of one batch into `slot` on `stream`.
 * seeds_dev: int64[n_seeds] in HBM.  The RNG stream is mt19937(rng_seed) with
 * the first rng_skip outputs discarded (rng_skip = 0 for Session batches). */
spp_status spp_sampler_sample(spp_sampler* s, int32_t slot, const int64_t* seeds_dev,
                              int64_t n_seeds, uint32_t rng_seed, int64_t rng_skip, void* stream);
/* BLOCKING: waits until the batch in `slot` is sampled and returns its counts. */
spp_status spp_sampler_wait(spp_sampler* s, int32_t slot, spp_mfg_counts* out);
/* Write the slot's MFG into caller buffers (int64, reference layout) on `stream`. */
spp_status spp_sampler_export(spp_sampler* s, int32_t slot, const spp_mfg_out* out, void* stream);
/* Fused serial_index over the slot's node list (worker lines fast_sampler.cpp:1006-1010):
 *   dst[i,:] = src[n_id[i],:] for i < n_rows   (n_rows = U for x, batch size for y) */
spp_status spp_sampler_gather(spp_sampler* s, int32_t slot, const void* src_dev, int64_t src_rows,
                              int64_t row_bytes, int64_t src_stride_bytes /* 0 = dense */, int64_t n_rows,
                              void* dst_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * a10/a11  RangePartitionBook (range_partition_book.cpp:85-112) and Cache
 *          (range_partition_book.cpp:116-195) lookups on device.
 *          offsets_host: int64[P+1] on the HOST (P <= SPP_MAX_PARTS).
 *          cache_map_dev: int32[cache_map_len] direct map, -1 = not cached.
 * ------------------------------------------------------------------------- */
spp_status spp_nid2partid(const int64_t* offsets_host, int32_t n_offsets, const int64_t* nids_dev,
                          int64_t n, int64_t* out_dev, void* stream);
spp_status spp_cache_build_map(const int64_t* cached_vertices_dev, int64_t n_cached,
                               int32_t* cache_map_dev, int64_t cache_map_len, void* stream);
spp_status spp_cache_lookup(const int32_t* cache_map_dev, int64_t cache_map_len,
                            const int64_t* nids_dev, int64_t n, uint8_t* is_cached_dev /*nullable*/,
                            int64_t* cache_nid_dev /*nullable*/, void* stream);

/* ------------------------------------------------------------------------- *
 * a8/a9  per-batch ownership bucketing of the MFG node list
 *        (worker distributed branch, fast_sampler.cpp:1017-1262).
 *   parts_out_dev  int64[U]   concat(partition_nids[0..P-1])
 *   cached_out_dev int64[U]   cache-local indices of hits (first counts[P] valid)
 *   perm_out_dev   int64[U]   perm_partition_to_mfg
 *   counts_out_dev int64[P+2] [len(parts[0..P-1]), n_cached, n_local_on_host]
 *   cpu_local_out_dev int64[U] nullable: (v-off[rank])-x_gpu_rows of local rows
 *                     living in host memory, MFG order
 *   workspace: spp_partition_workspace_bytes(U) bytes of HBM scratch.
 * ------------------------------------------------------------------------- */
int64_t spp_partition_workspace_bytes(int64_t max_nodes);
spp_status spp_partition_batch(const int64_t* n_id_dev, int64_t U, const int64_t* offsets_host,
                               int32_t P, int32_t rank, int32_t use_cache,
                               const int32_t* cache_map_dev, int64_t cache_map_len,
                               int64_t x_gpu_rows, int64_t* parts_out_dev, int64_t* cached_out_dev,
                               int64_t* perm_out_dev, int64_t* counts_out_dev,
                               int64_t* cpu_local_out_dev, void* workspace_dev,
                               int64_t workspace_bytes, void* stream);

/* a16 (transferers.py:472-486) fused final assembly, replacing zeros+scatter+cat+permute:
 *   x_out[i,:] = row perm[i] of the virtual concatenation
 *                [ parts[0] rows | ... | parts[P-1] rows | cache rows ]
 * where the rank-th segment is gathered straight from x_local (local id =
 * n_id[i]-off[rank]), the cache segment from cache_feats[cached_nids], and every
 * other segment m from recv_dev (rows received from peer m, packed in partition
 * order with the own-rank segment absent). seg_start_host: int64[P+2] prefix of
 * segment lengths in the virtual concatenation. */
spp_status spp_assemble_features(const int64_t* n_id_dev, const int64_t* perm_dev, int64_t U,
                                 const int64_t* seg_start_host, int32_t P, int32_t rank,
                                 int64_t rank_offset, const void* x_local_dev, int64_t x_local_rows,
                                 const void* recv_dev, const void* cache_feats_dev,
                                 const int64_t* cached_nids_dev, int64_t row_bytes,
                                 int64_t x_local_stride_bytes /* 0 = dense */,
                                 int64_t cache_stride_bytes /* 0 = dense */,
                                 const int64_t* recv_base_host /* int64[P] or NULL: row of recv_dev where
                                    peer m's rows for this batch start, when recv_dev holds the rows of
                                    several batches (one exchange per group) */,
                                 void* x_out_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * a6/a7  Session runtime (fast_sampler.cpp:533-936 Session, :963-1016 worker,
 *        non-distributed branch).  The reference's CPU worker pool + MPMC queue
 *        + semaphore back-pressure is replaced by `max_items_in_queue` batch
 *        slots kept in flight on HIP streams; batches are delivered in index
 *        order.  Batch ranges and per-batch seeds follow fast_sampler.cpp:587-627
 *        and :994 exactly.
 * ------------------------------------------------------------------------- */
typedef struct spp_session spp_session;

typedef struct spp_session_cfg {
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_nodes;
  int64_t nnz;
  const int64_t* idx_dev;          /* int64[n_idx] seed nodes of this epoch, HBM */
  int64_t n_idx;
  int64_t batch_size;
  int32_t num_hops;
  int64_t sizes[SPP_MAX_HOPS];
  int32_t skip_nonfull_batch;
  int32_t force_exact_num_batches;
  int64_t exact_num_batches;
  int32_t max_items_in_queue;      /* upper bound on batches in flight (slots) */
  int32_t group_size;              /* batches sampled per launch sequence, at most 16 (0 = auto: max_items/4 capped at
                                      16 when 32 or more slots are allowed, else max_items/2 capped at 8);
                                      max_items_in_queue / group_size slot-sets (at most 8) are in flight and share
                                      the sampler's two sampling streams */
  int32_t device;
  /* Optional: borrow an existing sampler (same graph, fanouts; max_batch and num_slots at least
   * what this epoch needs) instead of allocating workspace per epoch -- the counterpart of the
   * reference's process-global worker pool that outlives Sessions (fast_sampler.cpp:512-513).
   * A borrowed sampler is not destroyed by spp_session_destroy. */
  spp_sampler* sampler;
  /* Optional ownership bucketing (NULL = off).  With a borrowed sampler it must equal the
   * sampler's own spp_partition_cfg. */
  const spp_partition_cfg* part;
  /* Optional native feature exchange (NULL = off; needs `part`).  See spp_exchange_cfg below. */
  const struct spp_exchange_cfg* exchange;
  /* Ordering of the session's own streams against the producer of its device inputs.  idx_dev (and
   * the feature / label / cache tables handed to export or spp_exchange_cfg) may still be the output
   * of work QUEUED on the caller's stream (e.g. a shuffle kernel writing this epoch's seed ids): with
   * order_after_input_stream != 0 every stream the session launches on first waits for what
   * `input_stream` (a hipStream_t, NULL = the null stream) holds at creation time.  0 = the inputs
   * are complete already. */
  void* input_stream;
  int32_t order_after_input_stream;
} spp_session_cfg;

typedef struct spp_batch_desc {
  int64_t batch_index;
  int32_t start, stop;             /* idx range, as PreparedSample's pair      */
  int32_t slot;
  spp_mfg_counts counts;
} spp_batch_desc;

spp_status spp_session_create(const spp_session_cfg* cfg, spp_session** out);
void spp_session_destroy(spp_session* s);
int64_t spp_session_num_total_batches(const spp_session* s);
int64_t spp_session_num_consumed_batches(const spp_session* s);
/* fills ranges (2*num_total_batches int32) -- the table of fast_sampler.cpp:587-627 */
spp_status spp_session_batch_ranges(const spp_session* s, int32_t* out_start_stop);
/* BLOCKING. Returns 1 and fills *out when the next batch (index order) is ready,
 * 0 at end of epoch (the reference returns None), <0 on error.
 * How far ahead the session samples (the counterpart of max_items_in_queue, fast_sampler.cpp:533-586): the slots form
 * `sets` slot-sets of group_size batches; the launcher keeps chains in flight for at most
 *     sets - refill_lag   groups beyond the groups the consumer has FINISHED
 * (refill_lag = SPP_REFILL_LAG, default 1, applied only with >= 3 sets and capped at sets - 2: the chain that refills a
 * freed set is enqueued one group later, for a set whose deliveries completed a group ago).  A group counts as finished
 * when the consumer COMES BACK FOR MORE after exporting its last batch -- at the next spp_session_next /
 * spp_session_try_next / spp_session_next_group -- not at that export: a consumer that exports a group's last batch and then
 * only polls slot events, or calls spp_session_quiesce, gets no refill until it asks for the next batch. */
int spp_session_next(spp_session* s, spp_batch_desc* out);
/* Non-blocking form (try_get_batch, fast_sampler.cpp:658-670): 2 when the next batch is not ready
 * yet, otherwise exactly what spp_session_next returns. */
int spp_session_try_next(spp_session* s, spp_batch_desc* out);
/* Write the batch returned by the last spp_session_next into caller buffers on
 * `stream`: MFG (as spp_sampler_export), optional x = x_src[n_id] and
 * y = y_src[n_id[:stop-start]]; then recycle its slot (the next pending batch
 * starts sampling into it, ordered after these copies). */
spp_status spp_session_export(spp_session* s, const spp_mfg_out* mfg,
                              const void* x_src_dev, int64_t x_rows, int64_t x_row_bytes,
                              int64_t x_src_stride_bytes /* 0 = dense */, void* x_out_dev,
                              const void* y_src_dev, int64_t y_rows, int64_t y_row_bytes, void* y_out_dev,
                              void* stream);
/* Group-at-a-time consumption.  The batches of a sampling group (spp_session_group_size of them; fewer in
 * the epoch's last group) become ready together, and delivering them with ONE launch keeps the delivery
 * stream's hardware queue busy: a launch per batch cost ~25 us of queue idle time around every ~105 us kernel
 * (completion signal, event markers, dispatch ramp), which bounded the whole pipeline.
 *   spp_session_next_group: the descriptors of ALL batches of the next group (index order).  Returns 1 and
 *     fills out[0 .. *n_out) when the group is sampled (and, with the native exchange, exchanged); 0 at the end
 *     of the epoch; 2 when block == 0 and the group is not ready yet; < 0 on error.  With consumer-issued
 *     exchanges (spp_exchange_cfg.issue_on_consumer) this is the program point at which the group's own exchange
 *     -- and, with three or more slot-sets, the next group's -- is issued.
 *   spp_session_export_group: writes the n batches returned by the last spp_session_next_group into caller
 *     buffers with one launch on `stream` (per batch as spp_session_export: MFG, x = x_src[n_id] or the rows
 *     assembled from the exchange, y = y_src[n_id[:stop-start]]), then recycles the group's slot-set.
 *   Fetch as a group, deliver one by one: instead of ONE spp_session_export_group the group returned by
 *     spp_session_next_group may be exported member by member, in index order, by n calls of spp_session_export
 *     (one launch each, on the stream given to each call; the slot-set is recycled after the last).  The caller
 *     then sizes and allocates the outputs of all n batches at once and pays one export call per batch, while the
 *     GPU sees the per-batch launches -- which measured faster than the single launch.  Once a
 *     member has been exported this way spp_session_export_group is refused for that group.
 * spp_session_next and the group calls may be mixed only at group boundaries. */
typedef struct spp_group_out {
  spp_mfg_out mfg;                 /* as spp_session_export's mfg (pointers may be NULL = skip) */
  void* x_out;                     /* [U, x_row_bytes] dense, or NULL                           */
  void* y_out;                     /* [stop - start, y_row_bytes], or NULL                      */
} spp_group_out;
int spp_session_next_group(spp_session* s, int32_t block, spp_batch_desc* out /* [group_size] */, int32_t* n_out);
spp_status spp_session_export_group(spp_session* s, int32_t n, const spp_group_out* outs /* [n] */,
                                    const void* x_src_dev, int64_t x_rows, int64_t x_row_bytes,
                                    int64_t x_src_stride_bytes /* 0 = dense */,
                                    const void* y_src_dev, int64_t y_rows, int64_t y_row_bytes, void* stream);
/* total time spp_session_next spent blocked, microseconds, and number of blocking waits
 * (fast_sampler.cpp:788-799 total_blocked_dur / total_blocked_occasions) */
int64_t spp_session_blocked_us(const spp_session* s);
int64_t spp_session_blocked_occasions(const spp_session* s);
/* batches per sampling group (they become ready together; exchanges are per group) */
int32_t spp_session_group_size(const spp_session* s);
/* the sampler owned by the session (for spp_sampler_gather on the current slot etc.) */
spp_sampler* spp_session_sampler(spp_session* s);

/* ------------------------------------------------------------------------- *
 * e1-e3  Remote-feature exchange over RCCL/xGMI, native (the DeviceDistributedPrefetcher
 *        stages of transferers.py:186-372: counts C1 :757, node ids C2 :709, feature rows C3 :521,
 *        serve K5 :645-658, combine :472-486).  One exchange per GROUP of batches (fewer, larger
 *        collectives), driven by a session-owned thread one group ahead of the consumer:
 *          all-gather of the request counts -> grouped send/recv of int32 node ids ->
 *          row gather out of the local partition -> grouped send/recv of the rows;
 *        spp_session_export then writes x in MFG order straight from {local partition,
 *        received rows, VIP cache} in the same launch that delivers the MFG and the labels.
 *        Every rank must run the same number of batches per epoch (force_exact_num_batches,
 *        as the reference's distributed mode requires).
 *
 *        fp8 partitions (f3c): with spp_exchange_cfg.x_elem = SPP_ELEM_FP8_E4M3 the partition, the cache and
 *        everything the exchange moves (served rows, send / receive buffers) are e4m3 bytes, row_bytes = F per
 *        row -- 4 + F algorithmic bytes per remote row on the wire against 4 + 2F for fp16 -- and only the
 *        assembly inside the delivery launch knows the element type: it writes fp16 rows
 *        x[r, c] = fp16(float32(q[r, c]) * 2^scale_log2[c]) (rounded once, to nearest even: the contract of
 *        spp_gather_rows_fp8), so the OUTPUT row pitch of spp_session_export / spp_session_export_group is
 *        2 * row_bytes and the caller sizes x_out_dev accordingly.  A row quantised by its owner is
 *        dequantised by its requester: every rank must hold the same column exponents, which the creation-time
 *        rendezvous checks (scales_tag).  The three fp8 fields sit at the END of spp_exchange_cfg: a
 *        zero-initialised struct (x_elem = 0) moves and assembles bytes exactly as before.
 * ------------------------------------------------------------------------- */
typedef struct spp_comm spp_comm;

#define SPP_COMM_ID_BYTES 128
/* rank 0: make the rendezvous token (ncclGetUniqueId); ship it to the other ranks out of band
 * (e.g. torch.distributed broadcast) */
spp_status spp_comm_unique_id(void* out_id /* SPP_COMM_ID_BYTES */);
/* collective over all ranks: ncclCommInitRank on `device`.  librccl.so.1 is resolved at run time
 * (the copy PyTorch already loaded when there is one). */
spp_status spp_comm_create(const void* id, int32_t rank, int32_t world, int32_t device, spp_comm** out);
/* `world` communicators that live in ONE process and copy device-to-device (no RCCL): ranks are
 * driven by different host threads.  A TEST AID compiled into the product library (the suite rehearses
 * the exchange logic above the transport on one GPU with it): refused with SPP_ERR_INVALID unless the
 * environment says SPP_ALLOW_LOCAL_COMM=1. */
spp_status spp_comm_create_local(int32_t world, int32_t device, spp_comm** out /* [world] */);
void spp_comm_destroy(spp_comm* c);
int32_t spp_comm_rank(const spp_comm* c);
int32_t spp_comm_world(const spp_comm* c);

typedef struct spp_exchange_cfg {
  spp_comm* comm;                  /* rank / world must match spp_partition_cfg                     */
  const void* x_local_dev;         /* this rank's feature rows [offsets[rank], offsets[rank+1]), HBM */
  int64_t x_local_rows;
  int64_t row_bytes;
  const void* cache_feats_dev;     /* VIP cache rows; NULL without use_cache                         */
  int64_t cache_rows;
  int64_t x_local_stride_bytes;    /* distance between rows of x_local / of the cache (0 = dense)    */
  int64_t cache_stride_bytes;
  /* P2P transport (opt-in; SURVEY 8(e) "direct P2P loads of peer HBM inside the gather kernel"): peer_x_dev != NULL
   * names, for every rank m, the base address IN THIS PROCESS of rank m's partition (its x_local: same row_bytes and
   * stride; peer_x_dev[rank] is ignored) -- plain device pointers when the ranks share a process, otherwise
   * mappings opened with spp_ipc_open from handles the owners exported (spp_ipc_export).  The delivery then reads a
   * remote row straight out of its owner's HBM over xGMI: no id exchange, no serve gather, no send / receive
   * buffers, no host read per group, and `comm` may be NULL.  The partitions must stay allocated and unchanged while
   * any peer's Session runs. */
  const void* const* peer_x_dev;   /* host array [num_parts], or NULL = exchange over `comm`         */
  int64_t peer_x_stride_bytes;     /* distance between rows of every peer's table (0 = x_local's)    */
  int32_t issue_on_consumer;       /* 0: a session thread issues each group's exchange as soon as its
                                      sampling completes (most overlap).  1: spp_session_next issues it,
                                      at the same point of the program on every rank (own group when
                                      needed, the next one from mid-group on) -- use it when the caller
                                      interleaves collectives of its own communicator, e.g. DDP gradient
                                      all-reduces: both communicators' kernels are then queued in the
                                      same order on every rank.                                      */
  /* Element type of the rows.  SPP_ELEM_F32 (0) / SPP_ELEM_F16 / SPP_ELEM_BF16: opaque bytes, delivered as they are.
   * SPP_ELEM_FP8_E4M3: e4m3 rows with per-column exponents, delivered as fp16 (see e1-e3 above).  Needs
   * row_bytes % 16 == 0, row strides that are multiples of 16, 16-byte aligned x_local_dev / cache_feats_dev /
   * scale_log2_dev, and the exchange over `comm` (peer_x_dev == NULL). */
  int32_t x_elem;
  const int8_t* scale_log2_dev;    /* [row_bytes] column exponents in [-64, 63], HBM; required iff fp8; must stay
                                      allocated while the Session lives                               */
  uint64_t scales_tag;             /* hash of the row_bytes exponent bytes (FNV-1a 64; 0 for a non-fp8 session):
                                      compared across the ranks at creation, a mismatch fails
                                      spp_session_create on every rank                                */
} spp_exchange_cfg;

/* Cross-process mapping of a device allocation (hipIpcGetMemHandle / hipIpcOpenMemHandle), for the P2P transport:
 * the owner exports the allocation that CONTAINS ptr_dev (handle_out: SPP_IPC_HANDLE_BYTES bytes; *offset_out = ptr_dev's
 * offset inside it), ships both out of band (e.g. torch.distributed all_gather_object), and a peer process on the same
 * node opens the handle and adds the offset.  spp_ipc_close unmaps what spp_ipc_open returned. */
#define SPP_IPC_HANDLE_BYTES 64
spp_status spp_ipc_export(const void* ptr_dev, void* handle_out, int64_t* offset_out);
spp_status spp_ipc_open(const void* handle, int32_t device, void** base_out);
spp_status spp_ipc_close(void* base);

/* BLOCKING: returns when the session's threads have issued everything they can without further
 * consumption (sampling chains and exchanges of the slot-sets in flight) and that work has completed
 * on the GPU.  Call it on every rank before issuing collectives of ANOTHER communicator (e.g. a
 * torch.distributed barrier): kernels of two communicators that wait for their peers must not be
 * queued behind one another in opposite orders on different ranks.  A finished group that has not been reported yet
 * (see spp_session_next: the report is deferred to the consumer's next request) stays unreported: quiesce starts no
 * refill chain of its own. */
spp_status spp_session_quiesce(spp_session* s);
/* bytes this rank sent / received through the exchange so far (ids + rows + counts) */
spp_status spp_session_exchange_stats(const spp_session* s, int64_t* sent_bytes, int64_t* recv_bytes);

/* ------------------------------------------------------------------------- *
 * f1  VIP analytic model (driver/drivers/ddp.py:135-239 get_frequency_tensors_fast): per vertex,
 *     the probability of being touched by one mini-batch of `batch_size` seeds drawn from
 *     train_idx, propagated over `fanouts` (in the order given, as the reference iterates them).
 *     float64.  out_dev: double[num_nodes]; workspace_dev: double[3*num_nodes].
 *     create_vip_cache (ddp.py:417-570) ranks the remote vertices by it.
 * ------------------------------------------------------------------------- */
spp_status spp_vip_frequencies(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_nodes,
                               const int64_t* train_idx_dev, int64_t n_train, int64_t batch_size,
                               const int64_t* fanouts_host, int32_t num_hops, double* out_dev,
                               double* workspace_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * f3  Mean aggregation of SAGEConv over one MFG hop (driver/models.py:19-56: SAGEConv(aggr='mean')
 *     on ((x, x_target), adj_t)); fp32 accumulate and output.
 *       forward : out[t,:] = sum_{e in row t} x[col[e],:] / max(deg t, 1);  x fp32 or fp16, rows
 *                 x_stride_elems apart (the batch's fp16 features can be aggregated directly);
 *                 out rows out_stride_elems apart (0 = dense), so the result can land in the left
 *                 half of the [T, 2F] operand of one fused lin_l|lin_r GEMM
 *       backward: grad_x[col[e],:] += grad_out[t,:] / deg t  (grad_x [S,F] fp32, zeroed by the
 *                 caller; hardware fp32 atomics, so the summation order is not fixed)
 *
 *     Every entry of this block and of the sum block below except spp_csr_mean_backward (the bare scatter step, which
 *     adds), spp_relu_dropout_* (element-wise) and the GAT entries is a FIXED-TYPE SPELLING of the descriptor entries
 *     spp_agg_forward / spp_agg_backward further down: fp32 out / grad / z, x fp32 or fp16 by the `*_is_half` flag
 *     (any non-zero value = fp16), source / epilogue / form as the name says.  It fills a descriptor and shares the
 *     descriptor path's validation, defaults and launch; errors name the entry that was called.  What an entry asks
 *     beyond the descriptor is said at its declaration.
 * ------------------------------------------------------------------------- */
spp_status spp_csr_mean_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t F,
                                float* out_dev, int64_t out_stride_elems, void* stream);
spp_status spp_csr_mean_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                 const float* grad_out_dev, int64_t grad_out_stride_elems, int64_t F,
                                 float* grad_x_dev, void* stream);
/* The fused operand of SAGEConv, [mean_j x_j | x_target] (fp32 [T, 2F], one GEMM with [W_l | W_r] then
 * replaces lin_l(mean) + lin_r(x_target)): the targets are the first T rows of x (the MFG contract,
 * driver/models.py:44-45 `x_target = x[:size[1]]`), converted to fp32 in the same pass.  The operand entries take an
 * explicit out_stride_elems >= 2F (their backwards an explicit grad_out_stride_elems >= 2F): 0 is refused, where the
 * descriptor reads it as dense. */
spp_status spp_sage_operand_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                    const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t F,
                                    float* out_dev, int64_t out_stride_elems /* >= 2F */, void* stream);
/* The same operand straight from the RESIDENT feature table (opt-in consumer of the data path, DESIGN section 5
 * "fused first layer"): row j of the batch is table[n_id[j]] (n_id int64 [S], the batch's node ids as the Session
 * delivers them; table rows table_stride_elems apart, fp16 or fp32), so the batch's feature matrix x = table[n_id]
 * (fast_sampler.cpp:1004-1016 `x = serial_index(x_cpu, n_id)`) is never written and read back -- the rows are summed
 * in the same order as spp_sage_operand_forward sums the rows of a materialised x: the operand is bit-identical.
 * An id outside [0, table_rows) reads row 0. */
spp_status spp_sage_operand_forward_table(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                          const void* table_dev, int32_t table_is_half, int64_t table_stride_elems,
                                          int64_t table_rows, const int64_t* n_id_dev, int64_t F, float* out_dev,
                                          int64_t out_stride_elems /* >= 2F */, void* stream);
/* The same operand from ROW REFERENCES (spp_mfg_out.row_addr): row j of the batch is the F elements at device
 * address row_addr_dev[j] (fp16 or fp32; 8-byte aligned fp16 / 16-byte aligned fp32 rows).  Same rows, same summation
 * order as spp_sage_operand_forward over the assembled x: the operand is bit-identical.  This entry has the vector form
 * only: F % 4 == 0, out_dev 16-byte aligned, out_stride_elems % 4 == 0 (the descriptor's SPP_AGG_ROWS takes any F). */
spp_status spp_sage_operand_forward_rows(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                         const int64_t* row_addr_dev, int32_t rows_are_half, int64_t F, float* out_dev,
                                         int64_t out_stride_elems /* >= 2F */, void* stream);
/* dst[j,:] = the row_bytes bytes at row_addr_dev[j], j < n: the feature matrix itself out of row references
 * (what any consumer other than the fused first layer reads: RowRefs.materialize()). */
spp_status spp_gather_row_refs(const int64_t* row_addr_dev, int64_t n, int64_t row_bytes, void* dst_dev, void* stream);
/* Its backward: grad_x [S, F] is written completely -- rows < T start from the gradient of the x_target
 * half, the others from zero, then the mean's gradient is scattered on top (fp32 atomics). */
spp_status spp_sage_operand_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                     int64_t num_sources, const float* grad_out_dev, int64_t grad_out_stride_elems,
                                     int64_t F, float* grad_x_dev, void* stream);
/* The same gradient by GATHER over the transposed hop (built on the fly: count, scan, fill): no fp32
 * atomics -- 42 M of them per step at papers scale run at the chip's atomic rate.  workspace_dev:
 * spp_sage_operand_backward_workspace_bytes(T, S, E) bytes of HBM, 16-byte aligned. */
int64_t spp_sage_operand_backward_workspace_bytes(int64_t num_targets, int64_t num_sources, int64_t num_edges);
spp_status spp_sage_operand_backward_gather(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                            int64_t num_sources, int64_t num_edges, const float* grad_out_dev,
                                            int64_t grad_out_stride_elems, int64_t F, float* grad_x_dev,
                                            void* workspace_dev, int64_t workspace_bytes, void* stream);
/* x = F.relu(x); x = F.dropout(x, p, training)  (driver/models.py:47-48) in one pass; the keep / drop
 * decisions come from a counter-based generator keyed by `seed`, and the backward pass needs only y
 * (y > 0 exactly where the input was positive and kept): grad_x = grad * scale where y > 0, scale = 1/(1-p)
 * in training and 1 in eval mode. */
spp_status spp_relu_dropout_forward(const float* x_dev, int64_t n, float p, int32_t training, uint64_t seed,
                                    float* y_dev, void* stream);
spp_status spp_relu_dropout_backward(const float* grad_dev, const float* y_dev, int64_t n, float scale,
                                     float* grad_x_dev, void* stream);
/* The same two steps without the activated copy: spp_sage_operand_forward_act builds [mean | x_target] of
 * relu_dropout(x) from the PRE-activation x (fp32, dense rows, F % 4 == 0), applying the activation to every
 * row as it is loaded -- the values spp_relu_dropout_forward(x, n = S*F, p, training, seed) would have
 * written -- and spp_relu_dropout_backward_pre recomputes the mask from x and the same (p, training, seed):
 * grad_x = grad / (1-p) where x > 0 and the element was kept (n % 4 == 0). */
spp_status spp_sage_operand_forward_act(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                        const float* x_dev, int64_t F, float* out_dev, int64_t out_stride_elems,
                                        float p, int32_t training, uint64_t seed, void* stream);
spp_status spp_relu_dropout_backward_pre(const float* grad_dev, const float* z_dev, int64_t n, float p,
                                         int32_t training, uint64_t seed, float* grad_x_dev, void* stream);
/* spp_sage_operand_backward_gather with spp_relu_dropout_backward_pre applied to every row before it is
 * stored: grad_x_dev becomes the gradient w.r.t. the pre-activation z_pre_dev (dense fp32 [S, F]). */
spp_status spp_sage_operand_backward_gather_act(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                                int64_t num_sources, int64_t num_edges, const float* grad_out_dev,
                                                int64_t grad_out_stride_elems, int64_t F, float* grad_x_dev,
                                                void* workspace_dev, int64_t workspace_bytes, const float* z_pre_dev,
                                                float p, int32_t training, uint64_t seed, void* stream);

/* GATConv(heads=1) message passing over one MFG hop (driver/models.py:195-231):
 *   e_ij = leaky_relu(a_src[j] + a_dst[i], negative_slope) over row i without its diagonal entry plus
 *   the self loop (i, i) that GATConv adds (set_diag);  out[i,:] = sum_j softmax_j(e_ij) h[j,:].
 *   h fp32 [S,F] dense (targets are its first rows), a_src fp32[S], a_dst fp32[T]; row_max/row_sum
 *   fp32[T] keep the softmax statistics for the backward pass.  Backward: grad_h [S,F] and
 *   grad_a_src [S] zeroed by the caller (fp32 atomics), grad_a_dst [T] written. */
spp_status spp_gat_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                           const float* h_dev, int64_t F, const float* a_src_dev, const float* a_dst_dev,
                           float negative_slope, float* out_dev, float* row_max_dev, float* row_sum_dev,
                           void* stream);
spp_status spp_gat_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                            const float* h_dev, int64_t F, const float* a_src_dev, const float* a_dst_dev,
                            float negative_slope, const float* out_dev, const float* row_max_dev,
                            const float* row_sum_dev, const float* grad_out_dev, float* grad_h_dev,
                            float* grad_a_src_dev, float* grad_a_dst_dev, void* stream);

/* GATConv in aggregate-then-project form (same function, far less work: see csrc/gat.hip).
 * With v_src = W^T att_src, v_dst = W^T att_dst (K-vectors):
 *   spp_gat_logits:            a_src[j] = x_j . v_src (all S rows), a_dst[i] = x_i . v_dst (the first T rows)
 *   spp_gat_aggregate_forward: z_i = sum_j softmax_j(leaky_relu(a_src[j] + a_dst[i])) x_j  over row i of the hop
 *                              (diagonal entry dropped, self loop added, as GATConv's set_diag); the layer's
 *                              output is then z @ W^T.  x rows are fp32, fp16 or bf16 (`x_is_half` is the element
 *                              code: 0 fp32, 1 fp16, 2 bf16, see spp_elem below), K % 4 == 0; the rest is fp32.
 *   spp_gat_aggregate_backward: from grad_z: grad_a_src [S] (caller zeroes it), grad_a_dst [T], and -- when
 *                              grad_x_dev != NULL (caller zeroes it) -- grad_x[j,:] += alpha_ij grad_z_i.
 *   spp_gat_logits_backward:   grad_v_src[c] = sum_j grad_a_src[j] x[j,c], grad_v_dst[c] = sum_{i<T} grad_a_dst[i] x[i,c].
 * Each of these (and spp_gat_aggregate_backward_gather below) is the heads = 1 spelling of its spp_gat_mh_* entry:
 * the same implementation, checks and kernels with the head count fixed at 1, so a_src, a_dst, row_max, row_sum and
 * grad_a_* are plain float arrays (4-byte aligned); z, grad_z, v_*, grad_x and the workspace are 16-byte aligned. */
spp_status spp_gat_logits(const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t num_sources,
                          int64_t num_targets, int64_t K, const float* v_src_dev, const float* v_dst_dev,
                          float* a_src_dev, float* a_dst_dev, void* stream);
spp_status spp_gat_logits_backward(const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t num_sources,
                                   int64_t num_targets, int64_t K, const float* grad_a_src_dev,
                                   const float* grad_a_dst_dev, float* grad_v_src_dev, float* grad_v_dst_dev,
                                   void* stream);
spp_status spp_gat_aggregate_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                     const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t K,
                                     const float* a_src_dev, const float* a_dst_dev, float negative_slope,
                                     float* z_dev, float* row_max_dev, float* row_sum_dev, void* stream);
spp_status spp_gat_aggregate_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                      const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t K,
                                      const float* a_src_dev, const float* a_dst_dev, float negative_slope,
                                      const float* z_dev, const float* row_max_dev, const float* row_sum_dev,
                                      const float* grad_z_dev, float* grad_x_dev, float* grad_a_src_dev,
                                      float* grad_a_dst_dev, void* stream);

/* spp_gat_aggregate_backward with the input gradient by GATHER over the transposed hop (built on the fly: count,
 * scan, fill) instead of E x K fp32 atomics: grad_x_dev [S, K] fp32 is written COMPLETELY, including the rank-1
 * terms of the logits -- grad_a_src[s] v_src for every source and grad_a_dst[s] v_dst for the first T -- that
 * the atomic form leaves to the caller (a_src = x v_src, a_dst = x[:T] v_dst).  grad_a_src_dev [S] is zeroed by the
 * caller as before.  workspace_dev: spp_gat_aggregate_backward_gather_workspace_bytes(T, S, E) bytes, 16-byte aligned
 * (= spp_gat_mh_aggregate_backward_gather_workspace_bytes(T, S, E, 1)).  The heads = 1 spelling of
 * spp_gat_mh_aggregate_backward_gather. */
int64_t spp_gat_aggregate_backward_gather_workspace_bytes(int64_t num_targets, int64_t num_sources, int64_t num_edges);
spp_status spp_gat_aggregate_backward_gather(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                             int64_t num_sources, int64_t num_edges, const void* x_dev,
                                             int32_t x_is_half, int64_t x_stride_elems, int64_t K,
                                             const float* a_src_dev, const float* a_dst_dev, float negative_slope,
                                             const float* z_dev, const float* row_max_dev, const float* row_sum_dev,
                                             const float* grad_z_dev, const float* v_src_dev, const float* v_dst_dev,
                                             float* grad_x_dev, float* grad_a_src_dev, float* grad_a_dst_dev,
                                             void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Multi-head GATConv (PyG's `heads` = H in {1, 2, 4, 8}) in the same aggregate-then-project form, per head.
 * W [H*C, K] holds H blocks W_h of C rows; V_src[h,:] = W_h^T att_src[h], V_dst[h,:] = W_h^T att_dst[h]. Layouts,
 * all fp32 and row-major: V_src, V_dst [H, K]; a_src [S, H]; a_dst [T, H]; z, grad_z [T, H, K]; row_max, row_sum
 * [T, H]; grad_a_src [S, H]; grad_a_dst [T, H]; grad_x [S, K].  x rows: element code x_elem (0 fp32, 1 fp16, 2 bf16),
 * K % 4 == 0, K <= 1024, rows aligned to 4 elements, as above.  z, grad_z, V, grad_x and the workspace are 16-byte
 * aligned; the per-head arrays (a_src, a_dst, row_max, row_sum, grad_a_src, grad_a_dst) are read and written H floats
 * at a time and need 4 * min(H, 4) bytes: 4 at H = 1, 8 at H = 2, 16 at H = 4 and 8.  Every entry checks the head
 * count, x_elem and K first, then the sizes (an empty hop returns SPP_OK here), then the buffers.  A head count outside {1, 2, 4, 8}, an unknown x_elem or a bad K returns SPP_ERR_INVALID before
 * anything is launched (the workspace query returns SPP_ERR_INVALID for a bad head count).  Each source row is read
 * once per edge for all H heads.
 *   spp_gat_mh_logits:           a_src[j,h] = x_j . V_src[h] (all S rows), a_dst[i,h] = x_i . V_dst[h] (the first T)
 *   spp_gat_mh_aggregate_forward: z[i,h,:] = sum_j softmax_j(leaky_relu(a_src[j,h] + a_dst[i,h])) x_j over row i
 *                                (diagonal entry dropped, self loop added); head h's output is z[:,h,:] @ W_h^T.  Per head
 *                                the result equals spp_gat_aggregate_forward's on a_src[:,h], a_dst[:,h].
 *   spp_gat_mh_aggregate_backward: from grad_z: grad_a_src (caller zeroes it), grad_a_dst, and -- when grad_x_dev !=
 *                                NULL (caller zeroes it) -- grad_x[j,:] += sum_h alpha_ij^h grad_z[i,h,:] (one fp32
 *                                atomic per column and edge; the rank-1 logit terms are left to the caller).
 *   spp_gat_mh_aggregate_backward_gather: the same with grad_x [S, K] written COMPLETELY by gather over the transposed
 *                                hop, including sum_h grad_a_src[s,h] V_src[h] and, for s < T, sum_h grad_a_dst[s,h]
 *                                V_dst[h].  workspace: spp_gat_mh_aggregate_backward_gather_workspace_bytes bytes.
 *   spp_gat_mh_logits_backward:  grad_V_src[h,c] = sum_j grad_a_src[j,h] x[j,c], grad_V_dst[h,c] = sum_{i<T}
 *                                grad_a_dst[i,h] x[i,c]  (both [H, K], zeroed here). */
spp_status spp_gat_mh_logits(const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t num_sources,
                             int64_t num_targets, int64_t K, int32_t heads, const float* v_src_dev,
                             const float* v_dst_dev, float* a_src_dev, float* a_dst_dev, void* stream);
spp_status spp_gat_mh_logits_backward(const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t num_sources,
                                      int64_t num_targets, int64_t K, int32_t heads, const float* grad_a_src_dev,
                                      const float* grad_a_dst_dev, float* grad_v_src_dev, float* grad_v_dst_dev,
                                      void* stream);
spp_status spp_gat_mh_aggregate_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                        const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K,
                                        int32_t heads, const float* a_src_dev, const float* a_dst_dev,
                                        float negative_slope, float* z_dev, float* row_max_dev, float* row_sum_dev,
                                        void* stream);
spp_status spp_gat_mh_aggregate_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                         const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K,
                                         int32_t heads, const float* a_src_dev, const float* a_dst_dev,
                                         float negative_slope, const float* z_dev, const float* row_max_dev,
                                         const float* row_sum_dev, const float* grad_z_dev, float* grad_x_dev,
                                         float* grad_a_src_dev, float* grad_a_dst_dev, void* stream);
int64_t spp_gat_mh_aggregate_backward_gather_workspace_bytes(int64_t num_targets, int64_t num_sources,
                                                             int64_t num_edges, int32_t heads);
spp_status spp_gat_mh_aggregate_backward_gather(const int64_t* rowptr_dev, const int64_t* col_dev,
                                                int64_t num_targets, int64_t num_sources, int64_t num_edges,
                                                const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K,
                                                int32_t heads, const float* a_src_dev, const float* a_dst_dev,
                                                float negative_slope, const float* z_dev, const float* row_max_dev,
                                                const float* row_sum_dev, const float* grad_z_dev,
                                                const float* v_src_dev, const float* v_dst_dev, float* grad_x_dev,
                                                float* grad_a_src_dev, float* grad_a_dst_dev, void* workspace_dev,
                                                int64_t workspace_bytes, void* stream);

/* f3t  ATTENTION DROPOUT: PyG's GATConv(dropout=p), F.dropout(alpha, p, training) on the attention coefficients.  The
 *      three aggregate entries above with (p, training, seed) appended after `stream`; everything else as above.
 *        alpha_ij = softmax_j(leaky_relu(a_src[j,h] + a_dst[i,h]))   over ALL entries: the mask never enters the softmax
 *        q_ij     = keep_ij / (1 - p)        keep in {0, 1} per (entry, head), the self loop included
 *        z[i,h,:] = sum_j q_ij alpha_ij x_j
 *      row_max and row_sum are exactly the values of the entry without dropout.  Backward, with go = g_i . z_i on the
 *      saved (dropped) z and gh = g_i . x_j:  ge = alpha_ij (q_ij gh - go) lrelu'(raw) (a dropped entry still sends
 *      -alpha go to its logits: dL/dalpha_ij = q_ij gh and sum_k alpha_ik q_ik gh_ik = go);  grad_x[j,:] += sum_h q_ij
 *      alpha_ij g_i^h;  the gather form's alpha_e / alpha_self hold q alpha.  Forward and backward take the same (p, seed).
 *   Keep rule (csrc/act_keep.hip.h attn_keep_heads; mix64 = the splitmix64 finaliser, keep_thr = (uint32_t)((1 - p) * 2^32),
 *   2^32 - 1 at p = 0, of spp_relu_dropout_forward), with E = rowptr[T] entries, T targets, H heads:
 *        draw index  i = k * H + h          for CSR entry k (a dropped diagonal entry consumes its index),
 *                    i = (E + t) * H + h    for target t's self loop;
 *        draw(i) = the low (i even) or high (i odd) 32 bits of mix64(seed + (i >> 1) * 0x9E3779B97F4A7C15);
 *        kept iff draw(i) < keep_thr.   One hash serves two heads (at H = 1, two neighbouring entries).
 *   Refusals: those of the entry each extends, in its order, with `0 <= p < 1` checked right after the head count,
 *   x_elem and K (so before the sizes and the buffers; a NaN p is refused).  training = 0 or p = 0 runs the kernels of
 *   the entry without dropout: the same bits.  spp_gat_mh_attn_keep writes the mask keep_dev [(E + T), H] (one byte, 0 / 1,
 *   entry-major: the E CSR entries, then the T self loops) with the device function the kernels call; it refuses
 *   negative sizes, a head count outside {1, 2, 4, 8} and p outside [0, 1), in this order.  SPP_ABI_VERSION stays 6. */
spp_status spp_gat_mh_aggregate_forward_drop(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                             const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K,
                                             int32_t heads, const float* a_src_dev, const float* a_dst_dev,
                                             float negative_slope, float* z_dev, float* row_max_dev,
                                             float* row_sum_dev, void* stream, float p, int32_t training,
                                             uint64_t seed);
spp_status spp_gat_mh_aggregate_backward_drop(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                              const void* x_dev, int32_t x_elem, int64_t x_stride_elems, int64_t K,
                                              int32_t heads, const float* a_src_dev, const float* a_dst_dev,
                                              float negative_slope, const float* z_dev, const float* row_max_dev,
                                              const float* row_sum_dev, const float* grad_z_dev, float* grad_x_dev,
                                              float* grad_a_src_dev, float* grad_a_dst_dev, void* stream, float p,
                                              int32_t training, uint64_t seed);
spp_status spp_gat_mh_aggregate_backward_gather_drop(const int64_t* rowptr_dev, const int64_t* col_dev,
                                                     int64_t num_targets, int64_t num_sources, int64_t num_edges,
                                                     const void* x_dev, int32_t x_elem, int64_t x_stride_elems,
                                                     int64_t K, int32_t heads, const float* a_src_dev,
                                                     const float* a_dst_dev, float negative_slope, const float* z_dev,
                                                     const float* row_max_dev, const float* row_sum_dev,
                                                     const float* grad_z_dev, const float* v_src_dev,
                                                     const float* v_dst_dev, float* grad_x_dev, float* grad_a_src_dev,
                                                     float* grad_a_dst_dev, void* workspace_dev,
                                                     int64_t workspace_bytes, void* stream, float p, int32_t training,
                                                     uint64_t seed);
spp_status spp_gat_mh_attn_keep(int64_t num_edges, int64_t num_targets, int32_t heads, float p, uint64_t seed,
                                uint8_t* keep_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * f3  Sum aggregation of GINConv over one MFG hop (driver/models.py:234-283: GINConv(nn) with PyG's
 *     defaults eps = 0, train_eps = False, aggr='add', on ((x, x_target), adj_t)); fp32 accumulate and output.
 *       forward : out[t,:] = s * x[t,:] + sum_{e in row t} x[col[e],:],  s = 1 + eps passed in; every entry of
 *                 the row counts (duplicates, self edges), an empty row gives s * x[t,:].  The targets are the
 *                 first T rows of x (the MFG contract, `x_target = x[:size[1]]`).  With s == 0 the target's own
 *                 row is not read.  x fp32 or fp16, rows x_stride_elems apart; out rows out_stride_elems apart
 *                 (0 = dense).
 *       backward: grad_x[j,:] = (j < T ? s * grad_out[j,:] : 0) + sum_{e: col[e] = j} grad_out[row e,:]; grad_x
 *                 [S, F] fp32 dense, written completely (fp32 atomics for the scatter: order not fixed).
 * ------------------------------------------------------------------------- */
spp_status spp_csr_sum_forward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                               const void* x_dev, int32_t x_is_half, int64_t x_stride_elems, int64_t F,
                               float self_scale, float* out_dev, int64_t out_stride_elems, void* stream);
/* The same sum straight from the RESIDENT feature table (the TableRows input of a table_features Session, as
 * spp_sage_operand_forward_table): row j of the batch is table[n_id[j]] (fast_sampler.cpp:1004-1016), same rows and
 * summation order as spp_csr_sum_forward over the materialised x.  An id outside [0, table_rows) reads row 0. */
spp_status spp_csr_sum_forward_table(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                     const void* table_dev, int32_t table_is_half, int64_t table_stride_elems,
                                     int64_t table_rows, const int64_t* n_id_dev, int64_t F, float self_scale,
                                     float* out_dev, int64_t out_stride_elems, void* stream);
/* The same sum from ROW REFERENCES (spp_mfg_out.row_addr, as spp_sage_operand_forward_rows; replaces the assembly
 * x = cat(...)[perm] of transferers.py:472-486): row j of the batch is the F elements at row_addr_dev[j]; any F
 * (8-byte aligned fp16 / 16-byte aligned fp32 rows when F % 4 == 0). */
spp_status spp_csr_sum_forward_rows(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                    const int64_t* row_addr_dev, int32_t rows_are_half, int64_t F, float self_scale,
                                    float* out_dev, int64_t out_stride_elems, void* stream);
spp_status spp_csr_sum_backward(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                int64_t num_sources, const float* grad_out_dev, int64_t grad_out_stride_elems,
                                int64_t F, float self_scale, float* grad_x_dev, void* stream);
/* The same gradient by GATHER over the transposed hop (no fp32 atomics), built as for
 * spp_sage_operand_backward_gather: workspace_dev holds spp_sage_operand_backward_workspace_bytes(T, S, E) bytes,
 * 16-byte aligned. */
spp_status spp_csr_sum_backward_gather(const int64_t* rowptr_dev, const int64_t* col_dev, int64_t num_targets,
                                       int64_t num_sources, int64_t num_edges, const float* grad_out_dev,
                                       int64_t grad_out_stride_elems, int64_t F, float self_scale, float* grad_x_dev,
                                       void* workspace_dev, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * f3  Aggregation by descriptor: the mean / operand / sum kernels above with a choice of element types -- among
 *     them bf16 activations and gradients for training under torch.autocast(dtype=torch.bfloat16) -- through two
 *     entries instead of one function per combination.
 *
 *   Element codes (spp_elem): SPP_ELEM_F32 = 0, SPP_ELEM_F16 = 1, SPP_ELEM_BF16 = 2 (SPP_ELEM_FP8_E4M3 = 3: f3c below).  The GAT entries' `x_is_half`
 *   argument is this code too (0 and 1 keep their meaning).
 *   Rounding rule: every load converts to fp32 exactly; every sum and product runs in fp32, in the order of the fp32
 *   kernels; each stored bf16 element is rounded ONCE, to nearest even.  So a bf16 output equals the fp32 output
 *   rounded to bf16 bit for bit, and a bf16 input gives the fp32 result on the input converted to fp32.
 *
 *   spp_agg_forward: `source` SPP_AGG_DENSE (x = the batch's matrix, rows x_stride_elems apart), SPP_AGG_TABLE
 *     (x = the resident table with x_rows rows, batch row j = x[n_id[j]]) or SPP_AGG_ROWS (n_id = the row
 *     addresses of spp_mfg_out.row_addr, x unused); `epilogue`:
 *       SPP_AGG_MEAN         out [T, F]  = the mean (spp_csr_mean_forward);
 *       SPP_AGG_OPERAND      out [T, 2F] = [mean | x_target] (spp_sage_operand_forward, _table, _rows);
 *       SPP_AGG_OPERAND_ACT  the operand of relu_dropout(x) for a PRE-activation x (spp_sage_operand_forward_act:
 *                            DENSE rows with x_stride_elems == F, F % 4 == 0, x fp32 or bf16, p / training / seed);
 *                            the dropout decisions depend on the element index only, so a bf16 x drops the same
 *                            elements as an fp32 x at the same seed;
 *       SPP_AGG_SUM          out [T, F]  = s * x[t] + the sum (spp_csr_sum_forward, _table, _rows), s = self_scale.
 *     x_elem: fp32 / fp16 / bf16; out_elem: fp32 / bf16.  out_stride_elems 0 = dense.
 *
 *   spp_agg_backward: grad_x [S, F] dense is written COMPLETELY (also for SPP_AGG_MEAN, whose old entry adds):
 *       SPP_AGG_MEAN (scatter only)  grad_x[s] = sum over the edges (t, s) of grad_out[t] / deg t;
 *       SPP_AGG_OPERAND              spp_sage_operand_backward / _gather (grad_out [T, 2F]);
 *       SPP_AGG_OPERAND_ACT          the same followed by the ReLU + dropout backward of the pre-activation z [S, F]
 *                                    (spp_sage_operand_backward_gather_act; p / training / seed of the forward);
 *       SPP_AGG_SUM                  spp_csr_sum_backward / _gather.
 *     grad_elem, out_elem, z_elem: fp32 / bf16 each.  form SPP_AGG_GATHER: over the transposed hop, workspace of
 *     spp_sage_operand_backward_workspace_bytes(T, S, E) bytes, fixed summation order.  form SPP_AGG_SCATTER: fp32
 *     atomics into an fp32 buffer (order not fixed), then one pass that applies the activation backward and / or
 *     rounds: with out_elem != fp32 that buffer is the workspace, 4 * S * F bytes; with fp32 it is grad_x itself and
 *     no workspace is needed.  Workspaces are 16-byte aligned.
 *
 *   An unknown source, epilogue, form or element code, or an element type an epilogue does not take, returns
 *   SPP_ERR_INVALID before anything is launched.
 * ------------------------------------------------------------------------- */
enum { SPP_ELEM_F32 = 0, SPP_ELEM_F16 = 1, SPP_ELEM_BF16 = 2, SPP_ELEM_FP8_E4M3 = 3 /* spp_agg_forward_fp8, spp_exchange_cfg.x_elem */ };
enum { SPP_AGG_DENSE = 0, SPP_AGG_TABLE = 1, SPP_AGG_ROWS = 2 };
enum { SPP_AGG_MEAN = 0, SPP_AGG_OPERAND = 1, SPP_AGG_OPERAND_ACT = 2, SPP_AGG_SUM = 3,
       SPP_AGG_MAX = 4, SPP_AGG_MAX_OPERAND = 5 /* spp_graph_agg_forward / _fp8 only (f3g); training: spp_agg_max_forward, f3q */ };
enum { SPP_AGG_SCATTER = 0, SPP_AGG_GATHER = 1 };

typedef struct spp_agg_fwd_desc {
  int32_t source;           /* SPP_AGG_DENSE / _TABLE / _ROWS */
  int32_t epilogue;         /* SPP_AGG_MEAN / _OPERAND / _OPERAND_ACT / _SUM */
  int32_t x_elem;           /* spp_elem of x's rows */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_targets;
  const void* x_dev;        /* DENSE: the batch's matrix; TABLE: the feature table; ROWS: unused */
  int64_t x_stride_elems;   /* DENSE / TABLE */
  int64_t x_rows;           /* TABLE: the table's rows */
  const int64_t* n_id_dev;  /* TABLE: the batch's node ids; ROWS: the row addresses */
  int64_t F;
  void* out_dev;
  int64_t out_stride_elems; /* 0 = dense */
  float self_scale;         /* SUM: s = 1 + eps */
  float p;                  /* OPERAND_ACT: dropout probability, 0 <= p < 1 */
  int32_t training;         /* OPERAND_ACT */
  int32_t reserved;
  uint64_t seed;            /* OPERAND_ACT */
} spp_agg_fwd_desc;

typedef struct spp_agg_bwd_desc {
  int32_t form;             /* SPP_AGG_SCATTER / SPP_AGG_GATHER */
  int32_t epilogue;         /* SPP_AGG_MEAN (scatter) / _OPERAND / _OPERAND_ACT / _SUM */
  int32_t grad_elem;        /* grad_out: SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t out_elem;         /* grad_x:   SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t z_elem;           /* z (OPERAND_ACT): SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t reserved;
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_targets;
  int64_t num_sources;
  int64_t num_edges;
  const void* grad_out_dev;
  int64_t grad_out_stride_elems; /* 0 = dense (F, or 2F for the operand) */
  int64_t F;
  void* grad_x_dev;         /* [S, F] dense */
  const void* z_dev;        /* OPERAND_ACT: the pre-activation [S, F], dense */
  float self_scale;         /* SUM */
  float p;                  /* OPERAND_ACT */
  int32_t training;         /* OPERAND_ACT */
  int32_t reserved2;
  uint64_t seed;            /* OPERAND_ACT */
} spp_agg_bwd_desc;

spp_status spp_agg_forward(const spp_agg_fwd_desc* desc, void* stream);
spp_status spp_agg_backward(const spp_agg_bwd_desc* desc, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * f3c  fp8 feature table (opt-in): one byte per element, OCP e4m3 (the encoding of torch.float8_e4m3fn, converted by
 *      gfx950's v_cvt_pk_f32_fp8), with one power-of-two exponent per feature COLUMN.
 *        q          e4m3 [rows, F], row-major, rows exactly F bytes apart, F % 16 == 0, base 16-byte aligned
 *        scale_log2 int8 [F], every entry in [-64, 63]
 *      The dequantised value is  v[i, c] = float32(q[i, c]) * 2^scale_log2[c]  -- exact in fp32.  A consumer of fp16
 *      gets v rounded ONCE, to nearest even.
 *
 *   spp_gather_rows_fp8: dst[j, :] = fp16(v[idx[j], :]) for j < n; dst fp16 [n, F] dense, 16-byte aligned; idx int64.
 *     An index outside [0, src_rows) reads row 0 and raises SPP_AERR_GATHER_INDEX (as spp_gather_rows).
 *   spp_agg_forward_fp8: spp_agg_forward with x_elem = SPP_ELEM_FP8_E4M3 (x_stride_elems in elements = bytes) and
 *     source SPP_AGG_DENSE or SPP_AGG_TABLE, epilogue SPP_AGG_MEAN / _OPERAND / _SUM: every load returns v, everything
 *     after the load is the fp32 kernel's code, so the result equals spp_agg_forward's on the fp32 matrix v bit for bit.
 *     Needs F % 4 == 0 and 4-byte aligned rows.  Anything else returns SPP_ERR_INVALID before a launch.
 * ------------------------------------------------------------------------- */
spp_status spp_gather_rows_fp8(const void* q_dev, int64_t src_rows, int64_t F, const int8_t* scale_log2_dev,
                               const int64_t* idx_dev, int64_t n, void* dst_dev, void* stream);
spp_status spp_agg_forward_fp8(const spp_agg_fwd_desc* desc, const int8_t* scale_log2_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * f3g  Aggregation over rows of the RESIDENT graph (exact, layer-wise inference): the mean / operand / sum of
 *      spp_agg_forward for targets that are ANY nodes of the graph, each with its whole neighbour row.
 *
 *        rowptr, col   the graph's CSR, int64: node t's neighbours are col[rowptr[t] .. rowptr[t+1]), global node ids
 *        x             one row per graph node, [x_rows, F], rows x_stride_elems apart; fp32 / fp16 / bf16
 *        targets       a slab  (target_row0 >= 0, target_ids_dev NULL):  output row i is node target_row0 + i
 *                      or a list (target_ids_dev int64 [num_targets], target_row0 < 0): output row i is node
 *                      target_ids[i]; any order, duplicates allowed
 *        epilogue      SPP_AGG_MEAN, SPP_AGG_OPERAND ([mean | x[target]]) or SPP_AGG_SUM (self_scale * x[target] + sum),
 *                      with the meaning and the rounding rule of spp_agg_forward; out_elem fp32 / bf16
 *
 *   Summation contract, C = spp_graph_agg_chunk() (a compile-time constant, >= 32):
 *     a row of d <= C entries is summed in CSR order, one addend at a time, in fp32, and the mean is
 *       sum * (1.0f / max(d, 1)): bit-identical to spp_agg_forward on the same row;
 *     a longer row is cut into consecutive chunks of C entries (the last may be shorter); each chunk is summed in CSR
 *       order in fp32 from zero, and the chunk sums are added in chunk order in fp32;
 *     the result of a row depends on nothing else -- not the grid, the slab, or the other rows of the call -- and no
 *       atomic touches the output.
 *
 *   The maximum (f3q): epilogue SPP_AGG_MAX gives out [T, F] = the element-wise maximum over the row, SPP_AGG_MAX_OPERAND
 *     [T, 2F] = [max | x[target]], by the comparison rule of spp_agg_max_forward: the best starts as the row's first entry,
 *     a later entry replaces it only if !(v <= best) and the best is no NaN; an empty row gives 0.  A long row's chunk
 *     maxima are combined by the same rule in chunk order.  Nothing is rounded before the store, so the result equals
 *     spp_agg_max_forward's on the same row bit for bit for EVERY row length.  spp_graph_agg_forward and
 *     spp_graph_agg_forward_fp8 take these two values; the entries over parts (f3j) refuse them.
 *
 *   Ids that leave the graph: a col entry outside [0, x_rows) reads row 0 (the rule of SPP_AGG_TABLE: no fault, no
 *   error); a target id outside [0, x_rows) gives an output row of zeros.  A slab that leaves [0, x_rows] is refused.
 *   Workspace: spp_graph_agg_workspace_bytes(num_targets) bytes, 16-byte aligned, the caller's; its contents mean nothing
 *   between calls.  The entry enqueues a 16-byte memset and two launches on `stream` and never waits for the device.
 *   With F % 4 == 0 and rows of x aligned to 4 elements the kernels move four columns per lane, and the output must be
 *   aligned to 4 elements too (base and stride); other rows of x are read one column per lane, with the same result.
 *   Refused with SPP_ERR_INVALID before anything is enqueued: both target forms or neither, a slab outside the graph,
 *   SPP_AGG_OPERAND_ACT or an unknown epilogue, an unknown element code, fp8 rows, such a misaligned output, a missing,
 *   misaligned or too small workspace.  (The row sources SPP_AGG_TABLE / SPP_AGG_ROWS do not exist here: x IS the table.)
 * ------------------------------------------------------------------------- */
typedef struct spp_graph_agg_desc {
  int32_t epilogue;         /* SPP_AGG_MEAN / _OPERAND / _SUM / _MAX / _MAX_OPERAND */
  int32_t x_elem;           /* SPP_ELEM_F32 / _F16 / _BF16 (SPP_ELEM_FP8_E4M3: spp_graph_agg_forward_fp8 only, f3o) */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t reserved;
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  const void* x_dev;
  int64_t x_stride_elems;
  int64_t x_rows;           /* the graph's nodes = the rows of x */
  int64_t F;
  int64_t target_row0;      /* slab: the first target; < 0 with a list */
  const int64_t* target_ids_dev; /* list: the targets; NULL with a slab */
  int64_t num_targets;
  void* out_dev;            /* [num_targets, F or 2F] */
  int64_t out_stride_elems; /* 0 = dense */
  float self_scale;         /* SUM: s = 1 + eps */
  int32_t reserved2;
} spp_graph_agg_desc;

int64_t spp_graph_agg_chunk(void);
int64_t spp_graph_agg_workspace_bytes(int64_t num_targets);
spp_status spp_graph_agg_forward(const spp_graph_agg_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                 void* stream);

/* ------------------------------------------------------------------------- *
 * f3j  The same aggregation over a ROW-PARTITIONED source: x is not one matrix but num_parts row ranges, each in an
 *      allocation of its own -- the ranks' partitions of the feature table or of a layer's activations, the peers' ones
 *      mapped into this process with spp_ipc_open (or plain device pointers of in-process ranks).
 *
 *        num_parts        P, 1 .. SPP_GRAPH_AGG_MAX_PARTS
 *        part_offsets     P + 1 entries (host, in the descriptor), non-decreasing, part_offsets[0] == 0: part p holds the
 *                         global rows [part_offsets[p], part_offsets[p + 1]); x_rows = part_offsets[P]
 *        x_parts_dev[p]   the address, in this process, of part p's FIRST row; NULL allowed exactly for an empty part
 *        x_stride_elems   one row stride for all parts
 *      rowptr, col (the whole graph's CSR, global ids), the targets (a slab or a list of GLOBAL ids), the epilogue, the
 *      element codes, F, the output and self_scale: as spp_graph_agg_desc.  The entry reads x_rows + 1 entries of rowptr.
 *
 *   The summation contract of spp_graph_agg_forward holds word for word, and the result is bit-identical to that entry on
 *   the concatenation of the parts.  A col entry outside [0, x_rows) reads global row 0, the first row of the first
 *   non-empty part; a target id outside gives a row of zeros; the target's own row (SPP_AGG_OPERAND, the self term of
 *   SPP_AGG_SUM) is read through the parts as well.  The vector form (four columns per lane) needs F % 4 == 0,
 *   x_stride_elems % 4 == 0 and EVERY non-empty part's base aligned to 4 elements; otherwise the rows are read one column
 *   per lane, with the same result.  An output misaligned for the vector form is refused, as there.  Workspace, stream
 *   and launches: as spp_graph_agg_forward.  The entry maps nothing and enables no peer access: every base must already
 *   be readable from the stream's device.
 *   Refused with SPP_ERR_INVALID before anything is enqueued: num_parts out of range, part_offsets[0] != 0 or decreasing
 *   offsets, a NULL base of a non-empty part, fp8 rows, and everything spp_graph_agg_forward refuses.
 * ------------------------------------------------------------------------- */
#define SPP_GRAPH_AGG_MAX_PARTS 16
typedef struct spp_graph_agg_parts_desc {
  int32_t epilogue;         /* SPP_AGG_MEAN / _OPERAND / _SUM */
  int32_t x_elem;           /* SPP_ELEM_F32 / _F16 / _BF16 (SPP_ELEM_FP8_E4M3: spp_graph_agg_parts_forward_fp8 only, f3o) */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t num_parts;        /* P */
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t part_offsets[SPP_GRAPH_AGG_MAX_PARTS + 1];
  const void* x_parts_dev[SPP_GRAPH_AGG_MAX_PARTS];
  int64_t x_stride_elems;
  int64_t F;
  int64_t target_row0;      /* slab: the first target (a global id); < 0 with a list */
  const int64_t* target_ids_dev; /* list: the targets (global ids); NULL with a slab */
  int64_t num_targets;
  void* out_dev;            /* [num_targets, F or 2F] */
  int64_t out_stride_elems; /* 0 = dense */
  float self_scale;         /* SUM: s = 1 + eps */
  int32_t reserved;
} spp_graph_agg_parts_desc;

spp_status spp_graph_agg_parts_forward(const spp_graph_agg_parts_desc* desc, void* workspace_dev,
                                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * f3o  Exact inference that reads an fp8 feature table (f3c: q e4m3 [rows, F], scale_log2 int8 [F]) IN PLACE.  Opt-in,
 *      beside the entries above, which keep refusing SPP_ELEM_FP8_E4M3: nothing the existing entries do changes.
 *
 *   spp_graph_agg_forward_fp8: spp_graph_agg_forward over the rows of q.  The descriptor is spp_graph_agg_desc with
 *     x_elem == SPP_ELEM_FP8_E4M3, x_dev = q and x_stride_elems in elements = BYTES; scale_log2_dev: the F column
 *     exponents on the device, 4-byte aligned.  Every load returns v[i, c] = float32(q[i, c]) * 2^scale_log2[c] (exact,
 *     for every exponent in [-64, 63]) and everything behind the load is the code of the fp32 rows, so the result is
 *     spp_graph_agg_forward's on the fp32 matrix v BIT FOR BIT: the summation contract, the epilogues, the target's own
 *     row (the right half of SPP_AGG_OPERAND, the self term of SPP_AGG_SUM), the rules for ids outside the graph, the
 *     workspace and the launches are that entry's.  A lane takes one dword, four columns: always the vector form, so
 *     out_dev must be aligned to 4 elements (base and stride).  A NaN code (0x7f, 0xff) gives a NaN; its payload is
 *     not part of the contract.
 *     Refused with SPP_ERR_INVALID before anything is enqueued: any other x_elem, F % 16 != 0, fp8 as out_elem, a NULL or
 *     not 4-byte aligned scale_log2_dev, a base or a row stride that is no multiple of 4 bytes, and everything
 *     spp_graph_agg_forward refuses.
 *   spp_graph_agg_parts_forward_fp8: the same over a ROW-PARTITIONED q, as spp_graph_agg_parts_forward: the descriptor is
 *     spp_graph_agg_parts_desc with x_elem == SPP_ELEM_FP8_E4M3 and the stride in bytes.  ONE exponent vector serves all
 *     parts: that the owners of the parts quantised against the same exponents is the caller's duty, as on the exchange
 *     path (spp_exchange_cfg.scales_tag).  Bit-identical to spp_graph_agg_forward_fp8 on the concatenation of the parts.
 *   spp_fp8_rows_f32: rows of the table as dense fp32, dst[j, :] = v[row(j), :] for j < n, dst fp32 [n, F] -- the exact
 *     values, nothing rounded: the tiles the GEMMs of exact inference take from an fp8 table.  The rows are a slab
 *     (row0 >= 0, ids_dev NULL: row(j) = row0 + j, which must stay inside [0, src_rows]) or a list (ids_dev int64 [n],
 *     row0 < 0: any order, duplicates allowed); an id outside [0, src_rows) reads row 0 and raises SPP_AERR_GATHER_INDEX
 *     (as spp_gather_rows_fp8).  q and dst 16-byte aligned, scale_log2_dev 4-byte aligned, F % 16 == 0; anything else
 *     returns SPP_ERR_INVALID before a launch.  n == 0 or F == 0: nothing is enqueued.
 * ------------------------------------------------------------------------- */
spp_status spp_graph_agg_forward_fp8(const spp_graph_agg_desc* desc, const int8_t* scale_log2_dev, void* workspace_dev,
                                     int64_t workspace_bytes, void* stream);
spp_status spp_graph_agg_parts_forward_fp8(const spp_graph_agg_parts_desc* desc, const int8_t* scale_log2_dev,
                                           void* workspace_dev, int64_t workspace_bytes, void* stream);
spp_status spp_fp8_rows_f32(const void* q_dev, int64_t src_rows, int64_t F, const int8_t* scale_log2_dev, int64_t row0,
                            const int64_t* ids_dev, int64_t n, void* dst_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * f3h  GATConv attention over rows of the RESIDENT graph (exact, layer-wise GAT inference), in PyG's project-first
 *      order: the rows are already projected, h = x W^T, and the logits already taken from them.
 *
 *        rowptr, col   the graph's CSR, int64, global node ids (as spp_graph_agg_forward)
 *        h             one projected row per graph node, [x_rows, F], rows x_stride_elems apart; fp32 / fp16 / bf16;
 *                      F = heads * C, head k owns columns k*C .. (k+1)*C
 *        a_src, a_dst  fp32 [x_rows, heads], dense: a_src[n,k] = h[n,k,:] . att_src[k], a_dst likewise
 *        targets       a slab or a list, exactly as spp_graph_agg_desc
 *
 *      For target t and head k (GATConv with add_self_loops, as spp_gat_aggregate_forward states it): the entries are
 *      col[rowptr[t] .. rowptr[t+1]) with every entry j == t skipped, plus one self loop j = t;
 *        e_j = leaky_relu(a_src[j,k] + a_dst[t,k], negative_slope),  alpha = softmax_j(e),
 *        out[i, k*C + c] = sum_j alpha_j h[j, k*C + c],  then max(., 0) if relu != 0;  out_elem fp32 / bf16, a bf16
 *      output is rounded once, to nearest even.  A node without neighbours gets its own row.  Logits and softmax state
 *      are fp32.  Any heads >= 1 that divides F.
 *
 *   Softmax contract, C_g = spp_graph_gat_chunk() (a compile-time constant, >= 32).  A state is (m, s, acc): the
 *   maximum logit so far, the denominator and the weighted sum of rows, both at that maximum.  Taking an entry with
 *   logit e and row v:  if e > m: r = __expf(m - e), acc *= r, s *= r, m = e;  then w = __expf(e - m), s += w,
 *   acc = fma(w, v, acc).  The result of a state is acc / s.
 *     a row of at most C_g raw entries (skipped ones count): ONE state, begun as the self loop's (m = e_t, s = 1,
 *       acc = h[t]), takes the row's entries in CSR order;
 *     a longer row is cut into consecutive chunks of C_g raw positions (the last may be shorter).  Chunk 0 begins as
 *       the self loop's state, every other chunk as the empty state (m = -inf, s = 0, acc = 0); each takes its entries
 *       in CSR order.  The running state is chunk 0's, and chunks 1, 2, ... are merged into it in chunk order:
 *         m' = max(m1, m2), f1 = __expf(m1 - m'), f2 = __expf(m2 - m'), s' = fma(s2, f2, s1 * f1),
 *         acc' = fma(f2, acc2, acc1 * f1);
 *     a chunk whose entries are all skipped stays the empty state; merging it changes nothing (f2 = 0, f1 = 1) and
 *       produces no NaN: the running state is always finite, because it begins with the self loop;
 *     the result of a row depends on nothing else -- not the grid, the slab, the order of a list or the other rows of
 *       the call -- and no atomic touches the output.
 *
 *   Ids that leave the graph: a col entry outside [0, x_rows) is node 0 in every respect (its row of h, its logit, and
 *   the comparison with t); a target id outside [0, x_rows) gives an output row of zeros.  Neither faults.
 *   Workspace: spp_graph_gat_workspace_bytes(num_targets) bytes, 16-byte aligned, the caller's; its contents mean
 *   nothing between calls.  The entry enqueues a 16-byte memset and two launches on `stream` and never waits for the
 *   device.  With C % 4 == 0 and rows of h aligned to 4 elements the kernels move four columns per lane, and the output
 *   must be aligned to 4 elements too (base and stride); other rows are read one column per lane, with the same rule.
 *   Refused with SPP_ERR_INVALID before anything is enqueued: a NULL descriptor, both target forms or neither, a slab
 *   outside the graph, heads < 1 or F % heads != 0, an unknown or fp8 element code, such a misaligned output, a
 *   missing, misaligned or too small workspace, a stride smaller than the row.  num_targets == 0 or F == 0: SPP_OK.
 * ------------------------------------------------------------------------- */
typedef struct spp_graph_gat_desc {
  int32_t x_elem;           /* h: SPP_ELEM_F32 / _F16 / _BF16 */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t heads;
  int32_t relu;             /* != 0: out = max(out, 0) */
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  const void* x_dev;        /* h */
  int64_t x_stride_elems;
  int64_t x_rows;           /* the graph's nodes = the rows of h, a_src and a_dst */
  int64_t F;                /* heads * C */
  const float* a_src_dev;   /* [x_rows, heads] */
  const float* a_dst_dev;   /* [x_rows, heads] */
  int64_t target_row0;      /* slab: the first target; < 0 with a list */
  const int64_t* target_ids_dev; /* list: the targets; NULL with a slab */
  int64_t num_targets;
  void* out_dev;            /* [num_targets, F] */
  int64_t out_stride_elems; /* 0 = dense */
  float negative_slope;
  int32_t reserved;
} spp_graph_gat_desc;

int64_t spp_graph_gat_chunk(void);
int64_t spp_graph_gat_workspace_bytes(int64_t num_targets);
spp_status spp_graph_gat_forward(const spp_graph_gat_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                 void* stream);

/* ------------------------------------------------------------------------- *
 * f3k  The same attention over a ROW-PARTITIONED h: the projected rows and their logits are not one matrix each but
 *      num_parts row ranges, each in allocations of its own -- the ranks' parts of a layer's h and logits, the peers'
 *      ones mapped into this process with spp_ipc_open (or plain device pointers of in-process ranks).
 *
 *        num_parts        P, 1 .. SPP_GRAPH_AGG_MAX_PARTS
 *        part_offsets     P + 1 entries (host, in the descriptor), non-decreasing, part_offsets[0] == 0: part p holds the
 *                         global rows [part_offsets[p], part_offsets[p + 1]); x_rows = part_offsets[P]
 *        h_parts_dev[p]   the address, in this process, of part p's FIRST projected row; NULL exactly for an empty part
 *        x_stride_elems   one row stride of h for all parts
 *        a_parts_dev[p]   part p's logits as ONE fp32 matrix [rows_p, 2 * heads]: a_src in columns [0, heads), a_dst in
 *                         [heads, 2 * heads) -- the product of the layer's input rows with [V_src; V_dst]^T as it comes
 *                         out of one GEMM; NULL exactly for an empty part
 *        a_stride_elems   one row stride of the logits for all parts; 0 = dense (2 * heads)
 *      rowptr, col (the whole graph's CSR, global ids), the targets (a slab or a list of GLOBAL ids), heads, relu,
 *      negative_slope, the element codes, F and the output: as spp_graph_gat_desc.  The entry reads x_rows + 1 entries
 *      of rowptr.
 *
 *   The softmax contract of spp_graph_gat_forward holds word for word, and the result is bit-identical to that entry on
 *   the concatenation of the parts (h, and a_src / a_dst as the two halves of the concatenated logits).  A col entry
 *   outside [0, x_rows) is global node 0 in every respect (its row of h, its logit, and the comparison with t): the
 *   first row of the first non-empty part.  A target id outside [0, x_rows) gives a row of zeros.  The target's own row
 *   and both of its logits are read through the parts as well.  One owner lookup per entry serves the row of h and the
 *   logit.  The vector form (four columns of one head per lane) needs C % 4 == 0, x_stride_elems % 4 == 0 and EVERY
 *   non-empty part's h base aligned to 4 elements; otherwise the rows are read one column per lane, with the same
 *   result.  An output misaligned for the vector form is refused, as there.  Workspace
 *   (spp_graph_gat_workspace_bytes), stream and launches (a 16-byte memset and two): as spp_graph_gat_forward.  The
 *   entry maps nothing and enables no peer access: every base must already be readable from the stream's device.
 *   Refused with SPP_ERR_INVALID before anything is enqueued: num_parts out of range, part_offsets[0] != 0 or
 *   decreasing offsets, a NULL h or logits base of a non-empty part, a negative a_stride_elems or a non-zero one below
 *   2 * heads, and everything spp_graph_gat_forward refuses.  num_targets == 0 or F == 0: SPP_OK.
 * ------------------------------------------------------------------------- */
typedef struct spp_graph_gat_parts_desc {
  int32_t x_elem;           /* h: SPP_ELEM_F32 / _F16 / _BF16 */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t heads;
  int32_t relu;             /* != 0: out = max(out, 0) */
  int32_t num_parts;        /* P */
  int32_t reserved;
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t part_offsets[SPP_GRAPH_AGG_MAX_PARTS + 1];
  const void* h_parts_dev[SPP_GRAPH_AGG_MAX_PARTS];
  const float* a_parts_dev[SPP_GRAPH_AGG_MAX_PARTS];   /* [rows_p, 2 * heads] = [a_src | a_dst] */
  int64_t x_stride_elems;
  int64_t a_stride_elems;   /* 0 = dense (2 * heads) */
  int64_t F;                /* heads * C */
  int64_t target_row0;      /* slab: the first target (a global id); < 0 with a list */
  const int64_t* target_ids_dev; /* list: the targets (global ids); NULL with a slab */
  int64_t num_targets;
  void* out_dev;            /* [num_targets, F] */
  int64_t out_stride_elems; /* 0 = dense */
  float negative_slope;
  int32_t reserved2;
} spp_graph_gat_parts_desc;

spp_status spp_graph_gat_parts_forward(const spp_graph_gat_parts_desc* desc, void* workspace_dev,
                                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * f3i  The layer tail of SAGEResInception in eval mode (exact, layer-wise inference): leaky_relu(BatchNorm(z)) plus
 *      the residual, one pass over the rows of a GEMM tile, written straight into a slab of the next activation matrix.
 *
 *   Arithmetic contract, all in fp32, for i < n and c < C:
 *        y        = fma(a[c], z[i,c], b[c])                    (one fma)
 *        y        = y >= 0 ? y : negative_slope * y
 *        out[i,c] = round_once(y + r[row(i), c])               (no residual: round_once(y))
 *      a, b are fp32 [C]: the caller folds BatchNorm's running statistics into them, a = gamma / sqrt(var + eps),
 *      b = beta - mean * a.  Nothing else enters an element.  round_once: fp32 as it is, bf16 to nearest even.
 *
 *        z    [n, C], rows z_stride_elems apart; fp32 / bf16
 *        r    the residual, [r_rows, C], rows r_stride_elems apart; fp32 / fp16 / bf16; NULL = no residual (r_elem,
 *             r_rows and r_stride_elems are then not read).  Addressed as a slab, row(i) = r_row0 + i (r_row0 >= 0,
 *             r_ids_dev NULL), or by a list, row(i) = r_ids[i] (int64 [n], any order, duplicates allowed, r_row0 < 0):
 *             the target convention of spp_graph_agg_desc.  A row index outside [0, r_rows) gives an OUTPUT row of
 *             zeros, without a fault (the target rule of the graph kernels).
 *        out  [n, C], rows out_stride_elems apart; fp32 / bf16
 *      A stride of 0 means dense (C).  out must not overlap z or r rows that other rows of the call still read.
 *
 *   One launch on `stream`, no workspace, no atomics; the entry never waits for the device.  The vector form moves
 *   W = 4 columns per lane when any of z, r, out is fp32 and W = 8 when all are 16-bit (the widest operand in 16-byte
 *   pieces); it applies when C and the three row strides are multiples of W, the three bases are aligned to W
 *   elements and a, b to 16 bytes.  Anything else runs one column per lane, with the same result.
 *   Refused with SPP_ERR_INVALID before anything is enqueued: a NULL descriptor; NULL z_dev, out_dev, a_dev or b_dev;
 *   an unknown element code (fp16 z or out, fp8 anywhere); C < 1; negative n, strides or r_rows; a non-zero stride
 *   smaller than C; both a slab and a list; a residual with neither; a residual of no rows with n > 0.
 *   n == 0: SPP_OK, nothing launched.
 * ------------------------------------------------------------------------- */
typedef struct spp_resinc_epilogue_desc {
  int32_t z_elem;            /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t r_elem;            /* SPP_ELEM_F32 / _F16 / _BF16 (with r_dev) */
  int32_t out_elem;          /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  float negative_slope;
  const void* z_dev;
  int64_t z_stride_elems;    /* 0 = dense */
  const float* a_dev;        /* [C] */
  const float* b_dev;        /* [C] */
  const void* r_dev;         /* NULL: no residual */
  int64_t r_stride_elems;    /* 0 = dense */
  int64_t r_rows;
  int64_t r_row0;            /* slab: the residual row of output row 0; < 0 with a list */
  const int64_t* r_ids_dev;  /* list: the residual row of every output row; NULL with a slab */
  int64_t n;
  int64_t C;
  void* out_dev;
  int64_t out_stride_elems;  /* 0 = dense */
} spp_resinc_epilogue_desc;

spp_status spp_resinc_epilogue(const spp_resinc_epilogue_desc* desc, void* stream);

/* ------------------------------------------------------------------------- *
 * f3m  The tail all models' exact inference shares: the predicted class and the negative log-likelihood of every row
 *      of a tile of logits, one pass, so that no [rows, classes] matrix of log-probabilities has to exist.
 *
 *   Contract, for i < n, everything in fp32 after an exact upcast of bf16:
 *        pred[i] = the index of the largest z[i,c] by torch.argmax's rules: the smallest index on ties, a NaN is larger
 *                  than everything and the first NaN wins.  Exact: the argmax of the LOGITS.
 *        m       = max_c z[i,c]
 *        nll[i]  = log(sum_c exp(z[i,c] - m)) - (z[i,y] - m),  y = the row's label; 0.0f when the row has none
 *      exp(t) is 2^(t * log2(e)) (one rounded product, the device's 2^x), log the device library's logf; the last bit
 *      is therefore not torch's.  |nll - exact| <= (C + 8) * 2^-24 * (1 + |z_y - m| + log C).
 *
 *        z     [n, C], rows z_stride_elems apart (0 = dense); fp32 / bf16
 *        y     int64 [y_rows], NULL = no labels (y_rows, y_row0 and row_ids_dev then select nothing).  Addressed as
 *              spp_resinc_epilogue's residual: a slab, row i reads y[y_row0 + i] (y_row0 >= 0, row_ids_dev NULL), or a
 *              list, row i reads y[row_ids[i]] (int64 [n], any order, duplicates allowed, y_row0 < 0).  An index
 *              outside [0, y_rows) is "no label", without a fault; so is a label outside [0, C) (-1 for an
 *              unlabelled node).
 *        pred  int64 [n], NULL = not wanted;  nll  fp32 [n], NULL = not wanted;  at least one of the two.
 *
 *   A row's pred and nll are a function of its C logits, its label, C and the element type ONLY -- not of n, the row's
 *   position in the call, the stride, the alignment or the load form -- and the same bits run to run: lpr lanes (a power
 *   of two <= 64, fixed by C and the type) own a row, column c belongs to lane (c / W) % lpr with W = 4 (fp32) or 8
 *   (bf16), a lane folds its columns in ascending order and the lanes' partial results meet in an xor-shuffle tree that
 *   carries the index through the maximum.  Loads move 16 bytes where the base, the stride and C are multiples of W
 *   elements, 8 or 4 bytes or one element otherwise; a row of more than 64 * W columns is walked twice (maximum, then sum).
 *   One launch on `stream`, no workspace, no atomics; the entry never waits for the device.
 *   Refused with SPP_ERR_INVALID before anything is enqueued: a NULL descriptor; NULL z_dev; pred_dev and nll_dev both
 *   NULL; an unknown element code (fp16, fp8); C outside [1, 2^31); negative n, stride or y_rows; a non-zero stride
 *   smaller than C; both a slab and a list; labels with neither.  n == 0: SPP_OK, nothing launched.
 * ------------------------------------------------------------------------- */
typedef struct spp_classify_desc {
  int32_t z_elem;              /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t reserved;
  const void* z_dev;
  int64_t z_stride_elems;      /* 0 = dense */
  int64_t n;
  int64_t C;
  const int64_t* y_dev;        /* NULL: no labels */
  int64_t y_rows;
  int64_t y_row0;              /* slab: the label row of output row 0; < 0 with a list */
  const int64_t* row_ids_dev;  /* list: the label row of every output row; NULL with a slab */
  int64_t* pred_dev;           /* NULL: not wanted */
  float* nll_dev;              /* NULL: not wanted */
} spp_classify_desc;

spp_status spp_classify_rows(const spp_classify_desc* desc, void* stream);

/* ------------------------------------------------------------------------- *
 * f3n  The receptive field of a few nodes: what touches the resident graph's rows when the nodes within h hops of
 *      `nodes` are numbered and their rows copied into a compact CSR that the f3g kernels run on unchanged.
 *
 *      The field's nodes carry SLOTS: depth 0 is the distinct ids of `nodes`, depth d every neighbour of a node of depth
 *      d-1 that has no smaller depth; slots count depth by depth, in ascending id order within a depth.  The caller keeps
 *        slot   int32 [num_nodes], -1 = not in the field
 *        flag   one byte per node, all 0 between hops
 *      and numbers a depth between the two entries (compact the flags into the ascending list of new ids, scatter their
 *      slots, clear the flags); no atomic decides a slot.
 *
 *   spp_field_mark: flag[j] = 1 for every entry j of the row of every frontier node ids[i], i < num_ids, that lies in
 *     [0, num_nodes) and has slot[j] < 0.  Plain byte stores; every writer of a flag stores the same value, so the result
 *     is the same from run to run.  Reads slot, writes flag only.
 *   spp_field_rows: for i < num_ids, fcol[frowptr[i] + k] = slot[col[rowptr[ids[i]] + k]] for every k of the node's row:
 *     the WHOLE row in CSR order, every entry replaced by its slot (multi-edges and self-loops stay, the degree is
 *     unchanged).  frowptr int64 [num_ids + 1] is the prefix sum of those degrees, fcol int64 [fcol_len].  An entry
 *     outside [0, num_nodes) or without a slot is written as -1 (a correctly built field has none).  If frowptr gives a
 *     row less room than its degree, or leaves [0, fcol_len], the copy is cut to what fits: nothing is written outside
 *     [frowptr[i], frowptr[i + 1]) or outside fcol.
 *
 *   An id outside [0, num_nodes) is an empty row in both entries: no fault, no error.  Load balance as f3g: lane groups
 *   finish the rows of at most C_f = spp_field_chunk() entries, a longer row's index goes to a list in the workspace and a
 *   second launch gives each listed row a workgroup.  Every offset is 64-bit.  Workspace: spp_field_workspace_bytes(num_ids)
 *   bytes, 16-byte aligned, the caller's; its contents mean nothing between calls.  Each entry enqueues a 16-byte memset and
 *   two launches on `stream` and never waits for the device.
 *   Refused with SPP_ERR_INVALID before anything is enqueued: a NULL descriptor; a negative num_nodes, num_ids or
 *   fcol_len; a missing, misaligned or too small workspace; and, unless num_ids == 0 (SPP_OK, nothing enqueued), a NULL
 *   rowptr, col, ids or slot, an empty graph, a NULL flag (mark), a NULL frowptr or a NULL fcol with fcol_len > 0 (rows).
 * ------------------------------------------------------------------------- */
typedef struct spp_field_desc {
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_nodes;          /* N: the graph's nodes */
  const int64_t* ids_dev;     /* mark: the frontier; rows: the field's rows by slot.  int64 [num_ids], global ids */
  int64_t num_ids;
  const int32_t* slot_dev;    /* int32 [num_nodes], -1 = not in the field */
  uint8_t* flag_dev;          /* mark: [num_nodes] bytes; unused by rows */
  const int64_t* frowptr_dev; /* rows: int64 [num_ids + 1]; unused by mark */
  int64_t* fcol_dev;          /* rows: int64 [fcol_len] */
  int64_t fcol_len;           /* rows: frowptr[num_ids]; 0 for mark */
} spp_field_desc;

int64_t spp_field_chunk(void);
int64_t spp_field_workspace_bytes(int64_t num_ids);
spp_status spp_field_mark(const spp_field_desc* desc, void* workspace_dev, int64_t workspace_bytes, void* stream);
spp_status spp_field_rows(const spp_field_desc* desc, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * f3p  The TRAINING form of the layer tail that follows a GEMM in GIN and SAGEResInception:
 *      y = dropout(act(BatchNorm(z))) [+ r], on batch statistics, forward and backward (f3i is its eval-only, forward-only
 *      relative on folded running statistics).
 *
 *   z, r, y are [n, C], row-major and dense, fp32 or bf16 each on its own; C >= 1 is any value.  A bf16 value is read as
 *   its fp32 value, every per-element operation is fp32 and a bf16 output is rounded once, to nearest even.  gamma, beta,
 *   the running statistics, mean, invstd, dgamma and dbeta are fp32 [C].
 *
 *   spp_bn_act_forward, training != 0 (n >= 2):
 *        mean[c]   = the mean, var[c] the BIASED variance of column c over the n rows
 *        invstd[c] = 1 / sqrt(var[c] + eps)
 *        u         = gamma[c] * (z[i,c] - mean[c]) * invstd[c] + beta[c]      of the fp32 operands, rounded once: the
 *                    rounding errors of the fp32 operations are recovered (two-sums, fma residuals) and added back
 *                    before the last rounding, so u is within about half an ulp of the exact expression
 *        a         = u (SPP_BN_ACT_NONE) | u > 0 ? u : 0 (SPP_BN_ACT_RELU) | u > 0 ? u : negative_slope * u (_LEAKY_RELU)
 *        y[i,c]    = round_once((keep(i*C + c) ? a * (1 / (1 - p)) : 0) + r[i,c])          (p == 0: a itself; no r: no add)
 *      keep(e) is the generator of spp_relu_dropout_forward over a dense array of n*C elements at the same (seed, p):
 *      an array of n*C positive values passed through that entry keeps exactly the same elements.
 *      mean and invstd are written (backward reads them), and the running buffers are updated as torch.nn.BatchNorm1d
 *      does, with f = momentum, or f = 1 / *num_batches_tracked_dev when momentum < 0 (the cumulative average; the
 *      CALLER has already counted this batch):
 *        running_mean = (1 - f) * running_mean + f * mean
 *        running_var  = (1 - f) * running_var  + f * var * n / (n - 1)                     (the UNBIASED variance)
 *      running_mean_dev / running_var_dev may both be NULL in training (nothing is tracked).
 *      Statistics: z is read once, no float atomics.  The rows are cut into slabs of SPP_BN_ACT_SLAB_ROWS, one workgroup
 *      per slab folds its rows into per-column (mean, M2) by Welford's update, and a second kernel combines the slabs in
 *      a fixed order by Chan's update (in fp64) and writes mean, invstd and the running buffers: the same bits from call
 *      to call on the same input.
 *   spp_bn_act_forward, training == 0: no statistics pass and no dropout (p and seed are not read); mean = running_mean,
 *      invstd = 1 / sqrt(running_var + eps), both written to mean_dev / invstd_dev; the running buffers are only read.
 *
 *   spp_bn_act_backward reads g (the gradient of y, [n, C], g_elem), z, mean, invstd, gamma, beta and the seed -- neither
 *   y nor a mask: the sign of u and keep(e) are recomputed, by the forward's own expressions.
 *        xh        = (z[i,c] - mean[c]) * invstd[c]                        (two fp32 operations)
 *        g_a       = g[i,c] * (keep ? 1 / (1 - p) : 0) * act'(u)          act'(u) = 1 for u > 0, else 0 / negative_slope
 *        dbeta[c]  = sum_i g_a        dgamma[c] = sum_i g_a * xh          (slab partials, combined in a fixed order in fp64)
 *        dz[i,c]   = round_once(gamma * invstd * (g_a - dbeta / n - xh * dgamma / n))      training
 *        dz[i,c]   = round_once(gamma * invstd * g_a)                                     training == 0
 *      dz has z's element type.  The gradient of r is g itself: no kernel runs for it.
 *
 *   The 16-byte vector form (4 columns per lane) applies when C % 4 == 0 and every matrix base is aligned to 4 of its
 *   elements, a workgroup-uniform choice; anything else runs one column per lane with the same result.
 *   Workspace: spp_bn_act_workspace_bytes(n, C) bytes, 16-byte aligned, the caller's; its contents mean nothing between
 *   calls.  The entries enqueue their launches on `stream` and never wait for the device.
 *   Refused with SPP_ERR_INVALID before anything is enqueued, in a message that names the entry: a NULL descriptor;
 *   n < 2 in training ("more than 1 value per channel"), negative n; C outside [1, 2^31); p outside [0, 1); an unknown
 *   act or element code (fp16, fp8); a NULL required pointer (z, gamma, beta, mean, invstd; y forward; g, dz, dgamma,
 *   dbeta backward; the running buffers in eval; num_batches_tracked_dev with momentum < 0 and running buffers); a
 *   missing, misaligned or too small workspace.  n == 0 in eval: SPP_OK, nothing enqueued, nothing written.
 * ------------------------------------------------------------------------- */
#define SPP_BN_ACT_SLAB_ROWS 32
enum { SPP_BN_ACT_NONE = 0, SPP_BN_ACT_RELU = 1, SPP_BN_ACT_LEAKY_RELU = 2 };

typedef struct spp_bn_act_desc {
  int32_t z_elem;            /* SPP_ELEM_F32 / SPP_ELEM_BF16; dz has the same */
  int32_t r_elem;            /* forward, with r_dev */
  int32_t y_elem;            /* forward */
  int32_t g_elem;            /* backward */
  int32_t act;               /* SPP_BN_ACT_* */
  int32_t training;
  float negative_slope;
  float p;                   /* dropout probability, [0, 1); training only */
  float eps;
  int32_t reserved;
  double momentum;           /* < 0: the cumulative average, 1 / *num_batches_tracked_dev */
  uint64_t seed;
  int64_t n;
  int64_t C;
  const void* z_dev;
  const float* gamma_dev;
  const float* beta_dev;
  float* running_mean_dev;   /* training: updated (NULL with running_var_dev: not tracked); eval: read */
  float* running_var_dev;
  const int64_t* num_batches_tracked_dev; /* read when momentum < 0; already counts this batch */
  const void* r_dev;         /* forward: the residual, NULL = none */
  void* y_dev;               /* forward: out */
  float* mean_dev;           /* forward: out; backward: in */
  float* invstd_dev;         /* forward: out; backward: in */
  const void* g_dev;         /* backward: the gradient of y */
  void* dz_dev;              /* backward: out */
  float* dgamma_dev;         /* backward: out */
  float* dbeta_dev;          /* backward: out */
  void* workspace_dev;
  int64_t workspace_bytes;
} spp_bn_act_desc;

int64_t spp_bn_act_slab_rows(void);
int64_t spp_bn_act_workspace_bytes(int64_t n, int64_t C);
spp_status spp_bn_act_forward(const spp_bn_act_desc* desc, void* stream);
spp_status spp_bn_act_backward(const spp_bn_act_desc* desc, void* stream);

/* ------------------------------------------------------------------------- *
 * f3q  MAX aggregation over an MFG hop's CSR: the message passing of SAGEConv(aggr="max"), forward and backward, with
 *      descriptors of its own (spp_agg_forward / spp_agg_backward accept what they accepted).
 *
 *   spp_agg_max_forward, for every target t < T and column c < F:
 *        out[t,c] = max over k in [rowptr[t], rowptr[t+1]) of x_row(col[k])[c]
 *        arg[t,c] = col[k*] as int32 (the batch-local source row), k* the FIRST entry in CSR order that attains out[t,c]
 *      an empty row gives out = 0 and arg = -1 (the fill of PyG's scatter-max).
 *      Comparison rule (the one of spp_classify_rows): the best starts as the row's FIRST entry -- not 0, not -FLT_MAX --
 *      and a later entry v replaces it only if !(v <= best) and best is not a NaN.  So the first NaN wins and stays (as
 *      torch.amax propagates it), otherwise the first strict maximum wins, and -0.0 and +0.0 tie: the earlier one stays.
 *      No arithmetic touches a value, so the result does not depend on how a row is cut or in which order its pieces
 *      are combined by the same rule in CSR order: it is the bits of one of the row's entries.
 *      Row sources: `source` SPP_AGG_DENSE / _TABLE / _ROWS with x_dev, x_stride_elems, x_rows and n_id_dev exactly as
 *      in spp_agg_fwd_desc, the rule that a TABLE id outside [0, x_rows) reads row 0 included (arg still names the batch
 *      row).  x_elem fp32 / fp16 / bf16, or SPP_ELEM_FP8_E4M3 (DENSE / TABLE) with the per-column exponents
 *      scale_log2_dev (f3c; a load returns the exact v, and the maximum is taken over v).  out_elem fp32 / bf16; a bf16
 *      output rounds each stored element once (an fp16 / bf16 / e4m3 input's maximum is unchanged by it only where it
 *      fits).  concat_target != 0: out is [T, 2F] = [max | x_target], x_target = batch row t, as SPP_AGG_OPERAND.
 *      arg_dev: int32 [T, F] dense, or NULL (inference, no gradient): then no argmax is written, out is the same.
 *      The vector form (four columns per lane) runs when F % 4 == 0 and x's rows, out's rows and arg are aligned to 4
 *      elements (fp8: exponents to 4 bytes); anything else runs one column per lane with the same result.  Lanes as in
 *      the mean's kernel: LPR lanes share a target, two independent rows are in flight.
 *
 *   spp_agg_max_backward: grad_x [S, F] dense is written COMPLETELY: zero, then grad_x[arg[t,c], c] += g[t,c] for every
 *      arg[t,c] >= 0 by fp32 atomics (T * F of them, not E * F; an arg outside [0, S) is skipped), and with concat_target
 *      (g is [T, 2F]) rows t < T start from g[t, F + c] instead of zero.  grad_elem, out_elem fp32 / bf16.  The atomics
 *      run in an fp32 buffer: grad_x itself when out_elem is fp32, else the workspace (4 * S * F bytes, 16-byte
 *      aligned), rounded once into grad_x by a last pass.
 *
 *   Refused with SPP_ERR_INVALID before anything is enqueued, in a message that names the entry: a NULL descriptor; an
 *   unknown source or element code; fp8 rows with SPP_AGG_ROWS or without exponents; negative T, F or S, S < T, T * F
 *   or S * F beyond 2^62, S beyond 2^31 (arg is int32); a stride smaller than its row; a NULL required pointer (rowptr,
 *   col, out, x or n_id as the source needs; arg, grad_out, grad_x backward); an out, arg, grad or workspace pointer not
 *   aligned to its element; a missing or too small workspace.  T == 0 or F == 0: SPP_OK (backward still zeroes grad_x).
 * ------------------------------------------------------------------------- */
typedef struct spp_agg_max_fwd_desc {
  int32_t source;           /* SPP_AGG_DENSE / _TABLE / _ROWS */
  int32_t x_elem;           /* spp_elem of x's rows, SPP_ELEM_FP8_E4M3 included */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t concat_target;    /* != 0: out is [T, 2F] = [max | x_target] */
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_targets;
  const void* x_dev;        /* DENSE: the batch's matrix; TABLE: the feature table; ROWS: unused */
  int64_t x_stride_elems;   /* DENSE / TABLE */
  int64_t x_rows;           /* TABLE: the table's rows */
  const int64_t* n_id_dev;  /* TABLE: the batch's node ids; ROWS: the row addresses */
  const int8_t* scale_log2_dev; /* fp8 rows: int8 [F] */
  int64_t F;
  void* out_dev;
  int64_t out_stride_elems; /* 0 = dense */
  int32_t* arg_dev;         /* int32 [T, F] dense, or NULL */
} spp_agg_max_fwd_desc;

typedef struct spp_agg_max_bwd_desc {
  int32_t grad_elem;        /* grad_out: SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t out_elem;         /* grad_x:   SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t concat_target;    /* != 0: grad_out is [T, 2F] */
  int32_t reserved;
  const int32_t* arg_dev;   /* int32 [T, F] dense: the forward's */
  int64_t num_targets;
  int64_t num_sources;
  const void* grad_out_dev;
  int64_t grad_out_stride_elems; /* 0 = dense (F, or 2F with concat_target) */
  int64_t F;
  void* grad_x_dev;         /* [S, F] dense */
  void* workspace_dev;      /* out_elem != fp32: 4 * S * F bytes */
  int64_t workspace_bytes;
} spp_agg_max_bwd_desc;

spp_status spp_agg_max_forward(const spp_agg_max_fwd_desc* desc, void* stream);
spp_status spp_agg_max_backward(const spp_agg_max_bwd_desc* desc, void* stream);

/* ------------------------------------------------------------------------- *
 * f3r  EDGE-WEIGHTED sum aggregation over an MFG hop's CSR, one fp32 weight per entry: the message passing of GCNConv
 *      and of any layer with importance-sampling, precomputed or learned edge weights.  Forward, input gradient, weight
 *      gradient and PyG's gcn_norm, with descriptors of their own (spp_agg_forward / spp_agg_backward accept what they
 *      accepted; SPP_ABI_VERSION stays 6).
 *
 *   spp_agg_weighted_forward, for every target t < T and column c < F:
 *        acc = 0
 *        for k in [rowptr[t], rowptr[t+1]), in CSR order, one entry at a time:  acc = fmaf(w[k], x_row(col[k])[c], acc)
 *        if self_w_dev != NULL:                                                 acc = fmaf(self_w[t], x_row(t)[c], acc)
 *        out[t,c] = acc                                   (an empty row without a self term gives 0)
 *      Summation rule: exactly this fmaf chain in fp32, the self term LAST (as SPP_AGG_SUM's), so a row's result depends
 *      on the row alone -- not on the grid, the other rows of the call, or how the kernel pairs the entries it loads.
 *      Row sources: `source` SPP_AGG_DENSE / _TABLE / _ROWS with x_dev, x_stride_elems, x_rows and n_id_dev exactly as in
 *      spp_agg_max_fwd_desc; a TABLE id outside [0, x_rows) reads row 0.  x_elem fp32 / fp16 / bf16 (read exactly).
 *      SPP_ELEM_FP8_E4M3 rows are REFUSED.  w_dev fp32 [E] and self_w_dev fp32 [T] (may be NULL), 4-byte aligned.
 *      out_elem fp32 / bf16, each stored element rounded once; out_stride_elems 0 = dense.  There is no operand
 *      ([sum | x_target]) form.  The vector form (four columns per lane) runs when F % 4 == 0 and x's and out's rows are
 *      aligned to 4 elements; anything else runs one column per lane with the same result.
 *
 *   spp_agg_weighted_backward writes grad_x [S, F] dense COMPLETELY:
 *        grad_x[s,c] = sum over the entries k = (t, s) of w[k] * g[t,c]  +  (s < T and self_w ? self_w[s] * g[s,c] : 0)
 *      as a gather over the transposed hop with edge ids, built in the workspace (count, scan, fill): one fp32 fmaf chain
 *      per element, the self term last, no atomic on an accumulator.  The order of a source's entries in the chain is
 *      the order the fill pass left them in, which is not fixed between runs.  g fp32 / bf16, grad_x fp32 / bf16
 *      (rounded once); vector and scalar forms as in the forward.  Workspace: 16-byte aligned,
 *      spp_agg_weighted_backward_workspace_bytes(T, S, E) bytes (-1 for sizes the entry refuses).
 *
 *   spp_agg_weighted_wgrad: the gradient of the weights, one dot product per entry, fp32:
 *        grad_w[k]      = sum_c g[t,c] * x_row(col[k])[c]     for k in row t
 *        grad_self_w[t] = sum_c g[t,c] * x_row(t)[c]          (only when grad_self_w_dev != NULL)
 *      Row sources and x_elem as in the forward; g fp32 / bf16.  The lanes of a target keep their columns of g[t,:] in
 *      registers over the row's entries, accumulate their columns in fp32 by fmaf in column order and reduce in a fixed
 *      butterfly; one lane stores.  No atomics, no LDS: the result is the same bits in every run.
 *
 *   spp_gcn_norm: PyG's gcn_norm of the hop padded to [S, S] (its first T rows are the hop, the others are empty):
 *        deg[i]  = fill + sum of row i's w  (w = 1 when w_dev is NULL) for i < T, = fill otherwise
 *        dinv    = 1.0f / sqrtf(deg), 0 where that is inf
 *        coef[k] = dinv[t] * w[k] * dinv[col[k]]          self_coef[t] = fill * dinv[t]^2
 *      fill 1, 2 (`improved`) or 0 (no self loops).  Two passes: dinv over the targets into dinv_dev (fp32 [T], the
 *      caller's: a workspace, or an output to keep), then the coefficients.  A source col[k] >= T has dinv = fill^-1/2
 *      (0 for fill 0) without a read.  With T == S == N this is PyG's normalisation of the whole graph.
 *      self_coef_dev may be NULL.
 *
 *   Refused with SPP_ERR_INVALID before anything is enqueued, in a message that names the entry: a NULL descriptor; an
 *   unknown source, element code or fill; fp8 rows; negative T, F, S or E, S < T, T * F or S * F beyond 2^62, S or E
 *   beyond 2^31 (backward); a stride smaller than its row; a NULL required pointer (SPP_AGG_ROWS without n_id_dev,
 *   SPP_AGG_TABLE without ids or rows included); a pointer not aligned to its element; a missing, misaligned or too small
 *   workspace (backward; gcn_norm: dinv_dev).  T == 0 or F == 0: SPP_OK (backward: S == 0 or F == 0; wgrad with F == 0
 *   writes zeros).
 * ------------------------------------------------------------------------- */
typedef struct spp_agg_weighted_fwd_desc {
  int32_t source;           /* SPP_AGG_DENSE / _TABLE / _ROWS */
  int32_t x_elem;           /* SPP_ELEM_F32 / _F16 / _BF16 */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t reserved;
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_targets;
  int64_t num_edges;
  const void* x_dev;        /* DENSE: the batch's matrix; TABLE: the feature table; ROWS: unused */
  int64_t x_stride_elems;   /* DENSE / TABLE */
  int64_t x_rows;           /* TABLE: the table's rows */
  const int64_t* n_id_dev;  /* TABLE: the batch's node ids; ROWS: the row addresses */
  int64_t F;
  const float* w_dev;       /* fp32 [E] */
  const float* self_w_dev;  /* fp32 [T], or NULL */
  void* out_dev;
  int64_t out_stride_elems; /* 0 = dense */
} spp_agg_weighted_fwd_desc;

typedef struct spp_agg_weighted_bwd_desc {
  int32_t grad_elem;        /* grad_out: SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t out_elem;         /* grad_x:   SPP_ELEM_F32 / SPP_ELEM_BF16 */
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_targets;
  int64_t num_sources;
  int64_t num_edges;
  const void* grad_out_dev;
  int64_t grad_out_stride_elems; /* 0 = dense */
  int64_t F;
  const float* w_dev;       /* fp32 [E] */
  const float* self_w_dev;  /* fp32 [T], or NULL */
  void* grad_x_dev;         /* [S, F] dense */
} spp_agg_weighted_bwd_desc;

typedef struct spp_agg_weighted_wgrad_desc {
  int32_t source;           /* SPP_AGG_DENSE / _TABLE / _ROWS */
  int32_t x_elem;           /* SPP_ELEM_F32 / _F16 / _BF16 */
  int32_t grad_elem;        /* grad_out: SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t reserved;
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_targets;
  int64_t num_edges;
  const void* x_dev;
  int64_t x_stride_elems;
  int64_t x_rows;
  const int64_t* n_id_dev;
  int64_t F;
  const void* grad_out_dev;
  int64_t grad_out_stride_elems; /* 0 = dense */
  float* grad_w_dev;        /* fp32 [E] */
  float* grad_self_w_dev;   /* fp32 [T], or NULL */
} spp_agg_weighted_wgrad_desc;

typedef struct spp_gcn_norm_desc {
  int32_t fill;             /* 1; 2 = improved; 0 = no self loops */
  int32_t reserved;
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_targets;
  int64_t num_sources;
  int64_t num_edges;
  const float* w_dev;       /* fp32 [E], or NULL: ones */
  float* dinv_dev;          /* fp32 [T]: the first pass's result */
  float* coef_dev;          /* fp32 [E] */
  float* self_coef_dev;     /* fp32 [T], or NULL */
} spp_gcn_norm_desc;

spp_status spp_agg_weighted_forward(const spp_agg_weighted_fwd_desc* desc, void* stream);
int64_t spp_agg_weighted_backward_workspace_bytes(int64_t num_targets, int64_t num_sources, int64_t num_edges);
spp_status spp_agg_weighted_backward(const spp_agg_weighted_bwd_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                     void* stream);
spp_status spp_agg_weighted_wgrad(const spp_agg_weighted_wgrad_desc* desc, void* stream);
spp_status spp_gcn_norm(const spp_gcn_norm_desc* desc, void* stream);

/* ------------------------------------------------------------------------- *
 * f3s  EDGE-WEIGHTED sum aggregation over rows of the RESIDENT graph: the weighted member of the f3g family, the message
 *      passing of exact, layer-wise GCN inference.  The graph, x, the targets (a slab or a list) and the output are
 *      spp_graph_agg_desc's, unchanged in meaning; the weights come in one of two forms:
 *
 *        explicit   (dinv_dev NULL)  the weight of entry k is  c_k = w_dev ? w[k] : 1.0f,  and when self_w_dev is given the
 *                   target's own row is added with the weight self_w[t] (fp32 [x_rows], indexed by the GLOBAL node id t)
 *        in-kernel  (dinv_dev given: fp32 [x_rows], spp_gcn_dinv's result)  PyG's gcn_norm formed on the fly,
 *                       c_k    = dinv[t] * (w_dev ? w[k] : 1.f) * dinv[col[k]]
 *                       self_c = dinv[t] * fill * dinv[t]          (fill 0 / 1 / 2 as in spp_gcn_norm; no self term for 0)
 *                   -- the fp32 expressions of spp_gcn_norm, evaluated left to right: the bits of its coef / self_coef
 *                   for the whole graph as one hop (T = S = N), without the fp32 [E] array (12.8 GB at E = 3.2 G).
 *                   fill is read only in this form.  A col[k] outside [0, x_rows) reads dinv[0], as the row source
 *                   reads row 0.
 *
 *   Summation contract, C = spp_graph_agg_chunk() (f3g's constant):
 *     a row of d <= C entries: acc = 0, then acc = fmaf(c_k, x[col[k]], acc) once per entry in CSR order, then the self
 *       term LAST as one more fmaf(self_c, x[t], acc): the arithmetic of spp_agg_weighted_forward, bit-identical to it on
 *       the same row;
 *     a longer row is cut into consecutive chunks of C entries (the last may be shorter); each chunk is such an fmaf chain
 *       from zero, the chunk sums are added in chunk order in fp32, and the self term is one fmaf on the total;
 *     a target id outside [0, x_rows) gives a row of zeros; the result of a row depends on nothing else -- not the grid,
 *       the slab, or the other rows of the call; a bf16 output rounds each stored element once; no atomic touches the
 *       output.
 *
 *   Load balance, workspace (spp_graph_agg_workspace_bytes(num_targets), 16-byte aligned), the vector and scalar forms
 *   and what is enqueued (a 16-byte memset and two launches, no wait): as spp_graph_agg_forward.  Per entry the kernels
 *   stream 8 bytes of col and 4 bytes of w, or gather 4 bytes of dinv, next to the F * sizeof(x_elem) bytes of the row.
 *   Refused with SPP_ERR_INVALID before anything is enqueued: everything spp_graph_agg_forward refuses (fp8 rows among
 *   it: there is no _fp8 form), dinv_dev together with self_w_dev, fill outside 0..2 with dinv_dev, and w_dev, dinv_dev
 *   or self_w_dev not 4-byte aligned.  Not built: a row-partitioned x, fp8 tables, weights in the receptive-field entries.
 *
 *   spp_gcn_dinv: the first pass of spp_gcn_norm alone, over the num_nodes rows of rowptr:
 *        dinv[t] = 1.0f / sqrtf(fill + sum of row t's w in CSR order), 0 where that is inf; the row LENGTH when w_dev is NULL
 *      -- the same kernel, so the bits of the dinv inside spp_gcn_norm -- without the [E] coefficient array.  With weights
 *      one thread walks a whole row, a hub's 10^5 entries included: it runs once per model evaluation and is not tuned.
 *      Refused: a NULL descriptor, fill outside 0..2, a negative or out-of-range num_nodes, NULL rowptr_dev or dinv_dev,
 *      w_dev or dinv_dev not 4-byte aligned.  num_nodes == 0: SPP_OK.
 * ------------------------------------------------------------------------- */
typedef struct spp_graph_agg_weighted_desc {
  int32_t x_elem;           /* SPP_ELEM_F32 / _F16 / _BF16 */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t fill;             /* with dinv_dev: 1; 2 = improved; 0 = no self loops */
  int32_t reserved;
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  const void* x_dev;
  int64_t x_stride_elems;
  int64_t x_rows;           /* the graph's nodes = the rows of x */
  int64_t F;
  int64_t target_row0;      /* slab: the first target; < 0 with a list */
  const int64_t* target_ids_dev; /* list: the targets; NULL with a slab */
  int64_t num_targets;
  void* out_dev;            /* [num_targets, F] */
  int64_t out_stride_elems; /* 0 = dense */
  const float* w_dev;       /* fp32, one value per entry of col; NULL: ones */
  const float* dinv_dev;    /* fp32 [x_rows], or NULL */
  const float* self_w_dev;  /* fp32 [x_rows] by global node id, or NULL; not with dinv_dev */
} spp_graph_agg_weighted_desc;

typedef struct spp_gcn_dinv_desc {
  int32_t fill;             /* 1; 2 = improved; 0 = no self loops */
  int32_t reserved;
  const int64_t* rowptr_dev;
  int64_t num_nodes;
  const float* w_dev;       /* fp32, one value per entry, or NULL: ones */
  float* dinv_dev;          /* fp32 [num_nodes] */
} spp_gcn_dinv_desc;

spp_status spp_graph_agg_weighted_forward(const spp_graph_agg_weighted_desc* desc, void* workspace_dev,
                                          int64_t workspace_bytes, void* stream);
spp_status spp_gcn_dinv(const spp_gcn_dinv_desc* desc, void* stream);

/* ------------------------------------------------------------------------- *
 * f3v  GATv2Conv ("dynamic attention", PyG's GATv2Conv) over an MFG hop, on rows the caller has projected:
 *        x_l [S, H, C] = lin_l(x)          x_r [T, H, C] = lin_r(x_target)          D = H * C
 *        e_ij^h     = sum_c att[h,c] * leaky_relu(x_l[j,h,c] + x_r[i,h,c], negative_slope)
 *        alpha^h    = softmax_j(e_ij^h)
 *        out[i,h,:] = sum_j alpha_ij^h * x_l[j,h,:]
 *      Row i runs over its CSR entries with col == i dropped, plus one self loop (i, i) whose message is SOURCE row
 *      x_l[i] (the set_diag convention of the GAT entries); a target with no kept entry returns x_l[i] exactly.
 *      The nonlinearity sits between the projection and att, so the aggregate-then-project form of the GAT entries does
 *      not apply: the logit of every entry is a C-wide dot product per head.
 *
 *   Layouts: x_l [S, D] and x_r [T, D], rows of x_elem (SPP_ELEM_F32 / _F16 / _BF16, one code for both), each with its own
 *   row stride in elements; x_r may alias x_l (share_weights: x_r = x_l[:T]) or not -- neither is assumed.  att [H, C],
 *   out and grad_out [T, D], row_max and row_sum [T, H], grad_x_l [S, D], grad_x_r [T, D], grad_att [H, C]: fp32, dense,
 *   row-major.  Alignment: the rows of x_l / x_r to 4 elements (base and stride); att, out, grad_out, grad_x_l, grad_x_r,
 *   grad_att to 16 bytes; row_max, row_sum to 4; rowptr, col to 8.
 *   Shapes: heads in {1, 2, 4, 8}; C % 4 == 0 and C / 4 A POWER OF TWO (the per-head reduction is an xor butterfly over
 *   aligned lane segments: C = 12, 20, 24, ... are refused, and the caller computes them another way); D <= 1024;
 *   0 <= T <= S.  col may be NULL when the hop has no entries.
 *
 *   spp_gatv2_forward: writes out, row_max (the row's largest logit) and row_sum (sum_j exp(e_ij - row_max)).  One pass
 *      over the row with a running maximum per head, in the order self loop, then CSR order (the order of
 *      spp_gat_mh_aggregate_forward); weights by expf (the library function, not the __expf of the GAT entries: the
 *      model-level comparison of DESIGN section 7 f3v is why).  A lane's four products of a logit, its chunks, and the
 *      butterfly across the head's lanes are added in an order fixed by (H, C), which this header does not spell out:
 *      compare row_max within the rounding of a C-term dot product, not bit for bit.  No atomics: the same bits in every run.
 *   spp_gatv2_backward: reads the forward's out, row_max, row_sum and grad_out (g).  Per head, with
 *      alpha_ij = expf(e_ij - row_max) / row_sum (e recomputed; no [E, H] array), pre = x_l[j,h,c] + x_r[i,h,c] and
 *      d = pre > 0 ? 1 : negative_slope  (so lrelu'(0) = negative_slope):
 *        go = g_i . out_i     gh = g_i . x_l[j]     ge = alpha (gh - go)
 *        grad_x_l[j,h,c] += alpha * g[i,h,c] + ge * att[h,c] * d     fp32 atomics, one per column per entry, on
 *                                                                     buffers the CALLER has zeroed; NULL: not wanted
 *        grad_x_r[i,h,c]  = sum_j ge * att[h,c] * d                   written completely
 *        grad_att[h,c]    = sum_ij ge * leaky_relu(pre)               zeroed by the entry, then one atomic per column
 *                                                                     per workgroup
 *
 *   Refused with SPP_ERR_INVALID before anything is enqueued, checked in this order: a NULL descriptor; heads outside
 *   {1, 2, 4, 8}; an unknown x_elem; C <= 0 or C % 4 != 0; C / 4 not a power of two; D > 1024; T < 0 or S < T;
 *   (backward: a NULL or misaligned grad_att;)  -- T == 0 returns SPP_OK here (the backward after zeroing grad_att) --
 *   a row stride below D or not a multiple of 4; a NULL rowptr, x_l, x_r, att, out, row_max or row_sum; one of them, or
 *   col, misaligned; (backward: a NULL grad_out or grad_x_r; a misaligned grad_out, grad_x_l or grad_x_r).
 *   T > 0 with no entries is a hop like any other.  SPP_ABI_VERSION stays 6.
 * ------------------------------------------------------------------------- */
typedef struct spp_gatv2_desc {
  int32_t heads;              /* H: 1, 2, 4 or 8 */
  int32_t x_elem;             /* x_l and x_r: SPP_ELEM_F32 / _F16 / _BF16 */
  float negative_slope;
  int32_t reserved;
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_targets;        /* T */
  int64_t num_sources;        /* S >= T */
  int64_t C;                  /* channels per head */
  const void* x_l_dev;        /* [S, D] */
  int64_t x_l_stride_elems;
  const void* x_r_dev;        /* [T, D]; may alias x_l_dev */
  int64_t x_r_stride_elems;
  const float* att_dev;       /* fp32 [H, C] */
  float* out_dev;             /* fp32 [T, D]: written by the forward, read by the backward */
  float* row_max_dev;         /* fp32 [T, H]: likewise */
  float* row_sum_dev;         /* fp32 [T, H]: likewise */
  const float* grad_out_dev;  /* backward: fp32 [T, D] */
  float* grad_x_l_dev;        /* backward: fp32 [S, D], zeroed by the caller; NULL: not wanted */
  float* grad_x_r_dev;        /* backward: fp32 [T, D] */
  float* grad_att_dev;        /* backward: fp32 [H, C], zeroed by the entry */
} spp_gatv2_desc;

spp_status spp_gatv2_forward(const spp_gatv2_desc* desc, void* stream);
spp_status spp_gatv2_backward(const spp_gatv2_desc* desc, void* stream);

/* ------------------------------------------------------------------------- *
 * f3w  GATv2Conv attention over rows of the RESIDENT graph (exact, layer-wise GATv2 inference), on rows the caller has
 *      projected.  Forward only.
 *
 *        rowptr, col   the graph's CSR, int64, global node ids (as spp_graph_agg_forward)
 *        x_l, x_r      [x_rows, D] each, D = heads * C, head h in columns h*C .. (h+1)*C; fp32 / fp16 / bf16, one code
 *                      for both, each with its own row stride; BOTH indexed by global node id.  x_r may be the very
 *                      pointer of x_l (share_weights); neither is assumed.
 *        att           fp32 [heads, C], dense
 *        targets       a slab or a list, exactly as spp_graph_gat_desc
 *
 *      For target t and head h (GATv2Conv's convention here, as spp_gatv2_forward states it): the entries are
 *      col[rowptr[t] .. rowptr[t+1]) with every entry j == t skipped, plus one self loop j = t whose message is x_l[t];
 *        e_j = sum_c att[h,c] * leaky_relu(x_l[j,h,c] + x_r[t,h,c], negative_slope),  alpha = softmax_j(e),
 *        out[i,h,:] = sum_j alpha_j x_l[j,h,:],  then max(., 0) if relu != 0;  out_elem fp32 / bf16, a bf16 output is
 *      rounded once, to nearest even.  A node without neighbours gets x_l[t].  Logits and softmax state are fp32.
 *      Shapes, as the training pair: heads in {1, 2, 4, 8}; C % 4 == 0 with C / 4 a power of two; D <= 1024; the rows
 *      of x_l and x_r aligned to 4 elements (base and stride), att to 16 bytes, the output to 4 elements.
 *
 *   Softmax contract, C_g = spp_graph_gatv2_chunk() (a compile-time constant, >= 32).  A state is PER HEAD (m, s, acc):
 *   the maximum logit so far, the denominator and the weighted sum of the head's C columns of x_l, both at that maximum.
 *   Taking an entry with logit e and row v:  if e > m: r = expf(m - e), acc *= r, s *= r, m = e;  then w = expf(e - m),
 *   s += w, acc += w * v.  The result of a state is acc * (1 / s).  expf is the library function, as in
 *   spp_gatv2_forward and for the reason f3v records -- not the __expf of f3h.
 *     a row of at most C_g raw entries (skipped ones count): ONE state, begun as the self loop's (m = e_tt, s = 1,
 *       acc = x_l[t]), takes the row's entries in CSR order;
 *     a longer row is cut into consecutive chunks of C_g raw positions (the last may be shorter).  Chunk 0 begins as
 *       the self loop's state, every other chunk as the empty state (m = -inf, s = 0, acc = 0); each takes its entries
 *       in CSR order.  The running state is chunk 0's, and chunks 1, 2, ... are merged into it in chunk order:
 *         m' = max(m1, m2), f1 = expf(m1 - m'), f2 = expf(m2 - m'), s' = fma(s2, f2, s1 * f1),
 *         acc' = fma(f2, acc2, acc1 * f1);
 *     a chunk whose entries are all skipped stays the empty state; merging it changes nothing (f2 = 0, f1 = 1) and
 *       produces no NaN: the running state is always finite, because it begins with the self loop;
 *     the dot product of a logit is added in an order fixed by (heads, C) -- a lane's four products per 4-column piece,
 *       its pieces of the head, then an xor butterfly over the head's lanes, widest step first -- the same for every
 *       entry, whatever the row's length, its chunk, its lane group, the grid, the slab or the list order;
 *     the result of a row depends on nothing else -- not the grid, the slab, the order of a list or the other rows of
 *       the call -- and no atomic touches the output.  The only atomic is the counter of the long-row list in the
 *       workspace, which the entry zeroes.
 *   For a call whose rows all have at most C_g raw entries, fp32 output and relu == 0, the output is BIT-IDENTICAL to
 *   spp_gatv2_forward's out on the same rows with the hop the whole graph (T = S = x_rows): both run one body
 *   (csrc/gatv2_core.hip.h), written with contraction off and every fused multiply-add spelled fmaf.
 *
 *   Ids that leave the graph: a col entry outside [0, x_rows) is node 0 in every respect (its row of x_l and the
 *   comparison with t); a target id outside [0, x_rows) gives an output row of zeros.  Neither faults.  Every offset is
 *   64-bit.  Workspace: spp_graph_gatv2_workspace_bytes(num_targets) bytes, 16-byte aligned, the caller's; its contents
 *   mean nothing between calls.  The entry enqueues a 16-byte memset and two launches on `stream` and never waits for
 *   the device.
 *   Refused with SPP_ERR_INVALID before anything is enqueued: a NULL descriptor; heads outside {1, 2, 4, 8}; C <= 0 or
 *   C % 4 != 0; C / 4 not a power of two; D > 1024; an unknown or fp8 element code; both target forms or neither; a slab
 *   outside the graph; an output stride smaller than the row; a missing, misaligned or too small workspace; -- here
 *   num_targets == 0 returns SPP_OK -- a NULL buffer; a row stride smaller than the row; rows of x_l / x_r or an output
 *   not aligned to 4 elements (base and stride); att not aligned to 16 bytes.  SPP_ABI_VERSION stays 6.
 * ------------------------------------------------------------------------- */
typedef struct spp_graph_gatv2_desc {
  int32_t x_elem;           /* x_l and x_r: SPP_ELEM_F32 / _F16 / _BF16 */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t heads;            /* 1, 2, 4 or 8 */
  int32_t relu;             /* != 0: out = max(out, 0) */
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  const void* x_l_dev;      /* [x_rows, D] */
  int64_t x_l_stride_elems;
  const void* x_r_dev;      /* [x_rows, D]; may be x_l_dev */
  int64_t x_r_stride_elems;
  int64_t x_rows;           /* the graph's nodes = the rows of x_l and x_r */
  int64_t C;                /* channels per head; D = heads * C */
  const float* att_dev;     /* fp32 [heads, C] */
  int64_t target_row0;      /* slab: the first target; < 0 with a list */
  const int64_t* target_ids_dev; /* list: the targets; NULL with a slab */
  int64_t num_targets;
  void* out_dev;            /* [num_targets, D] */
  int64_t out_stride_elems; /* 0 = dense */
  float negative_slope;
  int32_t reserved;
} spp_graph_gatv2_desc;

int64_t spp_graph_gatv2_chunk(void);
int64_t spp_graph_gatv2_workspace_bytes(int64_t num_targets);
spp_status spp_graph_gatv2_forward(const spp_graph_gatv2_desc* desc, void* workspace_dev, int64_t workspace_bytes,
                                   void* stream);

/* ------------------------------------------------------------------------- *
 * f3x  ATTENTION DROPOUT for GATv2Conv: PyG's GATv2Conv(dropout=p), F.dropout(alpha, p, training) on the attention
 *      coefficients.  The pair of f3v with (p, training, seed) appended after `stream`; the descriptor, the layouts,
 *      the shapes and everything else as f3v states them.
 *        alpha_ij = softmax_j(e_ij)          over ALL entries, exactly as f3v: the mask never enters the softmax
 *        q_ij     = keep_ij / (1 - p)        keep in {0, 1} per (entry, head), the self loop dropped like any other entry
 *        out[i,h,:] = sum_j q_ij alpha_ij x_l[j,h,:]
 *      row_max and row_sum are the values of spp_gatv2_forward on the same inputs, bit for bit.  Backward, with
 *      go = g_i . out_i on the saved (dropped) out and gh = g_i . x_l[j]:
 *        ge = alpha (q gh - go)              a dropped entry still sends -alpha go to its logit: dL/dalpha_ij = q_ij gh
 *                                            and sum_k alpha_ik q_ik gh_ik = go, so this is the softmax gradient (f3t)
 *        grad_x_l[j,h,c] += q alpha g[i,h,c] + ge att[h,c] d,     grad_x_r and grad_att from ge as in f3v.
 *      Forward and backward take the same (p, seed).
 *   Keep rule: f3t's, unchanged, with E = rowptr[T] (read by the kernels), T targets, H heads: draw index i = k * H + h for
 *   CSR entry k (a skipped diagonal entry consumes its index), i = (E + t) * H + h for target t's self loop; draw(i) = the
 *   low (i even) or high (i odd) 32 bits of mix64(seed + (i >> 1) * 0x9E3779B97F4A7C15); kept iff draw(i) < keep_thr.
 *   spp_gat_mh_attn_keep(E, T, H, p, seed, ...) therefore writes the mask these entries apply.
 *   Refusals: those of the entry each extends, in its order, with `0 <= p < 1` checked right after the shape (D <= 1024
 *   and 0 <= T <= S), so before the backward's grad_att, the T == 0 return and the rows; a NaN p is refused.
 *   training = 0 or p = 0 launches the kernels of the entry without dropout: the same bits.  spp_gatv2_desc is untouched;
 *   SPP_ABI_VERSION stays 6.
 * ------------------------------------------------------------------------- */
spp_status spp_gatv2_forward_drop(const spp_gatv2_desc* desc, void* stream, float p, int32_t training, uint64_t seed);
spp_status spp_gatv2_backward_drop(const spp_gatv2_desc* desc, void* stream, float p, int32_t training, uint64_t seed);

/* ------------------------------------------------------------------------- *
 * f3y  TransformerConv (scaled dot-product attention; Shi et al., "Masked Label Prediction"; PyG's TransformerConv)
 *      over an MFG hop, on rows the caller has projected:
 *        q [T, H, C] = lin_query(x_target)     k [S, H, C] = lin_key(x)     v [S, H, C] = lin_value(x)     D = H * C
 *        e_ij^h     = scale * sum_c q[i,h,c] * k[j,h,c]          (scale: fp32, below; the layer passes 1 / sqrt(C))
 *        alpha^h    = softmax_j(e_ij^h)
 *        out[i,h,:] = sum_j alpha_ij^h * v[j,h,:]
 *      Row i runs over ALL its CSR entries, in CSR order: NO self loop is added, diagonal entries (col == i) are kept,
 *      and a repeated entry counts as often as it appears (PyG's TransformerConv; not the set_diag convention of the
 *      GAT and GATv2 entries).
 *      EMPTY ROWS are therefore a real case: a target without entries gets out = 0, row_sum = 0 and row_max = 0 --
 *      defined values -- and in the backward grad_q = 0 and nothing else; no NaN, nothing is divided by zero.
 *
 *   Layouts: q [T, D], k [S, D] and v [S, D] are rows of x_elem (SPP_ELEM_F32 / _F16 / _BF16, one code for the three),
 *   each with its own base pointer and its own row stride in elements: k and v may be the two halves of one [S, 2 D]
 *   matrix (v = k + D, both strides 2 D) or separate matrices; no aliasing is assumed either way.  out and grad_out
 *   [T, D], row_max and row_sum [T, H], grad_q [T, D], grad_k and grad_v [S, D]: fp32, dense, row-major.
 *   Alignment, as f3v: the rows of q / k / v to 4 elements (base and stride); out, grad_out, grad_q, grad_k, grad_v to
 *   16 bytes; row_max, row_sum to 4; rowptr, col to 8.
 *   Shapes, as f3v: heads in {1, 2, 4, 8}; C % 4 == 0 and C / 4 a power of two; D <= 1024; 0 <= T <= S.  col may be
 *   NULL when the hop has no entries.  The inputs are finite.
 *
 *   spp_transformer_forward: writes out, row_max (the row's largest logit) and row_sum (sum_j exp(e_ij - row_max)).
 *      One pass over the row with a running maximum per head, from the empty state, in CSR order; weights by expf (the
 *      library function: DESIGN section 7 f3v records why).  The dot product of a logit is added in ONE order, fixed
 *      by C alone and walked by both entries: the C products q[c] k[c], each rounded, are added pairwise by xor
 *      distance of the column index within the head, in the order 1, 2, then C / 2, C / 4, ..., 4, every addition a
 *      rounded fp32 addition and none fused with a product; then ONE rounded product by scale.  The online softmax is
 *      csrc/gatv2_core.hip.h's State, unchanged (contraction off, its fused multiply-adds spelled fmaf).  No atomics:
 *      the same bits in every run.
 *   spp_transformer_backward: reads the forward's out, row_max, row_sum and grad_out (g).  Per head, with
 *      alpha_ij = expf(e_ij - row_max) / row_sum (e recomputed, THE FORWARD'S BITS: the order above; no [E, H] array):
 *        go = g_i . out_i     gv = g_i . v[j]     ge = alpha (gv - go)
 *        grad_v[j,h,c] += alpha * g[i,h,c]             fp32 atomics, one per column per entry, on a buffer the CALLER
 *                                                      has zeroed; NULL: not wanted
 *        grad_k[j,h,c] += ge * scale * q[i,h,c]        likewise, independently NULL-able
 *        grad_q[i,h,c]  = sum_j ge * scale * k[j,h,c]  written completely, every row, zeros for an empty one
 *
 *   Refused with SPP_ERR_INVALID before anything is enqueued, checked in this order (f3v's where the cases coincide):
 *   a NULL descriptor; heads outside {1, 2, 4, 8}; an unknown x_elem; C <= 0 or C % 4 != 0; C / 4 not a power of two;
 *   D > 1024; T < 0 or S < T;  -- T == 0 returns SPP_OK here, and touches nothing --  a row stride of q, k or v below
 *   D or not a multiple of 4; a NULL rowptr, q, k, v, out, row_max or row_sum (backward: or grad_out or grad_q); one
 *   of them, or col, misaligned (backward: then a misaligned grad_out, grad_q, grad_k or grad_v); a scale that is not
 *   finite or not positive.  spp_last_error names the failing condition.  SPP_ABI_VERSION stays 6.
 *   Not built: edge features (PyG's edge_dim).  Attention dropout is f4a, the entry over the resident graph f3z, both
 *   below.
 * ------------------------------------------------------------------------- */
typedef struct spp_transformer_desc {
  int32_t heads;              /* H: 1, 2, 4 or 8 */
  int32_t x_elem;             /* q, k and v: SPP_ELEM_F32 / _F16 / _BF16 */
  float scale;                /* > 0, finite; the logit is scale * (q . k) */
  int32_t reserved;
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  int64_t num_targets;        /* T */
  int64_t num_sources;        /* S >= T */
  int64_t C;                  /* channels per head */
  const void* q_dev;          /* [T, D] */
  int64_t q_stride_elems;
  const void* k_dev;          /* [S, D] */
  int64_t k_stride_elems;
  const void* v_dev;          /* [S, D]; may be k_dev + D of one [S, 2 D] matrix */
  int64_t v_stride_elems;
  float* out_dev;             /* fp32 [T, D]: written by the forward, read by the backward */
  float* row_max_dev;         /* fp32 [T, H]: likewise */
  float* row_sum_dev;         /* fp32 [T, H]: likewise */
  const float* grad_out_dev;  /* backward: fp32 [T, D] */
  float* grad_q_dev;          /* backward: fp32 [T, D] */
  float* grad_k_dev;          /* backward: fp32 [S, D], zeroed by the caller; NULL: not wanted */
  float* grad_v_dev;          /* backward: fp32 [S, D], zeroed by the caller; NULL: not wanted */
} spp_transformer_desc;

spp_status spp_transformer_forward(const spp_transformer_desc* desc, void* stream);
spp_status spp_transformer_backward(const spp_transformer_desc* desc, void* stream);

/* ------------------------------------------------------------------------- *
 * f3z  TransformerConv attention over rows of the RESIDENT graph (exact, layer-wise GraphTransformer inference), on
 *      rows the caller has projected.  Forward only.
 *
 *        rowptr, col   the graph's CSR, int64, global node ids (as spp_graph_agg_forward)
 *        q, k, v       [x_rows, D] each, D = heads * C, head h in columns h*C .. (h+1)*C; fp32 / fp16 / bf16, one code
 *                      for the three, each with its own base and row stride; ALL indexed by global node id.  k and v
 *                      may be the halves of one [x_rows, 2 D] matrix (v = k + D, both strides 2 D).
 *        skip          NULL, or rows of x_elem [x_rows, D] with their own stride, indexed by global node id (the
 *                      layer's lin_skip(x))
 *        targets       a slab or a list, exactly as spp_graph_gatv2_desc
 *
 *      For target t and head h (f3y's convention): EVERY entry of col[rowptr[t] .. rowptr[t+1]) in CSR order; no self
 *      loop is added, diagonal entries are kept, a repeated entry counts as often as it appears.
 *        e_j = scale * sum_c q[t,h,c] * k[j,h,c],   alpha = softmax_j(e),   r[h,:] = sum_j alpha_j v[j,h,:]
 *      A row without entries has r = 0: decided by s == 0, nothing is divided.  Epilogue, in this order: r = r + skip[t]
 *      if skip is given (one rounded fp32 addition per column); max(r, 0) if relu != 0; one rounding to out_elem
 *      (fp32 / bf16; bf16 to nearest even).  A target id outside [0, x_rows) gives an output row of zeros and NO skip is
 *      added; a col entry outside [0, x_rows) is node 0.  Neither faults.
 *      Shapes, as f3y: heads in {1, 2, 4, 8}; C % 4 == 0 with C / 4 a power of two; D <= 1024; the rows of q / k / v /
 *      skip aligned to 4 elements (base and stride), the output to 4 elements.
 *
 *   Aliasing: skip may alias out when the skip row of target t and output row i are the same addresses (the same element
 *   type, a slab over a [x_rows, D] matrix).  A lane reads its columns of the skip row before it writes them and no other
 *   lane touches them.  q, k and v must not overlap out.
 *
 *   Softmax contract, C_g = spp_graph_transformer_chunk() (a compile-time constant, >= 32): f3w's State, take, merge and
 *   result, weights by expf, with ONE difference: every chunk, chunk 0 included, begins from the empty state
 *   (m = -inf, s = 0, acc = 0).
 *     a row of at most C_g entries: ONE state from the empty state takes the row's entries in CSR order;
 *     a longer row is cut into consecutive chunks of C_g entries (the last may be shorter); each begins empty and takes
 *       its entries in CSR order; the running state is chunk 0's and chunks 1, 2, ... are merged into it in chunk order
 *       (f3w's merge).  Every chunk of such a row holds at least one entry and every entry is taken, so both states of a
 *       merge are finite: two empty states are never merged (that would be expf(-inf + inf)).
 *     the logit's summation tree is f3y's, fixed by C alone; the result of a row depends on nothing else -- not the
 *       grid, the slab, the order of a list or the other rows of the call -- and no atomic touches the output.
 *   For a call whose rows all have at most C_g entries, fp32 output, no skip and relu == 0, the output is BIT-IDENTICAL
 *   to spp_transformer_forward's out with the hop the whole graph (T = S = x_rows): both run one body
 *   (csrc/transformer_core.hip.h).
 *
 *   Workspace: spp_graph_transformer_workspace_bytes(num_targets) bytes, 16-byte aligned, the caller's.  The entry
 *   enqueues a 16-byte memset and two launches on `stream` and never waits for the device.
 *   Refused with SPP_ERR_INVALID before anything is enqueued, in this order: f3w's refusals (a NULL descriptor; heads;
 *   C; C / 4 not a power of two; D > 1024; element codes; both target forms or neither; a slab outside the graph; an
 *   output stride smaller than the row; the workspace; -- here num_targets == 0 returns SPP_OK and touches nothing --
 *   a NULL rowptr, col, q, k, v or out, or x_rows == 0; k_stride_elems smaller than the row; an output not aligned to 4
 *   elements); then a stride of q, v or skip smaller than the row; rows of q / k / v / skip not aligned to 4 elements
 *   (base and stride); last a scale that is not finite or not positive.  SPP_ABI_VERSION stays 6.
 *   Not built: attention dropout, edge features, partitioned or fp8 rows.
 * ------------------------------------------------------------------------- */
typedef struct spp_graph_transformer_desc {
  int32_t x_elem;           /* q, k, v and skip: SPP_ELEM_F32 / _F16 / _BF16 */
  int32_t out_elem;         /* SPP_ELEM_F32 / SPP_ELEM_BF16 */
  int32_t heads;            /* 1, 2, 4 or 8 */
  int32_t relu;             /* != 0: out = max(out, 0), after the skip */
  const int64_t* rowptr_dev;
  const int64_t* col_dev;
  const void* q_dev;        /* [x_rows, D] */
  int64_t q_stride_elems;
  const void* k_dev;        /* [x_rows, D] */
  int64_t k_stride_elems;
  const void* v_dev;        /* [x_rows, D]; may be k_dev + D of one [x_rows, 2 D] matrix */
  int64_t v_stride_elems;
  int64_t x_rows;           /* the graph's nodes = the rows of q, k, v and skip */
  int64_t C;                /* channels per head; D = heads * C */
  int64_t target_row0;      /* slab: the first target; < 0 with a list */
  const int64_t* target_ids_dev; /* list: the targets; NULL with a slab */
  int64_t num_targets;
  void* out_dev;            /* [num_targets, D] */
  int64_t out_stride_elems; /* 0 = dense */
  const void* skip_dev;     /* NULL, or [x_rows, D] rows of x_elem; may alias out_dev (above) */
  int64_t skip_stride_elems;
  float scale;              /* > 0, finite; the logit is scale * (q . k) */
  int32_t reserved;
} spp_graph_transformer_desc;

int64_t spp_graph_transformer_chunk(void);
int64_t spp_graph_transformer_workspace_bytes(int64_t num_targets);
spp_status spp_graph_transformer_forward(const spp_graph_transformer_desc* desc, void* workspace_dev,
                                         int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * f4a  ATTENTION DROPOUT for TransformerConv: PyG's TransformerConv(dropout=p), F.dropout(alpha, p, training) on the
 *      attention coefficients.  The pair of f3y with (p, training, seed) appended after `stream`, exactly as f3x extends
 *      f3v; the descriptor, the layouts, the shapes and everything else as f3y states them.  Per target i and head h,
 *      over ALL CSR entries of row i in CSR order (f3y's convention: no self loop, diagonal entries kept, repeats
 *      counted):
 *        alpha_ij = softmax_j(scale * q_i . k_j)   over ALL entries, exactly as f3y: the mask never enters the softmax
 *        d_ij     = keep_ij / (1 - p)              keep in {0, 1} per (entry, head)
 *        out[i,h,:] = sum_j d_ij alpha_ij v[j,h,:]     computed as acc * (drop_scale / row_sum), drop_scale the fp32
 *                                                      value of 1 / (1 - p), acc taking only the kept entries
 *      row_max and row_sum are the values of spp_transformer_forward on the same inputs, bit for bit.  A row without
 *      entries gives exact zeros (f3y's row_sum == 0 guard); a (target, head) whose every entry is dropped gives exact
 *      zeros in out, with the row_max / row_sum of the p = 0 call.  Backward, with go = g_i . out_i on the saved
 *      (dropped) out, gh = g_i . v_j and d = keep ? drop_scale : 0:
 *        ge = alpha (d gh - go)                    a dropped entry still sends -alpha go to its logit: dL/dalpha_ij = d_ij gh
 *                                                  and sum_k alpha_ik d_ik gh_ik = go, so this is the softmax gradient (f3t)
 *        grad_q[i,h,c]  = sum_j ge * scale * k[j,h,c]
 *        grad_k[j,h,c] += ge * scale * q[i,h,c]
 *        grad_v[j,h,c] += d * alpha * g[i,h,c]
 *      alpha is recomputed from the forward's logit through f3y's summation tree, bit for bit; grad_k and grad_v are
 *      independently NULL-able as in f3y.  Forward and backward take the same (p, seed).
 *   Keep rule: f3t's, unchanged, WITHOUT self-loop draws: draw index i = k * H + h for CSR entry k (its absolute position
 *   in col, so a hop's mask does not depend on which workgroup handles the row); draw(i) = the low (i even) or high
 *   (i odd) 32 bits of mix64(seed + (i >> 1) * 0x9E3779B97F4A7C15); kept iff draw(i) < keep_thr.  The first E * H bytes of
 *   spp_gat_mh_attn_keep(E, T, H, p, seed, ...) are therefore the mask these entries apply.
 *   Refusals: those of the entry each extends, in f3y's order, with `0 <= p < 1` checked right after the shape checks
 *   (through 0 <= T <= S), so before the T == 0 return, the strides, the NULL and alignment checks and scale; a NaN p is
 *   refused, and p is checked with training = 0 too.
 *   training = 0 or p = 0 launches the kernels of the entry without dropout: the same bits.  spp_transformer_desc is
 *   untouched; SPP_ABI_VERSION stays 6.
 *   Not built: dropout in the entry over the resident graph (f3z scores in eval mode).
 * ------------------------------------------------------------------------- */
spp_status spp_transformer_forward_drop(const spp_transformer_desc* desc, void* stream, float p, int32_t training,
                                        uint64_t seed);
spp_status spp_transformer_backward_drop(const spp_transformer_desc* desc, void* stream, float p, int32_t training,
                                         uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* SPP_H */
