/*
 * tsne_hip.h -- C ABI of libtsne_hip, the MI355X-native hot path of
 * tsne-flink (ChristophAl/tsne-flink): brute-force kNN, perplexity-calibrated
 * affinities, and the Barnes-Hut gradient / optimizer loop.
 *
 * The reference exposes this path as Scala object methods over Flink
 * DataSets (TsneHelpers.scala).  Each entry point below replaces exactly one
 * of them; a JNI shim turns the DataSet partition into the
 * flat arrays used here.  Conventions:
 *   - point ids are dense 0..n-1 (the host mirror remaps arbitrary int ids);
 *   - sparse matrices are CSR: row_ptr[n+1] (int64), col[nnz] (int32),
 *     val[nnz] (double);
 *   - embeddings are row-major n x n_components doubles;
 *   - every call returns a tsne_status; on error tsne_last_error() holds a
 *     thread-local message.  No C++ exception crosses this boundary.
 *   - tsne_* functions take HOST buffers (caller-owned); tsne_dev_* take
 *     DEVICE buffers on the context's device and enqueue on its stream.
 * Numerics are fp64 everywhere except the kNN candidate filter: a bf16x3
 * split-precision MFMA pass (each fp32 coordinate as two bf16 parts, three
 * bf16 products per term, fp32 accumulation) with a rigorous error bound,
 * followed by an exact fp64 re-rank of the survivors.
 */
#ifndef TSNE_HIP_H
#define TSNE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSNE_HIP_ABI_VERSION 2
#define TSNE_UNIQUE_ID_BYTES 128

typedef enum {
    TSNE_OK = 0,
    TSNE_ERR_ARG = -1,          /* IllegalArgumentException in the reference */
    TSNE_ERR_HIP = -2,          /* HIP runtime / kernel launch failure */
    TSNE_ERR_NOMEM = -3,
    TSNE_ERR_UNSUPPORTED = -4,  /* e.g. n_components not 2 or 3 (Cell.scala:32 requires 2) */
    TSNE_ERR_CAPACITY = -5,     /* caller buffer too small; required size reported */
    TSNE_ERR_COMM = -6,         /* RCCL failure */
    TSNE_ERR_NO_DEVICE = -7
} tsne_status;

/* Tsne.getMetric (Tsne.scala:161-168) */
typedef enum {
    TSNE_METRIC_SQEUCLIDEAN = 0,
    TSNE_METRIC_EUCLIDEAN = 1,
    TSNE_METRIC_COSINE = 2
} tsne_metric;

/* Optimizer parameters; defaults = Tsne.scala:47-63 + TsneHelpers.scala:386. */
typedef struct {
    int32_t n_components;       /* --nComponents, 2 (3: octree extension) */
    int32_t metric;             /* --metric, sqeuclidean (used for the attractive q) */
    double learning_rate;       /* --learningRate, 1000 */
    int32_t iterations;         /* --iterations, 300 */
    double early_exaggeration;  /* --earlyExaggeration, 4 */
    double initial_momentum;    /* --initialMomentum, 0.5 */
    double final_momentum;      /* --finalMomentum, 0.8 */
    double theta;               /* --theta, 0.25 */
    double min_gain;            /* hard-coded 0.01 (TsneHelpers.scala:386) */
} tsne_params;

typedef struct tsne_ctx tsne_ctx;

/* ---------------------------------------------------------------- basics */
int tsne_abi_version(void);
const char *tsne_last_error(void);
void tsne_params_default(tsne_params *p);
/* Tsne.getMetric (Tsne.scala:161-168): unknown name -> TSNE_ERR_ARG. */
int tsne_metric_from_name(const char *name, int32_t *metric_out);
/* Host-side CSR from COO triples, for callers that receive a DataSet's
 * triples one at a time (the JNI operator bodies stream a Flink iterator into
 * off-heap arrays: TsneHelpers.scala:162-196's groupBy(0) without JVM arrays,
 * so nothing is bounded by 2^31 elements).  row[e] in [0, n); rows come out
 * in index order, each row's entries in input order (a stable counting sort,
 * the reference's group order).  row_ptr_out: n + 1; col_out / val_out: nnz
 * (val / val_out may be NULL).  No context, no device. */
int tsne_coo_to_csr(const int32_t *row, const int32_t *col, const double *val, int64_t nnz, int64_t n,
                    int64_t *row_ptr_out, int32_t *col_out, double *val_out);
/* Row shard [r0, r1) of rank `rank` out of `world` (contiguous, balanced). */
int tsne_shard_rows(int64_t n, int32_t world, int32_t rank, int64_t *r0, int64_t *r1);
/* Cost-balanced cuts of the Morton-sorted BH queries (the rule the multi-GPU
 * optimizer applies on the device every iteration): bcost[b] = cost of the
 * queries [b*bucket, (b+1)*bucket); bounds[0..world] with bounds[0] = 0,
 * bounds[world] = n and bounds[r] = min(n, (b+1)*bucket) for the first bucket
 * b whose inclusive cost prefix reaches total*r/world (a zero target cuts at
 * 0; all-zero costs cut equal counts). */
int tsne_balance_cuts(const uint64_t *bcost, int64_t nb, int64_t n, int32_t world, int32_t bucket,
                      int64_t *bounds);
/* The same cuts computed by the device kernel (bucket 256) from device
 * buffers; for testing the kernel against tsne_balance_cuts. */
int tsne_dev_balance_cuts(tsne_ctx *ctx, const uint64_t *d_bcost, int64_t n, int32_t world, int64_t *d_bounds);

/* ---------------------------------------------------------------- context */
int tsne_ctx_create(int32_t device, tsne_ctx **out);
/* One caller, several GPUs (SURVEY.md 8b "Threading": a Flink operator at
 * parallelism 1 drives the node).  Creates one rank context per entry of
 * devices[0..ndev) and their communicator: RCCL (ncclCommInitAll, over xGMI)
 * when all devices are distinct, an in-process loopback when all are the same
 * device (ndev ranks sharing one GPU -- executes the multi-GPU code path on a
 * single GPU, for testing).  On the returned handle tsne_knn splits the query
 * rows and tsne_optimize shards the rows of P and the BH queries over the
 * ranks, one host thread per rank, results written to the caller's buffers
 * once; every other host-buffer operator, and the single-device tsne_dev_*
 * calls (kNN, affinities, joint, repulsion), run on the first device.  The
 * device-resident optimizer (tsne_dev_opt_*) holds one rank's state and
 * returns TSNE_ERR_UNSUPPORTED on a handle of ndev > 1: use tsne_optimize
 * there, or one context per rank.  Destroy with tsne_ctx_destroy. */
int tsne_ctx_create_multi(const int32_t *devices, int32_t ndev, tsne_ctx **out);
int tsne_ctx_destroy(tsne_ctx *ctx);
/* Enqueue on a caller-owned hipStream_t (e.g. torch's current stream). NULL = own stream. */
int tsne_ctx_set_stream(tsne_ctx *ctx, void *hip_stream);
void *tsne_ctx_stream(tsne_ctx *ctx);
int tsne_ctx_synchronize(tsne_ctx *ctx);
/* Per-handle tunables (no reference counterpart: the reference has no BH
 * shortcuts).  The defaults are the library's choices; a setting applies to
 * every later call on this handle (every rank of a tsne_ctx_create_multi
 * handle), never to other handles or threads.  Keys:
 *   "near_tol_early" 1e-6, "near_tol_late" 5e-6   near-exact BH subtrees:
 *       relative bound per summarised cell, for single gradients and the
 *       optimizer's early-exaggeration phase / after it (0: the test is off);
 *   "mom_tol" 1e-12           subtree-moment truncation bound (2-D);
 *   "near_tol3_early" 1e-7, "near_tol3_late" 5e-6, "mom3_tol" 1e-12, and
 *   "oct_moments" 1           the same for the 3-D octree;
 *   "oct_records" 2           3-D: octal records and the 64-query record
 *                             traversal (1: the 8-query one; 0: the
 *                             binary-node walk);
 *   "oct_layout_switch" 6     3-D with oct_records 2: the 8-query layout
 *                             while the octree's root half-width is below
 *                             this x the near-exact radius (0: never);
 *   "coherent_sort" 1         the trees' Morton sort from the previous build's
 *                             order (0: rocPRIM's radix sort; the same
 *                             permutation);
 *   "root_tile" 1             root-tile shortcut of the small-embedding phase;
 *   "attract_tiles" 1         tiled attraction where the labels allow it;
 *   "attract_tiles3" 0        3-D: the tiled attraction too (slower than the
 *                             row kernel beside the octree traversal at C4);
 *   "attract_cfg" -1          its tile shape (-1 automatic, 0..3);
 *   "attract_pipe" 0          2-D tiled attraction: 0 attract_tiles; 1..5 the
 *                             pipelined kernel (entries of the next 1 or 2
 *                             slices in flight; identical results);
 *   "attract_dyn" 1           attract_tiles: the waves claim a tile's slices
 *                             instead of taking every 16th (non-loss launches;
 *                             identical results);
 *   "attract_stream" 1        2-D tiled attraction with "attract_pipe" 0: the
 *                             non-loss launches read a second storage of the
 *                             tiles (each wave's entries of a row block one
 *                             contiguous stream, every step padded to 64
 *                             lanes with zero values) through a ring of
 *                             unconditional wide loads (attract_tiles_stream;
 *                             identical results; 0: attract_tiles only);
 *   "graph_order" 1           P's graph order as the initial labels;
 *   "relabel" -1              Morton relabels: -1 automatic, 0 never, 1 by
 *                             locality score, 2 always;
 *   "recut" 0                 several ranks on the tiled layout: re-cut the
 *                             row ownership by BH cost instead of relabels;
 *   "knn_bf16" 1              kNN threshold filter on bf16x3 MFMA (0: the
 *                             f32-input MFMA; results are identical);
 *   "narrow" 3                BH: 64-query groups costing >= this x the mean
 *                             run in the narrow layout (0: off).  The
 *                             selection reads the previous traversal's costs:
 *                             the optimizer's previous iteration, and for the
 *                             single-call operators only with
 *   "spill" 0, "spill_task" 0.25, "spill_min" 256, "spill_force" 0,
 *   "spill_drains" 2          BH work splitting (2-D): a walk past spill x the
 *                             previous traversal's mean cost (>= spill_min
 *                             record pops; spill_force: a fixed budget) hands
 *                             the rest of its stack to task lists that
 *                             spill_drains follow-up launches take, splitting
 *                             again past spill_task x that budget; the sums are
 *                             deterministic, equal to the unsplit walk to
 *                             rounding (0: off, the default: slower at C3);
 *   "tile_stream" 0, "tile_stream_max" 0, "tile_stream_frac" 1,
 *   "tile_stream_wait" 48, "tile_stream_gate" 1, "trav_prio" 0
 *                             BH tile streaming (2-D, one rank): tile_stream
 *                             workgroups per CU (<= 8), on a stream of their
 *                             own and (gate 1) dispatched once every traversal
 *                             block has started, sum the finished traversal
 *                             waves' tile lists of cost (points + 16 per task)
 *                             <= tile_stream_max (0: tile_stream_frac x the
 *                             previous tile plan's chunk unit) while the
 *                             traversal's last waves run, leaving after
 *                             tile_stream_wait polls (~0.4 us each) without a
 *                             list; the slot path sums the rest.  Deterministic;
 *                             tile_stream_max <= 4095: the bits of 0 (off, the
 *                             default: measured slower at C3).
 *                             trav_prio 1-3: the 64-query traversal's waves at
 *                             that issue priority (no measured effect);
 *   "trav_burst" 1            the 64-query BH traversal (2-D) reads a popped
 *                             record's fields from LDS in bursts: the head's
 *                             at once, each child's while the child before it
 *                             is evaluated (0: one by one, at first use; the
 *                             same bits; not the tree partition's walks);
 *   "trav_front" 0             > 0: the 64-query traversal's workgroups whose
 *                             heaviest wave cost >= this x the previous
 *                             traversal's mean are dispatched first (the order
 *                             is made with the narrow selection; same sums; no
 *                             measured gain);
 *   "trav_front_cur" 0         > 0: as trav_front with the order predicted from
 *                             each point's previous cost through the current
 *                             Morton order (made during the build; slower);
 *   "attract_serial_t0" 0, "attract_serial_t1" -1
 *                             2-D optimizer: for t in [t0, t1] the attraction
 *                             runs after the BH kernels instead of beside them
 *                             (an A/B of the overlap; slower);
 *   "wave_log" 0               with "rep_stats": the counting call logs every
 *                             BH wave's start and end (tsne_debug_wave_log);
 *   "bh_split" 0              several ranks (2-D), 1: partition the Barnes-Hut
 *                             tree by ranges of its sorted points -- every rank
 *                             walks every query over the cells holding its own
 *                             points, each term taken by one rank, and the
 *                             forces are summed by a reduce-scatter to the row
 *                             owners (0: partition the queries, Z-only exchange);
 *   "bu_acqrel" 1             the tree build's cross-workgroup bottom-up
 *                             hand-off uses agent-scope acquire-release
 *                             arrivals (the HIP memory model's ordering); 0:
 *                             relaxed arrivals ordered by gfx950's in-order
 *                             issue (the same trees; no measurable cost
 *                             difference);
 *   "build_fuse" 1            the 2-D tree build's short chain: the coherent
 *                             sort computes the Morton keys itself and writes
 *                             the sorted positions, the in-root count and the
 *                             duplicate counts from its bucket workgroups, and
 *                             the subtree moments run on the second stream
 *                             beside the traversal; 0: one launch per pass
 *                             (the same arrays, bit for bit);
 *   "bh_chain" 1              2-D Barnes-Hut, where the tile sums wait for
 *                             nothing they do not read: the subtree moments
 *                             "build_fuse" defers run on a stream of their own
 *                             from the traversal's start, the narrow groups'
 *                             moment sums and the next traversal's selection
 *                             on the second stream; 0: the moments behind the
 *                             narrow waves, the rest on the main stream behind
 *                             the tile sums (the same F, Z, bit for bit; 0 is
 *                             also what "spill", "tile_stream" and
 *                             "trav_front_cur" keep);
 *   "tile_pass" 0            the tile sums' packed rounds (<= 64 points of
 *                             consecutive small tiles): 1: each lane walks its
 *                             tiles of a round as runs of staged points; 2, 4,
 *                             8: over passes of that many consecutive rounds,
 *                             staged together and walked in one loop; 0: the
 *                             earlier slot-mask loops, a round at a time (the
 *                             same sums, bit for bit, for every value);
 *   "tile_prefetch" 1         the tile sums' lane-wise windows (tile_pass 0,
 *                             the traversal waves' own lists, n <= 2^28): 1:
 *                             a lane gathers the two points of its next step
 *                             while it sums this step's, through 32-bit offsets
 *                             from the sorted positions; 0: each step waits
 *                             for its own gathers (the same sums, bit for bit);
 *   "transform_resort" 10    tsne_dev_transform_step: the new points are sorted
 *                             again by the map tree's Morton key every this
 *                             many steps (0: only at setup); changes no result,
 *                             only which points share a wave;
 *   "transform_split" 0       1: a transform step as two launches (the walk,
 *                             then attraction + update) instead of the fused
 *                             one; the same bits (an A/B);
 *   "transform_stats" 0       1: tsne_[dev_]repulsion_queries_c on a 3-D map
 *                             counts its walk's stack pops, read with the
 *                             "xform3.pops" counter below (a measurement aid;
 *                             the same sums);
 *   "loop_serial" 0         1 (a loopback tsne_ctx_create_multi group, set
 *                             before tsne_optimize): the ranks take turns on the
 *                             device and log their work between collectives --
 *                             a one-GPU projection of N GPUs, read with
 *                             tsne_ctx_loop_profile;
 *   "comm_world1" 0           1: tsne_ctx_init_comm / tsne_ctx_init_comm_callbacks
 *                             at world 1 still create the communicator (RCCL:
 *                             a one-rank ncclCommInitRankConfig, id may be
 *                             NULL), and the optimizer runs its sharded path
 *                             through it -- the transport's own test;
 *   "rep_stats" 0             1: tsne_repulsion / tsne_dev_repulsion (2-D) run
 *                             the traversal's counting variant, read with the
 *                             "bh.*" counters below (diagnostics; the same sums);
 *   "reuse_costs" 0           1: tsne_gradient / tsne_repulsion select from the
 *                             previous call's costs (results then depend on
 *                             the call history at rounding level; 0 keeps
 *                             every single call a function of its input).
 * Unknown keys and out-of-range values return TSNE_ERR_ARG. */
int tsne_ctx_set_option(tsne_ctx *ctx, const char *key, double value);
/* HIP runtime versions (HIP_VERSION encoding, major * 10^7 + minor * 10^5 +
 * patch): the headers this library was built with, and the runtime the
 * process loaded (e.g. a host framework's bundled libamdhip64).  The
 * bindings refuse a different major version.  No device needed. */
int tsne_hip_versions(int32_t *built_out, int32_t *runtime_out);
int tsne_ctx_get_option(tsne_ctx *ctx, const char *key, double *value_out);
/* The loopback group's "loop_serial" summary (JSON: the span of the ranks'
 * work between collectives, per collective and per 100 occurrences) of the
 * segments logged since the last read; *len_out = its length (buf may be NULL
 * to ask: the summary is then kept for the next call, which copies it out), at
 * most cap - 1 bytes + NUL written.  Empty for other handles. */
int tsne_ctx_loop_profile(tsne_ctx *ctx, char *buf, int64_t cap, int64_t *len_out);
/* Diagnostic counters of the last call (synchronises the context's stream):
 *   "bh.narrow_groups"   64-query groups the last single-call BH traversal
 *                        (tsne_gradient / tsne_repulsion) ran in the narrow layout;
 *   "opt.narrow_groups"  the same for the optimizer's last iteration;
 *   "bh.pops", "bh.child_slots", "bh.tile_points", "bh.visits"  with option
 *                        "rep_stats": the last 2-D single-call repulsion's
 *                        traversal stack pops (wave level), child slots
 *                        evaluated (wave level), tile points, and
 *                        reference-equivalent node evaluations;
 *   "bh.wave_ticks_max", "bh.wave_ticks_sum", "bh.span_ticks"  (rep_stats) the
 *                        traversal waves' longest and summed run time and
 *                        the grid's span, in 100 MHz ticks (both layouts);
 *   "bh.tile_ticks_max", "bh.tile_ticks_sum", "bh.tile_span_ticks"  (rep_stats)
 *                        the same for tile_apply's waves;
 *   "bh.dense_pairs", "bh.moment_evals", "bh.tile_steps0".."bh.tile_steps3",
 *   "bh.tile_pairs0".."bh.tile_pairs3"  (rep_stats) exact-sum work: pair terms,
 *                        moment evaluations, and per dense path of tile_apply
 *                        (lane-wise, packed, query-major, staged sweep) the
 *                        wave steps issued and the useful lane pairs;
 *   "bh.tile_gsteps<p>_<G>", p = 0 | 1, G = 2 | 4 | 8  (rep_stats, tile_pass <= 1)
 *                        the wave steps that passes over G consecutive
 *                        lane-wise windows (0) / packed rounds (1) would take;
 *   "bh.tile_rounds_max", "bh.tile_chunked_waves"  (rep_stats) the most packed
 *                        rounds of one tile_apply wave; the waves that are one
 *                        chunk of a split tile list;
 *   "bh.narrow_moment_tasks"  (rep_stats) the moment evaluations listed for the
 *                        narrow groups' queries ("bh.moment_evals" counts the
 *                        64-query groups' only);
 *   "comm.kind"         the context's communicator: 0 none, 1 RCCL, 2 loopback,
 *                        3 caller callbacks; "comm.calls" collectives it issued;
 *   "opt.attract_kernel" the optimizer's attraction kernel: 0 attract_rows,
 *                        1 attract_tiles, 2 attract3 (3-D), 3 attract_tiles3
 *                        (3-D, tiled), -1 no optimizer;
 *   "opt.attract_cfg"    the tiled layout's row-block configuration: 0..3 the
 *                        2-D ATCfg0..3 (512 .. 4096 rows), 4 / 5 the 3-D
 *                        2048- / 512-row blocks; -1 when the layout is off;
 *   "opt.attract_pad_ppm" the stream layout's stored slots per real entry,
 *                        in parts per million (>= 1000000; 0: not built);
 *   "opt.csort_oversized_total"  the same summed over every build of the optimizer's tree;
 *   "bh.csort_oversized", "opt.csort_oversized"  buckets of the last coherent
 *                        Morton sort (csort.hpp) beyond its LDS capacity;
 *   "bh.spill_tasks", "opt.spill_tasks"  BH walks split off as tasks (option
 *                        "spill"), summed over every traversal of the tree;
 *   "bh.spill_flags", "opt.spill_flags"  1 a task list full, 2 task tile pages
 *                        exhausted (those walks went on unsplit / untiled: the
 *                        same sums, but their split points then depend on timing);
 *   "bh.stream_lists", "opt.stream_lists"  tile lists the streaming consumers
 *                        summed (option "tile_stream"), over every traversal;
 *   "xform3.pops"        with option "transform_stats": stack pops (wave level,
 *                        64 queries per wave) of the last 3-D
 *                        tsne_[dev_]repulsion_queries_c walk;
 *   "knn.fallback_queries"  queries of the handle's last tsne_[dev_]knn /
 *                        tsne_[dev_]knn_cross call that the exact fp64 scan
 *                        answered instead of the filter + re-rank (candidate
 *                        buffer overflow, a crowd at the k-th distance, or k
 *                        beyond the cross form's buffers), summed over the cross
 *                        form's query slices and a group's ranks.  Kept on the
 *                        host: no synchronisation; no result depends on it;
 *   "quality.fallback_x", "quality.fallback_y"  the same count for the neighbour
 *                        lists in X and in Y of the handle's last
 *                        tsne_[dev_]embedding_quality call. */
int tsne_ctx_counter(tsne_ctx *ctx, const char *name, int64_t *value_out);

/* Diagnostics (option "wave_log" with "rep_stats"): the last counting
 * repulsion call's BH waves as (start, end << 2 | kind) pairs in 100 MHz wall
 * ticks, kind 0 64-query traversal, 1 narrow, 2 tile_apply; up to cap pairs
 * copied to out, *count = the pairs logged (<= 2^17). */
int tsne_debug_wave_log(tsne_ctx *ctx, uint64_t *out, int64_t cap, int64_t *count);

/* Multi-GPU, one process per GPU over RCCL.  Rank 0 calls
 * tsne_comm_unique_id and ships the bytes to the other ranks out of band
 * (torch.distributed / MPI / a file); every rank then calls
 * tsne_ctx_init_comm.  Afterwards tsne_optimize / tsne_dev_opt_* shard the
 * rows of P and the BH queries (each rank owns a range of internal labels,
 * re-cut by measured BH cost when the labels are renumbered); per iteration
 * only the updated embedding slices (all-gather) and Z (all-reduce) cross
 * ranks.  Results are replicated on every rank.  (tsne_knn takes explicit
 * query ranges per rank.) */
int tsne_comm_unique_id(uint8_t id_out[TSNE_UNIQUE_ID_BYTES]);
int tsne_ctx_init_comm(tsne_ctx *ctx, int32_t rank, int32_t world,
                       const uint8_t id[TSNE_UNIQUE_ID_BYTES]);
int tsne_ctx_rank(tsne_ctx *ctx, int32_t *rank, int32_t *world);

/* Collectives supplied by the host dataflow instead of RCCL (e.g. carried by
 * the JVM's own network stack across nodes, or torch.distributed in tests).
 * Each operates in place on a HOST buffer and returns 0 on success; every
 * rank calls them in the same order.  allgatherv: rank r's bytes
 * [off[r], off[r+1]) of buf (off has world + 1 entries) must reach every
 * rank's buf. */
typedef struct {
    int (*allreduce_sum_f64)(void *user, double *buf, int64_t count);
    int (*allreduce_sum_u64)(void *user, uint64_t *buf, int64_t count);
    int (*allgatherv)(void *user, void *buf, const int64_t *off);
} tsne_comm_ops;
int tsne_ctx_init_comm_callbacks(tsne_ctx *ctx, int32_t rank, int32_t world, const tsne_comm_ops *ops,
                                 void *user);

/* ------------------------------------------------- host-buffer operators */

/* kNearestNeighbors (TsneHelpers.scala:41-59).  X: n x d row-major.
 * For query rows [q0, q1): the kk = min(k, n-1) nearest j != i, ascending by
 * (metric value, j).  idx_out / dist_out: (q1-q0) x kk.  Distances are the
 * exact fp64 breeze metric values (sequential sums). */
int tsne_knn(tsne_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t metric,
             int32_t k, int64_t q0, int64_t q1, int32_t *idx_out, double *dist_out);

/* projectKnn (TsneHelpers.scala:93-160, ZOrder.scala:25-42; --knnMethod
 * project): candidates = the k Z-order neighbours on either side of each
 * point in the input and in `iterations - 1` shifted copies x + r_s (shifts:
 * (iterations-1) x d, uniform [0,1) vectors supplied by the caller -- the
 * reference draws them unseeded), ranked by the exact fp64 metric; idx_out /
 * dist_out: n x min(k, n-1), ascending by (distance, j).  The Z-order
 * comparator is the reference's (signed XOR of the raw bit patterns) and is a
 * total order for nonnegative inputs.  2*k*iterations <= 1024. */
int tsne_project_knn(tsne_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t metric, int32_t k,
                     int32_t iterations, const double *shifts, int32_t *idx_out, double *dist_out);
/* pairwiseAffinities (TsneHelpers.scala:162-180 + 434-504): per CSR row the
 * beta binary search to entropy ln(perplexity); p_out has the layout of dist. */
int tsne_pairwise_affinities(tsne_ctx *ctx, const int64_t *row_ptr, const double *dist,
                             int64_t nrows, double perplexity, double *p_out);

/* jointDistribution (TsneHelpers.scala:182-196): P = (C + C^T) / sum over the
 * union pattern (explicit zeros kept); output rows sorted by column.  If
 * cap < nnz returns TSNE_ERR_CAPACITY with *nnz_out set (cap = 2*nnz_in
 * always suffices). */
int tsne_joint_distribution(tsne_ctx *ctx, const int64_t *row_ptr, const int32_t *col,
                            const double *p, int64_t n, int64_t cap, int64_t *out_row_ptr,
                            int32_t *out_col, double *out_val, int64_t *nnz_out);

/* gradient (TsneHelpers.scala:221-318): Barnes-Hut with the reference
 * quadtree semantics and opening criterion.  P values are multiplied by
 * `exaggeration`.  Y, grad_out: n x 2.  sumq_out (Z) and loss_out (KL term
 * of TsneHelpers.scala:297-299) are optional (NULL). */
int tsne_gradient(tsne_ctx *ctx, const int64_t *row_ptr, const int32_t *col, const double *P,
                  int64_t n, const double *Y, int32_t metric, double theta, double exaggeration,
                  double *grad_out, double *sumq_out, double *loss_out);

/* gradient for c = 2 (== tsne_gradient) or c = 3: the 3-D octree extension
 * (the reference itself requires 2-D, Cell.scala:32): root
 * Cell(0,0,0,W) with W = max(dX, dY, dZ), 8 children (upper/lower x NW, NE,
 * SW, SE), the same max(h)/D < theta criterion on squared 3-D distances.
 * Y, grad_out: n x c.  Other c -> TSNE_ERR_UNSUPPORTED. */
int tsne_gradient_c(tsne_ctx *ctx, const int64_t *row_ptr, const int32_t *col, const double *P, int64_t n,
                    int32_t c, const double *Y, int32_t metric, double theta, double exaggeration,
                    double *grad_out, double *sumq_out, double *loss_out);
/* QuadTree.computeRepulsiveForce (QuadTree.scala:123-152; tree built as in
 * TsneHelpers.scala:227-256) for every point: F_out (n x c, the repulsive
 * force sum before the 1/Z normalisation) and z_out (n, the point's sumQ
 * contribution; Z = their sum, TsneHelpers.scala:266), original order.
 * c = 2, or 3 for the octree extension. */
int tsne_repulsion(tsne_ctx *ctx, const double *Y, int64_t n, int32_t c, double theta, double *F_out,
                   double *z_out);

/* updateEmbedding (TsneHelpers.scala:341-369), in place on Y, upd, gains. */
int tsne_update_embedding(tsne_ctx *ctx, int64_t n, int32_t c, const double *grad, double *Y,
                          double *upd, double *gains, double min_gain, double momentum,
                          double learning_rate);

/* centerEmbedding (TsneHelpers.scala:320-329), in place. */
int tsne_center_embedding(tsne_ctx *ctx, int64_t n, int32_t c, double *Y);

/* initWorkingSet (TsneHelpers.scala:198-219): Y ~ N(0, 1e-4^2) from a
 * counter-based generator keyed by `seed` (the reference ignores
 * --randomState; this build honours it), upd = 0, gains = 1. */
int tsne_init_working_set(tsne_ctx *ctx, int64_t n, int32_t c, uint64_t seed, double *Y,
                          double *upd, double *gains);

/* optimize (TsneHelpers.scala:396-430): all iterations on the device; Y,
 * upd and gains (n x n_components, 2 or 3) are read and written back.  loss_keys / loss_vals
 * receive (t, KL) for every t % 10 == 0 (the "loss" accumulator,
 * TsneHelpers.scala:297-300), at most loss_cap entries. */
int tsne_optimize(tsne_ctx *ctx, const tsne_params *params, const int64_t *row_ptr,
                  const int32_t *col, const double *P, int64_t n, double *Y, double *upd,
                  double *gains, int32_t *loss_keys, double *loss_vals, int32_t loss_cap,
                  int32_t *n_loss);

/* ----------------------------------------------------- device-buffer API */
/* Same operators, pointers on the context's device, enqueued on its stream.
 * They do not synchronise unless a result size must reach the host. */
int tsne_dev_knn(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t metric,
                 int32_t k, int64_t q0, int64_t q1, int32_t *d_idx, double *d_dist);
int tsne_dev_project_knn(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t metric, int32_t k,
                         int32_t iterations, const double *d_shifts, int32_t *d_idx, double *d_dist);
int tsne_dev_repulsion(tsne_ctx *ctx, const double *dY, int64_t n, int32_t c, double theta, double *d_F,
                       double *d_z);
int tsne_dev_pairwise_affinities(tsne_ctx *ctx, const int64_t *d_row_ptr, const double *d_dist,
                                 int64_t nrows, double perplexity, double *d_p);
/* Fixed-k conditional rows (row i = entries [i*k, (i+1)*k)), symmetrised into
 * caller-allocated CSR (capacity 2*n*k); *nnz_out is synchronised to host. */
int tsne_dev_joint_distribution(tsne_ctx *ctx, const int64_t *d_row_ptr, const int32_t *d_col,
                                const double *d_p, int64_t n, int64_t cap, int64_t *d_out_row_ptr,
                                int32_t *d_out_col, double *d_out_val, int64_t *nnz_out);

/* Device-resident optimizer.  setup copies the FULL P (every rank holds it;
 * rank r computes the rows of its range of the optimizer's internal point
 * labels) and the working set (Y, upd, gains: n x n_components, original
 * point order) into its own state and allocates the workspace; step runs
 * global iteration t (1-based) with the reference phase schedule; sync
 * writes the working set back to the caller's Y, upd and gains (original
 * order; with several ranks a collective call).  The caller's buffers are
 * not touched by a step (round 5: the per-step scatter of Y was a third of
 * the update's HBM traffic).  Losses for t % 10 == 0 stay on the device
 * and are read by tsne_dev_opt_losses.  Internal labels (2-D): P's graph
 * order at setup (connected components, BFS level), then every 25
 * iterations the Morton order of the embedding when it keeps more of P's
 * edges local -- cache locality of the CSR attraction's gathers; results do
 * not depend on the labelling beyond summation order.  n_components = 3 runs
 * the octree extension (see tsne_gradient_c). */
int tsne_dev_opt_setup(tsne_ctx *ctx, const tsne_params *params, const int64_t *d_row_ptr,
                       const int32_t *d_col, const double *d_P, int64_t n, double *d_Y,
                       double *d_upd, double *d_gains);
int tsne_dev_opt_step(tsne_ctx *ctx, int32_t t);
int tsne_dev_opt_sync(tsne_ctx *ctx);
int tsne_dev_opt_losses(tsne_ctx *ctx, int32_t *loss_keys, double *loss_vals, int32_t cap,
                        int32_t *n_loss);
/* The Z normaliser (sum of the BH sumQ over all points, TsneHelpers.scala:266)
 * of the last tsne_dev_opt_step: the value its gradient and loss used.
 * Synchronises the context stream. */
int tsne_dev_opt_last_z(tsne_ctx *ctx, double *z_out);
/* Per-stage timing of the last step (HIP events on the ctx stream), in ms:
 * [0] tree build, [1] BH repulsion (traversal + tile and moment kernels),
 * [2] Z reduce (+ its all-reduce with several ranks), [3] attraction kernel
 * (attract_tiles / attract_rows, timed on the stream it runs on -- a side
 * stream when it overlaps [0]-[2]), [4] wait for it, combine + update, loss,
 * embedding exchange, centring.
 * Also BH work counters of the last step (counters_out5, may be NULL):
 * [0] reference-equivalent node evaluations (lane visits; a leaf tile of m
 * points counts m), [1] subtree-moment evaluations, [2] dense pair terms,
 * [3] wave-level cell pops, [4] wave-level tile points, [5] lane child
 * evaluations, [6] wave child slots (lane utilisation = [5] / (64 * [6])),
 * [7] heaviest wave (its pops + tile points / 16), [8] most pops of a
 * wave, [9] most tile points of a wave.
 * enable: 1 on, 0 off, -1 leave unchanged. */
int tsne_dev_opt_profile(tsne_ctx *ctx, int32_t enable, double *ms_out5, int64_t *counters_out10);
/* Kernel time of every attraction launch since tsne_dev_opt_setup (HIP
 * events on the stream it ran on): its iteration t, a placement code
 * (0 non-loss launch on the side stream, concurrent with the tree build / BH
 * traversal; 1 loss launch alone on the context stream after Z; 2 loss launch
 * on the side stream with Z-free KL terms; 3 non-loss launch alone on the
 * context stream), ms.  Synchronises on the recorded events; *count = number
 * of launches kept (the last 16384; entries beyond cap are not written). */
int tsne_dev_opt_attract_log(tsne_ctx *ctx, int32_t *iters, int32_t *standalone, double *ms, int32_t cap,
                             int32_t *count);
/* Stage timers of the context (HIP events around the stage's kernels, on
 * their stream), in ms per interval since the stage was last reset:
 * "knn.filter" (the fp32-MFMA distance filter launches of the last kNN call),
 * "opt.attract" (see above), "opt.update" (combine + updateEmbedding +
 * centerEmbedding + write-back, per iteration), "pca.colmean", "pca.gram",
 * "pca.reduce", "pca.project" (the kernels of the last tsne_[dev_]pca* call,
 * one interval each).  *count = intervals. */
int tsne_ctx_stage_ms(tsne_ctx *ctx, const char *stage, double *ms_out, int32_t cap, int32_t *count);

/* ------------------------------------- embedding new points into a fitted map */
/* The reference embedding Yref (n x 2) stays fixed; m new points are placed
 * into it.  Not in the reference job (which only fits): the pieces are the
 * reference's own operators applied across two point sets.  The entry points
 * without a suffix are 2-D; the _c forms further down take the map's dimension
 * c = 2 or 3.  On a tsne_ctx_create_multi handle these run on the first
 * device. */

/* Cross kNN: for each of the m rows of Xq (m x d) the min(k, n) nearest rows
 * of X (n x d), ascending by (exact fp64 breeze metric, j).  No candidate is
 * excluded: a query equal to a reference row gets it at distance 0.  Ids and
 * distances are as exact as tsne_knn's.  idx_out / dist_out: m x min(k, n).
 * (X and Xq are stacked in a workspace copy: (n + m) x d doubles.) */
int tsne_knn_cross(tsne_ctx *ctx, const double *X, int64_t n, const double *Xq, int64_t m, int32_t d,
                   int32_t metric, int32_t k, int32_t *idx_out, double *dist_out);
int tsne_dev_knn_cross(tsne_ctx *ctx, const double *dX, int64_t n, const double *dXq, int64_t m, int32_t d,
                       int32_t metric, int32_t k, int32_t *d_idx, double *d_dist);

/* QuadTree.computeRepulsiveForce (QuadTree.scala:123-152) of the tree of the
 * n points of Y (built as in TsneHelpers.scala:227-256) for m points Q (m x 2)
 * that are NOT in the tree: F_out (m x 2) and z_out (m), in the order of Q.
 * The root cell goes through the h / D < theta test like any cell; a leaf
 * whose point equals the query contributes 0.  Every cell decision is the
 * reference's (no near-exact or moment shortcuts).  A query's result does not
 * depend on the other queries of the call, bit for bit. */
int tsne_repulsion_queries(tsne_ctx *ctx, const double *Y, int64_t n, double theta, const double *Q, int64_t m,
                           double *F_out, double *z_out);
int tsne_dev_repulsion_queries(tsne_ctx *ctx, const double *dY, int64_t n, double theta, const double *dQ,
                               int64_t m, double *d_F, double *d_z);

/* Initial positions of the new points: y_i = sum_e P_e Yref[col_e] over the
 * point's CSR row (row_ptr[m + 1], col = ids into the reference, P = the
 * conditional p_{j|i} of tsne_pairwise_affinities on the cross-kNN distances:
 * row-normalised, not symmetrised), summed sequentially in CSR order.  A row
 * without entries is TSNE_ERR_ARG.  Y_out: m x 2. */
int tsne_transform_init(tsne_ctx *ctx, const int64_t *row_ptr, const int32_t *col, const double *P, int64_t m,
                        const double *Yref, int64_t n, double *Y_out);

/* The transform optimizer: params->iterations iterations that move only the
 * new points.  Per iteration and new point i, independently of every other:
 *   rep_i, z_i = computeRepulsiveForce(y_i) over the tree of Yref,
 *   attr_i     = sum_e (ex P_e) q_e (y_i - Yref[col_e]),  q_e = 1 / (1 + |y_i - Yref[col_e]|^2),
 *   grad_i     = attr_i - rep_i / z_i      (the point's own normaliser, not a global Z),
 *   updateEmbedding(grad_i) with params' learning_rate, momenta and min_gain; no centring.
 * The exaggeration / momentum schedule is tsne_optimize's.  (t, loss) for
 * t % 10 == 0, loss = sum_i sum_e pe ln(pe / (q_e / z_i)), pe = ex P_e.  With
 * the per-point z_i a new point's result does not depend on which other
 * points are in the batch, bit for bit.  Y, upd, gains: m x 2, read and
 * written back.  m = 0 is a no-op; n_components != 2 is TSNE_ERR_UNSUPPORTED.
 * The host form validates row_ptr and col (TSNE_ERR_ARG). */
int tsne_transform(tsne_ctx *ctx, const tsne_params *params, const double *Yref, int64_t n,
                   const int64_t *row_ptr, const int32_t *col, const double *P, int64_t m, double *Y, double *upd,
                   double *gains, int32_t *loss_keys, double *loss_vals, int32_t loss_cap, int32_t *n_loss);
/* Device-resident form.  setup builds the tree of d_Yref once and sorts the
 * new points by its Morton key; the caller's buffers (all on the device) are
 * used in place and must stay valid and unchanged by others until the last
 * step.  step runs iteration t (1-based): one kernel launch, plus a small
 * reduce on loss iterations.  sync waits for the steps enqueued so far: the
 * working set is then current in d_Y, d_upd and d_gains (caller's order).
 * The state may coexist with tsne_dev_opt_*'s. */
int tsne_dev_transform_setup(tsne_ctx *ctx, const tsne_params *params, const double *d_Yref, int64_t n,
                             const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P, int64_t m,
                             double *d_Y, double *d_upd, double *d_gains);
int tsne_dev_transform_step(tsne_ctx *ctx, int32_t t);
int tsne_dev_transform_sync(tsne_ctx *ctx);
int tsne_dev_transform_losses(tsne_ctx *ctx, int32_t *loss_keys, double *loss_vals, int32_t cap,
                              int32_t *n_loss);

/* The same operators with an explicit map dimension c (the tsne_gradient_c
 * precedent).  c == 2 runs the 2-D path above, bit for bit.  c == 3 runs over
 * the octree of the map (the 3-D extension of the reference tree: root
 * Cell(0, 0, 0, W), W the largest of the three extents, criterion h / D <
 * theta with D the squared 3-D distance; 21 levels per axis -- distinct map
 * points that share a level-21 cell interact with a query directly; exact
 * duplicates are counted as the reference's insert counts them: a splitting
 * leaf re-inserts its point once).  Any other c is TSNE_ERR_UNSUPPORTED.  As in 2-D, no
 * near-exact, tile or moment shortcut is used for foreign queries, and a
 * query's result does not depend on the other queries of the call, bit for
 * bit.
 *   tsne_repulsion_queries_c: Y is n x c, Q m x c, F_out m x c, z_out m.
 *   tsne_transform_init_c:    Yref n x c, Y_out m x c.
 *   tsne_transform_c / tsne_dev_transform_setup_c: params->n_components (2 or
 *     3) is the width of Yref, Y, upd and gains; otherwise the arguments and
 *     results of tsne_transform / tsne_dev_transform_setup.
 * tsne_dev_transform_step / _sync / _losses serve whichever state was set up
 * last.  The host forms validate row_ptr and col as the 2-D ones do. */
int tsne_repulsion_queries_c(tsne_ctx *ctx, const double *Y, int64_t n, int32_t c, double theta, const double *Q,
                             int64_t m, double *F_out, double *z_out);
int tsne_dev_repulsion_queries_c(tsne_ctx *ctx, const double *dY, int64_t n, int32_t c, double theta,
                                 const double *dQ, int64_t m, double *d_F, double *d_z);
int tsne_transform_init_c(tsne_ctx *ctx, const int64_t *row_ptr, const int32_t *col, const double *P, int64_t m,
                          const double *Yref, int64_t n, int32_t c, double *Y_out);
int tsne_transform_c(tsne_ctx *ctx, const tsne_params *params, const double *Yref, int64_t n,
                     const int64_t *row_ptr, const int32_t *col, const double *P, int64_t m, double *Y, double *upd,
                     double *gains, int32_t *loss_keys, double *loss_vals, int32_t loss_cap, int32_t *n_loss);
int tsne_dev_transform_setup_c(tsne_ctx *ctx, const tsne_params *params, const double *d_Yref, int64_t n,
                               const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P, int64_t m,
                               double *d_Y, double *d_upd, double *d_gains);

/* ------------------------------------ principal components of the input rows */
/* Not in the reference job: the usual companions of t-SNE, as the initial
 * embedding and as the reduction of the input in front of the kNN.  For X
 * (n x d, row-major):
 *   mu_j = (1/n) sum_i X_ij;
 *   C    = (1/n) sum_i (x_i - mu)(x_i - mu)^T, two-pass (rows centred before
 *          the products), exactly symmetric;
 *   lambda_1 >= lambda_2 >= ... the eigenvalues of C, v_a the unit
 *          eigenvectors, each signed so that its coordinate of largest
 *          absolute value is positive (ties: the lowest index);
 *   scores = (X - mu) V^T (n x c_out): score (i, a) is the sequential sum over
 *          j = 0..d-1 of (X_ij - mu_j) * V_aj, every product and sum rounded.
 * All sums run in a fixed order that depends on n and d only (never on the
 * device): a call repeated on the same data gives the same bits, and the host
 * and device forms give the same bits.  The Gram matrix runs on the fp64 MFMA
 * (DESIGN.md 3g); C crosses to the host for the eigen-solve (d <= 2048: at most
 * 32 MB), so the device forms synchronise the stream.
 * Errors: TSNE_ERR_ARG for n < 2, d < 1, c_out < 1, c_out > min(d, 64), c > d;
 * TSNE_ERR_UNSUPPORTED for d > 2048 and for c other than 2 or 3.  On a
 * tsne_ctx_create_multi handle these run on the first device. */

/* All eigenpairs of the symmetric d x d matrix A (row-major; the lower
 * triangle is read) on the host: Householder tridiagonalisation, then
 * implicit-shift QL; single-threaded and deterministic.  evals_out[d]
 * descending; evecs_out is d x d, row a = v_a with the sign rule above.  A
 * non-finite entry or d < 1 is TSNE_ERR_ARG.  No context, no device. */
int tsne_sym_eig(const double *A, int32_t d, double *evals_out, double *evecs_out);

/* mean_out[d] and cov_out[d * d] = C. */
int tsne_pca_covariance(tsne_ctx *ctx, const double *X, int64_t n, int32_t d, double *mean_out, double *cov_out);
int tsne_dev_pca_covariance(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, double *d_mean, double *d_cov);

/* The leading c_out principal components: mean_out[d], components_out
 * [c_out * d] (row a = v_a), eigvals_out[c_out], scores_out[n * c_out].  Any
 * output may be NULL (without scores_out no projection runs). */
int tsne_pca(tsne_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t c_out, double *mean_out,
             double *components_out, double *eigvals_out, double *scores_out);
int tsne_dev_pca(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t c_out, double *d_mean,
                 double *d_components, double *d_eigvals, double *d_scores);

/* PCA initialisation of the working set (instead of tsne_init_working_set):
 * Y = scores[:, :c] * (1e-4 / sqrt(lambda_1)), upd = 0, gains = 1 (each n x c,
 * c = 2 or 3).  The first column of Y has standard deviation 1e-4, the scale
 * of initWorkingSet's N(0, 1e-4^2); no generator is involved.  lambda_1 <= 0
 * (constant data) is TSNE_ERR_ARG. */
int tsne_init_working_set_pca(tsne_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t c, double *Y,
                              double *upd, double *gains);
int tsne_dev_init_working_set_pca(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t c, double *d_Y,
                                  double *d_upd, double *d_gains);

/* ------------------------------------------------------------ scoring a map */
/* Not in the reference job: the rank-based scores of a map at the map's own
 * size (no n x n matrix; csrc/ranks.hip).  For a point set A
 * (n x d, row-major) and a metric:
 *   D(i, l)      the exact fp64 breeze metric value tsne_knn ranks by and
 *                returns in dist_out, bit for bit (sequential sums over the
 *                coordinates, no FMA; cosine: 1 - s / (|a||b|), sequential norms);
 *   rank_A(i, j) = 1 + #{ l != i : (key(D(i,l)), l) < (key(D(i,j)), j) }, key the
 *                order-preserving map of a double the kNN sorts by: the 1-based
 *                position of j in row i of tsne_knn(A, k = n - 1);
 *   rank_A(i, i) = 0.
 * Row i is skipped by index, not by distance: duplicates of point i count.
 * For an input X, a map Y (n x c, ranked by sqeuclidean), k and s scored rows S:
 *   N_X(i), N_Y(i)  the tsne_knn rows of i in X and in Y (k ids, ascending by (D, j));
 *   S_T = sum_{i in S} sum_{j in N_Y(i)} max(0, rank_X(i, j) - k);
 *   S_C = sum_{i in S} sum_{j in N_X(i)} max(0, rank_Y(i, j) - k);
 *   S_R = sum_{i in S} |N_X(i) & N_Y(i)|                          (all int64);
 *   trustworthiness = 1 - 2 S_T / (s k (2 n - 3 k - 1)), continuity the same
 *   with S_C, knn_recall = S_R / (s k).
 * With S = all rows these are the values of sklearn.manifold.trustworthiness.
 * Every count is an integer: a result does not depend on the other rows of the
 * call or on the launch, and repeats bit for bit.
 * Errors: TSNE_ERR_ARG for a bad metric, an id outside [0, n) (host forms; the
 * message names the first one; the device forms trust their ids), rows NULL
 * with s != n, k < 1, 2 n - 3 k - 1 <= 0, s == 0 for the scores;
 * TSNE_ERR_UNSUPPORTED for m > 1024 and k > 896.  On a tsne_ctx_create_multi
 * handle these run on the first device. */

/* rank_out[a * m + e] = rank_A(rows[a], cand[a * m + e]) for s rows of m
 * candidate ids each (m <= 1024; ids may repeat).  rows NULL: row a is point
 * a, and s must equal n.  s == 0 is a no-op. */
int tsne_neighbor_ranks(tsne_ctx *ctx, const double *A, int64_t n, int32_t d, int32_t metric, const int64_t *rows,
                        int64_t s, const int32_t *cand, int32_t m, int32_t *rank_out);
int tsne_dev_neighbor_ranks(tsne_ctx *ctx, const double *d_A, int64_t n, int32_t d, int32_t metric,
                            const int64_t *d_rows, int64_t s, const int32_t *d_cand, int32_t m, int32_t *d_rank);

/* scores_out = {trustworthiness, continuity, knn_recall}; sums_out =
 * {S_T, S_C, S_R} and row_sums_out (s x 3, the same three per scored row) may
 * be NULL.  rows NULL: every row is scored, and s must equal n.  c >= 1: nothing
 * is specific to 2 or 3.  The device form takes device pointers for X, Y, the
 * rows and the row sums, writes scores_out / sums_out on the host and
 * synchronises the stream. */
int tsne_embedding_quality(tsne_ctx *ctx, const double *X, int64_t n, int32_t d, int32_t metric, const double *Y,
                           int32_t c, int32_t k, const int64_t *rows, int64_t s, double scores_out[3],
                           int64_t sums_out[3], int64_t *row_sums_out);
int tsne_dev_embedding_quality(tsne_ctx *ctx, const double *d_X, int64_t n, int32_t d, int32_t metric,
                               const double *d_Y, int32_t c, int32_t k, const int64_t *d_rows, int64_t s,
                               double scores_out[3], int64_t sums_out[3], int64_t *d_row_sums);

#ifdef __cplusplus
}
#endif
#endif /* TSNE_HIP_H */
