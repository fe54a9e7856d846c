/* ugs_mi355.h -- C ABI of libugs_mi355.so, the MI355X-native (gfx950 / HIP) uniform k-subgraph sampler.
 *
 * This is the drop-in boundary for the reference's `ugs_sampler` plugin (AniruddhaMandal/SS-GNN,
 * src/samplers/ugs_sampler).  The reference exposes a pybind11 module (src/extension.cpp:4-13) taking
 * torch::Tensor arguments; this library exposes the same operations over plain pointers and sizes so
 * that any host language can bind them (ctypes stub: ss-gnn_amd/ugs_sampler/__init__.py; see
 * INTEGRATION.md).  No torch types appear in any signature.
 *
 * Conventions
 *   - every function returns 0 on success or a negative UGS_E_* code; ugs_last_error() returns the
 *     message of the calling thread's last failure (same text as the reference's exception where the
 *     reference has one).
 *   - `edge_index` is int64 [2, E] with explicit row stride (elements) so non-contiguous tensors need no copy:
 *     source of column j = edge_index[j], destination = edge_index[row_stride + j].
 *   - all outputs are int64, caller-allocated; `dst_is_device` != 0 means the output pointers are
 *     device (HBM) pointers, otherwise host pointers (pinned or pageable).
 *   - sampling always runs on the GPU: there is no CPU fallback.  Without a usable HIP device every
 *     sampling entry point fails with UGS_E_NO_DEVICE.
 */
#ifndef UGS_MI355_H
#define UGS_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UGS_OK 0
#define UGS_E_INVALID_HANDLE (-1)   /* "Invalid preproc handle"            reference src/sampler.cpp:105 */
#define UGS_E_NO_ROOTS (-2)         /* "No viable roots available"         reference src/sampler.cpp:149 */
#define UGS_E_BAD_MODE (-3)         /* "mode must be one of: ..."          reference src/ugs_sampler_batch_extension.cpp:89-90 */
#define UGS_E_BAD_ARG (-4)
#define UGS_E_NO_DEVICE (-5)        /* no usable HIP device / kernel image */
#define UGS_E_HIP (-6)              /* a HIP runtime call failed */
#define UGS_E_UNSUPPORTED (-7)      /* outside the limits documented in DESIGN.md (k > 32, nnz >= 2^31 per plan, ...) */
#define UGS_E_EDGE_SRC (-8)         /* edge_src range check                reference src/ugs_sampler_batch_extension.cpp:213-222 */
#define UGS_E_CAPACITY (-9)         /* ugs_sample_batch_stream: the call produced more edge entries than edge_capacity */

/* edge_mode of sample()            reference src/sampler.cpp:95 ("local" | "flat" | "global") */
#define UGS_EDGE_LOCAL 0
#define UGS_EDGE_FLAT 1
#define UGS_EDGE_GLOBAL 2
/* mode of sample_batch()           reference src/ugs_sampler_batch_extension.cpp:81 ("sample" | "graph" | "global") */
#define UGS_MODE_SAMPLE 0
#define UGS_MODE_GRAPH 1
#define UGS_MODE_GLOBAL 2
/* ugs_plan_fill only (no reference counterpart): endpoints numbered r * k + local index, r = row's position inside this call's row range --
 * the edge index the consumer builds from edge_index_t + repeat_interleave(arange(B), counts) * k
 * (reference src/gps/gps/models/ss_gnn.py:463-464), so that step (and its host synchronisation) disappears */
#define UGS_FILL_BATCH 3

const char *ugs_last_error(void);
const char *ugs_version(void);

/* Number of usable HIP devices (0 is an error: UGS_E_NO_DEVICE). */
int ugs_device_count(int *count);
/* Select the HIP device used by the calling thread's subsequent calls (default: current HIP device). */
int ugs_set_device(int device);

/* Stream of the calling thread's subsequent JOBS (ugs_sample_*, ugs_sample_batch_*, ugs_eps_*, ugs_uniform_*, ugs_rwr_*): `use` != 0 runs their kernels
 * and copies on `stream` (a hipStream_t; NULL = the default stream) instead of the library's own non-blocking stream; `use` = 0
 * restores the library's stream.  A caller that hands in DEVICE output buffers obtained from a stream-ordered allocator
 * (torch.empty on torch's current stream) must run the job on that stream: a block the allocator just recycled may still be
 * read by kernels queued there, and only stream order keeps the job's writes behind them.  The plan API takes its stream per call. */
int ugs_set_stream(void *stream, int use);

/* ---- preprocessing handles: replaces create_preproc / destroy_preproc / has_graphlets / get_preproc_info
 *      (reference src/preproc.cpp:262-314, pybind names src/extension.cpp:7-10) --------------------------------
 *      k is not limited here, like the reference's: the k <= 32 limit belongs to the sampling entries.  A graph of >= 2^21 columns
 *      (UGS_DEVICE_PREPROC=1: any graph with a column; =0: none) is preprocessed by the kernels of ugs_preproc.hip when a device
 *      is present and has room, but only for k <= 32: their breadth-first list has 32 slots, so a larger k always takes the host
 *      stages.  Both give the reference's values for every k; k <= 0 behaves like k = 1 (every root reaches, every weight is 1). */
int ugs_create_preproc(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, int64_t num_nodes, int k,
                       int64_t *handle_out);
int ugs_destroy_preproc(int64_t handle);                       /* unknown handles are ignored, like the reference */
int ugs_has_graphlets(int64_t handle, int *out);               /* unknown handle -> 0 */
int ugs_get_preproc_info(int64_t handle, int *found, int64_t *num_nodes, int64_t *num_edges_stored, double *Z,
                         int *bucket_count_nonzero);
/* internals of a handle for the preprocessing parity tests (any pointer may be NULL):
 * indptr int64[n+1], indices int32[nnz], edge_col int32[nnz], order int32[n], index_of int32[n],
 * suffix_deg int32[n], bucket_b double[n], prob double[n], alias int32[n] */
int ugs_preproc_dump(int64_t handle, int64_t *indptr, int32_t *indices, int32_t *edge_col, int32_t *order,
                     int32_t *index_of, int32_t *suffix_deg, double *bucket_b, double *prob, int32_t *alias);

/* ---- sample(): replaces sample(handle, m_per_graph, k, edge_mode, base_offset, seed)
 *      (reference src/sampler.cpp:91-290).  Two phases so that the caller owns the outputs:
 *      begin  runs the walks on the GPU and reports the number of edge entries;
 *      finish writes nodes[m,k], edge_index[2,total_edges], edge_ptr[m+1], edge_src[total_edges] and frees the job.
 *      ugs_job_cancel frees a job that will not be finished. ------------------------------------------------- */
typedef struct ugs_job ugs_job;
int ugs_sample_begin(int64_t handle, int m_per_graph, int k, int edge_mode, int64_t base_offset, int seed,
                     ugs_job **job_out, int64_t *total_edges_out);
int ugs_sample_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *edge_src,
                      int dst_is_device);

/* ---- sample_batch(): replaces sample_batch(edge_index, ptr, m_per_graph, k, mode, seed)
 *      (reference src/ugs_sampler_batch_extension.cpp:77-299), including its process-global LRU of
 *      preprocessing handles keyed by an FNV-1a hash that ignores k (include/cache.hpp:81-109).
 *      finish writes nodes[G*m,k], edge_index[2,total_edges], edge_ptr[G*m+1], sample_ptr[G+1],
 *      edge_src_global[total_edges]. ----------------------------------------------------------------------- */
int ugs_sample_batch_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                           int64_t num_graphs, int m_per_graph, int k, int mode, int seed, ugs_job **job_out,
                           int64_t *total_edges_out);
int ugs_sample_batch_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr,
                            int64_t *sample_ptr, int64_t *edge_src_global, int dst_is_device);
int ugs_job_cancel(ugs_job *job);

/* ---- ugs_sampler.sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode): sample_batch with one seed per graph -- the batched
 *      form of the reference trainer's presample loop (gps/experiment.py:379-440: one one-graph call per dataset graph,
 *      seed = cfg.seed + i).
 *      The law: the call returns exactly what ugs_sample_batch_begin(edge_index, ptr, m_per_graph, k, mode, seed) returns for the
 *      same batch, except that row b = g m + i draws from xorshift64*((uint64_t)(int64_t)seeds[g] + i 0x9e3779b97f4a7c15) instead
 *      of from `seed`.  Everything else is sample_batch's behaviour: the preprocessing LRU visited once per graph in graph order
 *      (its key ignores k), evictions, graphs of fewer than k vertices (m rows of -1), the three modes, sample_ptr.
 *      Consequence: graph g's block of m rows -- edge_ptr re-based, and in mode "sample" ptr[g] subtracted from the nodes and
 *      the graph's first column from edge_src -- equals the one-graph call sample_batch(columns of g, {0, n_g}, m, k, mode,
 *      seeds[g]) made as the g-th of a sequence of such calls on the same LRU: the reference's sample_batch does the same get / put
 *      per graph that separate calls do.  That block is therefore what the reference's presample loop caches for graph g.
 *      seeds: host array of num_graphs C ints (the one-graph call's seed type); must not be NULL when num_graphs > 0.
 *      Same argument checks and errors as ugs_sample_batch_begin, same job: finish with ugs_sample_batch_finish.  The plan comes
 *      from ugs_plan_create_batch (LRU replay, device batch pass); no streamed form and no early start. -------------------- */
int ugs_sample_graphs_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                            int64_t num_graphs, int m_per_graph, int k, int mode, const int32_t *seeds, ugs_job **job_out,
                            int64_t *total_edges_out);

/* The same call (reference src/ugs_sampler_batch_extension.cpp:77-299, same LRU, same results) for LARGE host-visible batches,
 * in one piece: the caller hands over its (pinned) host buffers up front -- nodes[G*m,k], edge_ptr[G*m+1], sample_ptr[G+1],
 * edge_src_global[edge_capacity] and edge_index_out[2*edge_capacity] -- and the rows are sampled in chunks whose results cross
 * PCIe on a second stream while the next chunk walks (the two-phase call copies only after the last walk).  On return
 * *total_edges_out = total, edge_index_out holds [2, total] CONTIGUOUSLY at its start (row 1 begins at edge_index_out + total) and
 * edge_src_global[total].  edge_capacity is the caller's estimate (e.g. the total of an earlier call on the same batch plus a
 * margin); a call that needs more returns UGS_E_CAPACITY with the buffers' contents undefined and *total_edges_out = the entries
 * reached when the room ran out (> edge_capacity, a lower bound on the total) -- repeat it through ugs_sample_batch_begin / _finish.
 * k = 1 or m_per_graph = 0 produce no entries: edge_capacity 0 with null edge buffers is accepted.  UGS_STREAM_CHUNK_ROWS overrides the chunk size (default: an eighth of the rows, >= 65536). */
int ugs_sample_batch_stream(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                            int64_t num_graphs, int m_per_graph, int k, int mode, int seed, int64_t edge_capacity,
                            int64_t *nodes, int64_t *edge_index_out, int64_t *edge_ptr, int64_t *sample_ptr,
                            int64_t *edge_src_global, int64_t *total_edges_out);
/* sample() of the handle API (reference src/sampler.cpp:91-290) streamed the same way: nodes[m,k], edge_ptr[m+1],
 * edge_src[edge_capacity], edge_index_out[2*edge_capacity] (holds [2, total] contiguously on return); UGS_E_CAPACITY as above. */
int ugs_sample_stream(int64_t handle, int m_per_graph, int k, int edge_mode, int64_t base_offset, int seed,
                      int64_t edge_capacity, int64_t *nodes, int64_t *edge_index_out, int64_t *edge_ptr, int64_t *edge_src,
                      int64_t *total_edges_out);
/* ugs_sample_batch_stream starts early: a batch whose 32 sampled words (first / last / evenly spaced columns, ptr ends) match a
 * batch seen before begins its walks on that batch's plan while the real lookup -- the content hash over every column and the LRU
 * replay of include/cache.hpp:81-109 -- runs on a helper thread; the results stand only if the lookup names the same plan, otherwise
 * the streams are drained and the call runs again on the right plan (same results, the early work is lost).  Counters since process
 * start: early starts that stood / that were thrown away.  UGS_NO_SPECULATION set = always look up first.  ugs_sample_batch_begin does
 * the same for batches of >= 2^21 columns (UGS_SPEC_MIN_COLS overrides the threshold: testing aid) and counts here too. */
int ugs_stream_stats(int64_t *early_starts_kept, int64_t *early_starts_discarded);
/* ugs_sample_batch_begin / ugs_sample_graphs_begin run the step of a batch of small graphs at begin, walk + fill into one staging area
 * sized for 2 k (k - 1) edge entries per row (the packed step).  Counters since process start, bumped once per such step when its
 * total is known: steps whose outputs fitted the staging (finish only copies out) / steps the kernel refused because repeated columns
 * pushed the total above the staging (the kernel wrote no edge entry, finish fills the ordinary way).  Either pointer may be NULL. */
int ugs_step_stats(int64_t *packed_staged, int64_t *packed_refused);

/* LRU of preprocessing handles used by ugs_sample_batch_* (capacity from UGS_CACHE_SIZE, default 1000;
 * reference src/ugs_sampler_batch_extension.cpp:15-38).  Clearing it is the equivalent of a fresh process. */
int ugs_cache_clear(void);
int ugs_cache_stats(int64_t *size, int64_t *hits, int64_t *misses);
/* Which path preprocessed the graphs of ugs_create_preproc and of the batch calls' LRU misses.  Counters since process start: graphs
 * whose CSR and root stages ran in ugs_preproc.hip / graphs preprocessed by the host stages (no device, no room, fewer than 2^21
 * columns, k > 32, no column or no vertex, UGS_DEVICE_PREPROC=0) / plan pieces whose adjacency arrays were written on the device from
 * the CSR such a graph left in HBM (the first plan assembled from it; a graph without entries counts, there is nothing to write)
 * instead of being copied from the host.  Graphs the device batch pass builds are counted by ugs_batch_pass_stats, not here.
 * Any pointer may be NULL. */
int ugs_preproc_stats(int64_t *device_graphs, int64_t *host_graphs, int64_t *device_pieces);
/* The input side of ugs_sample_batch_begin / ugs_plan_create_batch for batches of small graphs runs on the device (SURVEY.md
 * 8(f) N4): one pass over edge_index + ptr replaces the reference's per-graph slicing (src/ugs_sampler_batch_extension.cpp:41-75),
 * hashing (include/cache.hpp:81-109) and CSR construction (src/preproc.cpp:32-86); the host replays the LRU on the G keys that
 * come back.  Counters since process start: plans built that way / calls that took the general (host) path instead
 * (UGS_DEVICE_BATCH=0, non-monotone ptr, a graph with more than 2048 vertices or more columns than the limit below). */
int ugs_batch_pass_stats(int64_t *device_plans, int64_t *general_path);
/* Columns per graph up to which the pass applies.  Default 1000: up to there the reference's LRU key covers a graph's whole content;
 * beyond, it hashes every (columns / 500)-th column only (include/cache.hpp:100-107).  A caller whose graphs are larger raises the
 * limit, to 8192 at most: the pass then runs the large form of its kernels, which compute that strided key plus a 128-bit content
 * fingerprint, and accepts a cached graph only if n, nnz and the fingerprint agree -- two different graphs sharing a key send the
 * batch to the general path, which samples from the cached graph as the reference does.  Results never depend on the limit.
 * Process-wide and atomic; calls in flight keep the value they started with.  Outside 1000 ... 8192: UGS_E_BAD_ARG, value kept.
 * previous_out may be NULL.  Initial value: UGS_BATCH_PASS_MAX_COLS in the environment, read at first use (out of range = ignored,
 * reported under UGS_DEBUG=1). */
int ugs_set_batch_pass_max_cols(int64_t cols, int64_t *previous_out);
int64_t ugs_batch_pass_max_cols(void);

/* ---- device-resident plans: the batch (or single graph) preprocessed once and kept in HBM, sampled many times,
 *      optionally over a sub-range of the G*m result rows (multi-GPU sharding: row b = g*m + i depends only on
 *      (graph g, seed, i)).  All pointers passed to walk/fill are DEVICE pointers; `stream` is a hipStream_t
 *      (NULL = default stream).  Nothing here synchronises with the host unless stated. ------------------------ */
typedef struct ugs_plan ugs_plan;
/* Builds (or fetches from the plan cache) the plan of a batch through the same LRU as ugs_sample_batch_begin. */
int ugs_plan_create_batch(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                          int64_t num_graphs, int k, ugs_plan **plan_out);
/* Plan of one preprocessing handle (the handle API's graph). */
int ugs_plan_create_handle(int64_t handle, ugs_plan **plan_out);
int ugs_plan_release(ugs_plan *plan);
/* What the walk kernels read for graph `graph` of a plan, copied back from HBM (parity tests of the preprocessing that runs on the
 * device, incl. the cold path of the device batch pass: graphs the LRU does not know get their root records from ugs_bp_roots;
 * the host path's counterpart is ugs_preproc_dump).  level 0: prob / alias / v_self = order[vi] / v_alias = order[alias[vi]] per
 * order position (reference include/sampler.hpp:44-69 + src/preproc.cpp:176-256); levels 1, 2: the viable list (vi, order[vi])
 * (src/sampler.cpp:121-150).  Arrays hold `capacity` entries; any pointer may be NULL.  Synchronises with the device. */
int ugs_plan_graph_roots(ugs_plan *plan, int64_t graph, int64_t capacity, int32_t *level, int32_t *num_nodes, int32_t *num_viable,
                         double *prob, int32_t *alias, int32_t *v_self, int32_t *v_alias, int32_t *viable_vi, int32_t *viable_v);
/* The CSR rows the kernels read for graph `graph` of a plan, copied back from HBM (read-only, diagnostic: parity tests of the device
 * batch pass, whose build kernel writes these arrays itself).  rowptr: num_nodes + 1 values relative to the graph's first entry;
 * per entry the neighbour w and rank(w) (adj) and w and the batch column (adjf).  rowptr holds node_capacity + 1 values, the
 * entry arrays entry_capacity; any pointer may be NULL.  A degenerate graph (n <= 0 or n < k) reports num_nodes = 0.
 * Synchronises with the device. */
int ugs_plan_graph_csr(ugs_plan *plan, int64_t graph, int64_t node_capacity, int64_t entry_capacity, int32_t *num_nodes,
                       int64_t *num_entries, int64_t *rowptr, int32_t *nbr, int32_t *nbr_rank, int32_t *nbr_f, int32_t *nbr_col);
/* A second plan over the same device arrays with private scratch (a plan's scratch serves one stream at a time): two steps in
 * flight on two streams go through a plan and its twin alternately.  Release both; the arrays live until the last one goes. */
int ugs_plan_twin(ugs_plan *plan, int k, ugs_plan **twin_out);
/* num_graphs, total vertices, total CSR entries, bytes resident in HBM, walk-kernel tier chosen for k */
int ugs_plan_info(const ugs_plan *plan, int k, int64_t *num_graphs, int64_t *num_vertices, int64_t *nnz,
                  int64_t *device_bytes, int *tier);
/* The first-pick table of a plan, copied back from HBM (testing aid).  Plans of one graph keep, beside their padded rows and built
 * with them at the first walk of a one-walk-per-wave tier, 64 bytes per vertex: byte r of vertex v is the position, in the candidate
 * list D1(v) that the scan of v's row leaves when v is the root (the distinct neighbours that pass the suffix filter, in
 * first-occurrence order), of the candidate at position r of the iteration order of the reference's unordered_set built from D1(v)
 * (reference src/sampler.cpp:55-80); defined for r < |D1(v)| <= 64, and for the vertices a root can be (every vertex of a graph
 * whose roots are drawn by weight; the viable list of a relaxed one).  The launch-uniform walk takes a walk's first pick from it.
 * num_vertices: the plan's vertices, or 0 when the plan has no table (not built yet, several graphs, UGS_NO_FIRST_PICK_TABLE=1).
 * c1[v] = |D1(v)| (-1: more than the 448-candidate tier holds; 0 for a vertex no root can be), ord1 = the table; both hold
 * `capacity` vertices, either may be NULL.  Synchronises with the device. */
int ugs_plan_first_pick_table(ugs_plan *plan, int64_t capacity, int64_t *num_vertices, int32_t *c1, uint8_t *ord1);
/* Walk phase for rows [row_begin, row_begin+row_count) of the G*m rows: writes d_nodes[row_count,k] and
 * d_edge_ptr[row_count+1] (exclusive scan of the per-row edge-entry counts, starting at 0).
 * If total_edges_host is not NULL the stream is synchronised and the total is returned there. */
int ugs_plan_walk(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed,
                  int64_t row_begin, int64_t row_count, void *stream, int64_t *d_nodes, int64_t *d_edge_ptr,
                  int64_t *total_edges_host);
/* Fill phase: writes d_edge_index[2, ld] and d_edge_src[ld] for the same rows.  ld is the row stride of d_edge_index AND the
 * capacity (in edge entries) of both buffers: entries at positions >= ld are not written (a caller that sized the buffers from
 * an estimate compares d_edge_ptr[row_count] with ld afterwards). */
int ugs_plan_fill(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int64_t row_begin,
                  int64_t row_count, void *stream, const int64_t *d_nodes, const int64_t *d_edge_ptr,
                  int64_t *d_edge_index, int64_t ld, int64_t *d_edge_src);
/* Walk + fill of the same rows as ONE call, for callers that hand over edge buffers of capacity ld up front (no host read-back
 * of the total in between: d_edge_ptr[row_count] holds it afterwards).  Same outputs as ugs_plan_walk followed by ugs_plan_fill
 * (reference src/sampler.cpp:91-290).  Knowing that nobody reads edge_ptr between the two phases, the step of a batch of small
 * graphs of up to 131 072 rows runs in two launches instead of three: the fill kernel scans the per-row counts itself.  A block takes
 * tiles of 32 rows and adds up what lies in front of a tile from the sums of 8 rows that the walk kernel left beside the counts; no
 * block waits for or talks to another (`UGS_NO_FUSED_SCAN` set = the three-launch form).
 * Concurrent use: several threads may step, walk and fill through one plan (or through plans that the plan cache shares, e.g. two
 * ugs_plan_create_batch of the same batch) at the same time, on one stream or on several; the calls are serialised through the
 * plan's scratch and each gets its own correct outputs.  A step holds the plan's lock from its walk to its fill.  Steps that should
 * overlap on the device go through a plan and its twin (ugs_plan_twin) on two streams. */
int ugs_plan_step(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed, int64_t row_begin,
                  int64_t row_count, void *stream, int64_t *d_nodes, int64_t *d_edge_ptr, int64_t *d_edge_index, int64_t ld,
                  int64_t *d_edge_src);
/* Share (1..100 percent, default 100) of the blocks a CU can hold that this plan's walk kernels occupy.  The walk kernels are
 * persistent grids that keep every CU's registers, LDS and wave slots to their end; a job that runs other kernels BESIDE a walk
 * (the collation of the previous batch and its RCCL transfer on another stream) lowers the share so that those find room on
 * every CU instead of queueing behind the walk. */
int ugs_plan_set_walk_share(ugs_plan *plan, int percent);
/* A whole step (seed upload, walk tiers, scan, fill) of a plan captured ONCE as a HIP graph and replayed with a new seed:
 * for batches of small graphs a step is a handful of launches for tens of microseconds of work, and the graph removes the
 * per-launch gaps.  The buffers are the caller's (d_edge_index[2, ld], d_edge_src[ld]: ld >= the largest total it expects;
 * entries beyond ld are not written, and a replay whose total exceeds ld must not be used -- compare d_edge_ptr[row_count] with ld).  No reference counterpart
 * (the reference launches nothing); same results as ugs_plan_walk + ugs_plan_fill with that seed.  Launches of one graph
 * must be issued by one thread at a time and on one stream at a time (the outputs are the graph's buffers); up to 256 replays
 * may be in flight (ring of pinned seed slots). */
typedef struct ugs_graph ugs_graph;
int ugs_plan_graph_create(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int64_t row_begin,
                          int64_t row_count, int64_t *d_nodes, int64_t *d_edge_ptr, int64_t *d_edge_index, int64_t ld,
                          int64_t *d_edge_src, ugs_graph **graph_out);
int ugs_plan_graph_launch(ugs_graph *graph, int seed, void *stream);
int ugs_plan_graph_destroy(ugs_graph *graph);
/* Name and per-launch statistics of the kernels the last ugs_plan_walk / ugs_plan_fill on this plan launched
 * (grid, block, LDS bytes) -- used by bench.py to label its roofline line. */
int ugs_plan_last_launch(const ugs_plan *plan, char *name_buf, int name_buf_len, int *grid, int *block,
                         int *lds_bytes, int64_t *overflow_rows);
/* The same for the fill: name, grid and block of the kernel that the last ugs_plan_fill, ugs_plan_step or packed step on this plan
 * launched to write the edge outputs ("ugs_fill<8>", "ugs_fill<64>", "ugs_fill_scan<8>"; empty before the first).  A fill that
 * expands the rows the walk staged (ugs_fill_staged) and then reads the leftover rows reports the leftover kernel, the second of its
 * two launches.  Testing aid: which form of the step ran is not visible in its outputs.  Any out pointer may be NULL. */
int ugs_plan_last_fill(const ugs_plan *plan, char *name_buf, int name_buf_len, int *grid, int *block);

/* ---- collation of a sharded batch (multi-GPU: SURVEY.md section 8(e); the reference is single-process and has no counterpart).
 *      Rank r samples the contiguous row range [row_off[r], row_off[r+1]) of the G*m rows; the finished batch is collated on
 *      the rank that feeds the trainer by ONE fixed-size message per rank (any transport: RCCL gather / all-gather of bytes).
 *      Wire format of a message (little endian, every section 16-byte aligned; ugs_collate_layout gives the offsets):
 *        header    int64 rows, int64 edge entries of this rank
 *        nodes     [rows_cap, k]  int32 | int64                     (int32 when every node id fits)
 *        edge_ptr  [rows_cap + 1] uint32, rank-local (starts at 0)
 *        edge_index [2, edge_cap] uint8 | int32 | int64              (uint8: mode "sample", local ids < k)
 *        edge_src  [edge_cap]     int32 | int64
 *      rows_cap / edge_cap are the job's fixed capacities (>= every rank's rows / edge entries), so message size does not depend
 *      on a step's outcome and no host round trip is needed per step.
 *      ugs_collate_unpack turns `world` messages (contiguous, d_msgs[world][msg_bytes]) into the batch's int64 tensors on the
 *      device: offsets are taken from the headers ON the device, entries at positions >= ld are not written.  A message whose
 *      edge total exceeds edge_cap was truncated by its sender: the batch is then INVALID; d_max_total (one device word, kept
 *      by the caller across steps) receives the largest total seen so that the caller can find out without a per-step host
 *      round trip (total > edge_cap).
 *      A batch without rows (row_off[world] == row_off[0]) is legal: nothing is launched over rows or edge entries, the one
 *      closing word edge_ptr[row_off[world]] is set to 0, d_nodes / d_edge_index / d_edge_src may be null (an empty device
 *      tensor has no address) and *d_max_total is left as it is.  With rows, a null output pointer is refused. */
int ugs_collate_layout(int k, int node_bytes, int eidx_bytes, int esrc_bytes, int64_t rows_cap, int64_t edge_cap,
                       int64_t *section_off4, int64_t *msg_bytes);
int ugs_collate_unpack(const void *d_msgs, int world, const int64_t *row_off /* host, world+1 */, int k, int node_bytes,
                       int eidx_bytes, int esrc_bytes, int64_t rows_cap, int64_t edge_cap, int64_t *d_nodes,
                       int64_t *d_edge_index, int64_t ld, int64_t *d_edge_ptr, int64_t *d_edge_src,
                       int64_t *d_max_total /* optional: max(*d_max_total, every message's edge total), for a lazy capacity check */,
                       void *stream);

/* ---- epsilon_uniform_sampler.sample_batch(edge_index, ptr, m_per_graph, k, mode, seed, epsilon): replaces the reference's
 *      src/samplers/epsilon_uniform_sampler/src/epsilon_uniform_sampler.cpp:122-377.
 *      Random frontier growth (:18-87) with acceptance min(1, eps/(w+eps)) (:238), at most max(10, 10/eps) attempts per
 *      sample (:207); nodes of a sample sorted ascending (:256); edges = the batch columns with both endpoints in the sample,
 *      in column order, each once (:265-291); mode 0 ("sample") numbers endpoints 0..k-1 by sorted position, any other mode
 *      uses batch node ids; failed samples are rows of -1 without edges.
 *      The reference is NOT deterministic here (per-thread generators seeded with the OpenMP thread id, dynamic schedule,
 *      rows written in thread-completion order, :209-319).  This implementation is deterministic: one counter-based
 *      generator per (row, attempt), rows in graph order; parity with the reference is statistical.
 *      Same two-phase job protocol as ugs_sample_batch_*; finish writes nodes[G*m,k], edge_index[2,total],
 *      edge_ptr[G*m+1], sample_ptr[G+1], edge_src[total]. */
int ugs_eps_sample_batch_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                               int64_t num_graphs, int m_per_graph, int k, int mode, uint64_t seed, double epsilon,
                               ugs_job **job_out, int64_t *total_edges_out);
int ugs_eps_sample_batch_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                                int64_t *edge_src, int dst_is_device);

/* ---- epsilon_uniform_sampler.sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode, epsilon): the batched form of the
 *      reference trainer's presample loop (gps/experiment.py:379-440), which calls the sampler once per graph with
 *      seed = cfg.seed + i.  Every graph g has its own seed seeds[g]: row b = g m + i keys its generator with
 *      (seeds[g], i, attempt) instead of (seed, b, attempt), and nothing else differs from ugs_eps_sample_batch_begin.
 *      The law: graph g's block -- nodes rows [g m, (g+1) m), their edge entries, edge_ptr re-based to the block -- equals what
 *      ugs_eps_sample_batch_begin(edge_index, row_stride, num_cols, ptr + g, 1, m_per_graph, k, mode, seeds[g], epsilon) returns:
 *      node ids and the edge ids of the batch-id mode are batch ids and edge_src holds batch column indices, so nothing else
 *      needs re-basing; columns outside the graph's range are dropped, both modes.  sample_ptr = [0, m, 2m, ..., G m].
 *      seeds: host array of num_graphs values (copied by begin); NULL with num_graphs > 0 is UGS_E_BAD_ARG.
 *      graph_status: host array of num_graphs entries (may be NULL), written all zero -- no condition of this sampler makes one
 *      graph fail alone; a graph with fewer than k vertices gives m rows of -1 without edges, as in sample_batch.
 *      Same argument checks and error texts as ugs_eps_sample_batch_begin, same job: finish with ugs_eps_sample_batch_finish. */
int ugs_eps_sample_graphs_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                                int64_t num_graphs, int m_per_graph, int k, int mode, const uint64_t *seeds, double epsilon,
                                int32_t *graph_status, ugs_job **job_out, int64_t *total_edges_out);

/* ---- uniform_sampler.sample_batch(edge_index, ptr, m_per_graph, k, mode, seed): replaces the reference's
 *      src/samplers/uniform_sampler/src/uniform_sampler.cpp:86-285 (exact uniform sampling over ALL connected k-subsets).
 *      The law, for each graph g in batch order, vertices [ptr[g], ptr[g+1]), n = ptr[g+1] - ptr[g]:
 *        1. adjacency: only columns with both endpoints inside g's range count, symmetrised (:121-136);
 *        2. S_g: every k-subset of g's local vertices whose induced subgraph is connected, in lexicographic order of the
 *           ascending vertex tuples (combination DFS :47-80); k = 0 or n < k gives an empty list;
 *        3. draws: ONE std::mt19937_64(seed) for the call (:144); for each graph with S_g non-empty, m draws in order, each
 *           std::uniform_int_distribution<int>(0, |S_g|-1) (:189, include/uniform_sampler.hpp:16-29) = libstdc++'s Lemire step
 *           with a 128-bit product; graphs with S_g empty consume no draws and give m rows of -1 without edges;
 *        4. a row holds ptr[g] + v for the drawn subset's ascending local vertices;
 *        5. its edges: every batch column e, in column order, with both endpoints in g's range and in the subset (loops and
 *           duplicate columns included), edge_src = e; mode 0 ("sample") numbers the endpoints by position in the row, any
 *           other mode keeps batch ids (:193-236).
 *      The whole computation runs on the device (ugs_uniform.hip): extension-set enumeration of the connected subsets only
 *      (never all C(n, k)), per-root sort into lexicographic order, one-workgroup mt19937_64, rows and edges.  Bit-exact.
 *      Same two-phase job protocol and stream rules as ugs_sample_batch_*; finish writes nodes[G*m,k], edge_index[2,total],
 *      edge_ptr[G*m+1], sample_ptr[G+1], edge_src[total].
 *      Representation.  A graph of at most 64 vertices holds a set as a 64-bit mask (sort key: the bit-reversed mask,
 *      complemented).  A WIDE graph -- more than 64 vertices -- holds it as its ascending tuple t packed big-endian in fields of
 *      b = bit length of n - 1 bits: key = sum of t[i] << (b (k - 1 - i)).  Ascending keys are the reference's order and the root is
 *      the first field, so sorting, draws and rows are shared by both forms; the law above is the same.  A graph takes the wide form
 *      when 64 < n <= the limit in force (ugs_uniform_set_max_vertices, default 64: no graph does), 1 <= k <= 8 and k b <= 64:
 *      n <= 1024 up to k = 6, n <= 512 at k = 7, n <= 256 at k = 8.
 *      Errors: UGS_E_BAD_ARG for num_graphs < 0 (empty ptr), m < 0, k < 0, a decreasing ptr (the reference aborts on the last
 *      three); UGS_E_UNSUPPORTED for a graph with at least k vertices that has more than 64 and either more than the limit in
 *      force or a k outside the rule above (the message names the graph, the limit and the rule), and for a call with more than
 *      2^25 connected k-subsets in all (the device budget; it also keeps every |S_g| within the reference's int).
 *      The library stays usable after any of them. */
int ugs_uniform_sample_batch_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                                   int64_t num_graphs, int m_per_graph, int k, int mode, uint64_t seed,
                                   ugs_job **job_out, int64_t *total_edges_out);
int ugs_uniform_sample_batch_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                                    int64_t *edge_src, int dst_is_device);
/* ---- uniform_sampler.enumerate_graphs(edge_index, ptr, k, mode, max_rows) / count_graphs(edge_index, ptr, k, limit): the population
 *      ugs_uniform_sample_batch_begin draws from, whole.  Items 1, 2, 4 and 5 of the law above hold verbatim; item 3 (the draws) is
 *      replaced by:
 *        - S_g is the list of item 2 (empty for k = 0 or n < k); sample_ptr[g+1] - sample_ptr[g] = |S_g| for a healthy graph and 0
 *          for a failed one, sample_ptr[0] = 0, R = sample_ptr[G];
 *        - row sample_ptr[g] + i is the i-th set of S_g written as item 4 says, its edges as item 5 says; no row is padded with -1;
 *        - so row sample_ptr[g] + d is exactly the row ugs_uniform_sample_batch_begin / _sample_graphs_begin emit when the graph's
 *          generator draws d.
 *      enumerate_begin runs the same count pass, scan, write pass and sorts as the samplers, reads the per-graph counts back (the
 *      row count is known only then: the first of its two read-backs, the second is the edge total), and turns every key of the
 *      sorted array into a row.  Outputs of finish: nodes[R,k], edge_index[2,total_edges], edge_ptr[R+1], sample_ptr[G+1],
 *      edge_src[total_edges].  Same job protocol, stream rules and ugs_job_cancel as the other jobs; enumerate_finish takes only an
 *      enumeration job, ugs_uniform_sample_batch_finish does not take one.
 *      A graph that fails alone contributes no rows and leaves the others undisturbed: graph_status[g] = 1 for a graph of at least k
 *      vertices that ugs_uniform_sample_batch_begin refuses for its size (more than 64 vertices and over the limit in force, or a k
 *      outside the wide rule), 2 for a graph whose own |S_g| exceeds max_rows (count_graphs: limit); 0 otherwise.  graph_status is a
 *      host array of num_graphs entries, written by the call.  Healthy graphs whose sets TOGETHER exceed max_rows fail the call:
 *      UGS_E_UNSUPPORTED, "split the call".  max_rows must be 1 ... 2^25 (the device budget), else UGS_E_BAD_ARG; it sizes the two
 *      key arrays, while nodes, edge_ptr and the per-row edge counts are sized by R.  The other argument errors are those of
 *      ugs_uniform_sample_batch_begin.
 *      count_graphs is synchronous and has no job: counts_out[g] = |S_g|, exact wherever |S_g| <= limit; -1, with graph_status as
 *      above, for a graph past limit or refused for its size.  limit must be 1 ... 2^32, else UGS_E_BAD_ARG.  It runs the column
 *      buckets, the adjacency and the count pass only, stores no keys, allocates the adjacency and the per-item counters but
 *      neither key array, and its work per graph is bounded by limit (a graph past it stops counting at its next flush). */
int ugs_uniform_count_graphs(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                             int k, int64_t limit, int64_t *counts_out, int32_t *graph_status);
int ugs_uniform_enumerate_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                                int64_t num_graphs, int k, int mode, int64_t max_rows, int32_t *graph_status,
                                ugs_job **job_out, int64_t *total_rows_out, int64_t *total_edges_out);
int ugs_uniform_enumerate_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                                 int64_t *edge_src, int dst_is_device);
/* ---- uniform_sampler.PopulationCache: the populations S_g of a dataset's graphs, enumerated once and kept on the device; every
 *      later sample call over any batch of those graphs is served from them and runs only column buckets, draws, rows and fill.
 *      The law.  Let graph g of the batch (vertices ptr[g] ... ptr[g+1]-1) have the same vertex count and the same adjacency (as
 *      a set of undirected non-loop pairs of local vertices) as the graph added under slots[g].  Then
 *        - population_sample_begin with seeds == NULL, finished, gives the five tensors of ugs_uniform_sample_batch_begin for the same
 *          edge_index, ptr, m, mode, seed and the population's k, bit for bit;
 *        - with seeds != NULL it gives those of ugs_uniform_sample_graphs_begin, graph_status included.
 *      The draws depend on the population only through |S_g|, which the slot holds; the vertex sets come from the slot's keys; edges
 *      and edge_src come from the batch's own columns, so column order, duplicate columns, loops and columns that cross graphs are
 *      treated as the uncached call treats them (items 1 and 5 of the law of ugs_uniform_sample_batch_begin).
 *      One difference: the uncached call refuses a batch with more than 2^25 sets in all; a call served from a population holds no
 *      key array of its own and does not refuse.
 *      create(k, block_keys): no device work.  Storage is a list of device blocks of block_keys keys (1 ... 2^28) that are never moved
 *      or reallocated; a graph's keys are contiguous in one block, a graph with more keys than a block gets a block of its own.  A
 *      population belongs to the device of its first add.  destroy may be called with jobs in flight: the storage is freed when the
 *      last of them has finished.
 *      add: ugs_uniform_enumerate_begin's passes (count, scan, write, sorts; per-graph budget max_rows, 1 ... 2^25) over the given
 *      batch, then a copy of each healthy graph's sorted keys into the storage, with a 64-bit fingerprint of its adjacency bitmap.
 *      slots_out[g] is the graph's slot (slots are never reused; adding a graph again gives a new one).  graph_status[g] as
 *      enumerate_begin sets it (1: refused for its size under the limit in force, 2: more than max_rows sets of its own): such a
 *      graph gets a slot without keys, marked failed.  Healthy graphs with more than max_rows sets TOGETHER fail the call
 *      (UGS_E_UNSUPPORTED, "split the call"; nothing is added).  Synchronous.  Adds take the population's lock exclusively and never
 *      invalidate a job in flight; any number of threads may sample from one population at once.
 *      sizes: |S_g| per slot, -1 for a failed one.  info: slots, keys held, bytes and blocks allocated (any may be NULL).
 *      sample_begin checks, before any device work: every slot exists (UGS_E_BAD_ARG), ptr[g+1] - ptr[g] equals the slot's vertex
 *      count (UGS_E_BAD_ARG, naming the graph and both counts), and, with seeds == NULL, no slot is a failed one (UGS_E_UNSUPPORTED
 *      naming the graph, as the uncached call refuses it); with seeds != NULL a failed slot gives m rows of -1 and graph_status[g] = 1.
 *      check != 0 also builds the batch's adjacency bitmaps and compares each graph's fingerprint with the slot's; the outcome
 *      comes back in the status words read with the edge total, and a mismatch is UGS_E_BAD_ARG naming the first such graph.
 *      check == 0 skips that stage: for a graph that is not the slot's the result is unspecified (never a fault: only the
 *      vertex count bounds what the kernels index).  Same job protocol, stream rules and ugs_job_cancel as the other jobs;
 *      population_sample_finish takes only a population job. */
typedef struct ugs_uniform_population ugs_uniform_population;
int ugs_uniform_population_create(int k, int64_t block_keys, ugs_uniform_population **pop_out);
int ugs_uniform_population_destroy(ugs_uniform_population *pop);
int ugs_uniform_population_add(ugs_uniform_population *pop, const int64_t *edge_index, int64_t row_stride, int64_t num_cols,
                               const int64_t *ptr, int64_t num_graphs, int64_t max_rows, int64_t *slots_out, int32_t *graph_status);
int ugs_uniform_population_sizes(ugs_uniform_population *pop, const int64_t *slots, int64_t num_graphs, int64_t *sizes_out);
int ugs_uniform_population_info(ugs_uniform_population *pop, int64_t *slots_out, int64_t *keys_out, int64_t *bytes_out,
                                int64_t *blocks_out);
int ugs_uniform_population_sample_begin(ugs_uniform_population *pop, const int64_t *slots, const int64_t *edge_index,
                                        int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph,
                                        int mode, uint64_t seed, const uint64_t *seeds, int check, int32_t *graph_status,
                                        ugs_job **job_out, int64_t *total_edges_out);
int ugs_uniform_population_sample_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                                         int64_t *edge_src, int dst_is_device);
/* ---- WL class indices of a population: the vocabulary ids of the sampled subgraphs from the cache, no hashing per step.
 *      A row of the uniform sampler is one member of the fixed population S_g, and its WL digest (ugs_wl_hash below) is a function of
 *      that member and of the graph alone.  A population made by create_wl hashes every member once, when its graph is added, and
 *      keeps an int32 class index beside every key; a sample call then gathers.
 *      The law.  For a batch that passes the call's checks, population_sample_wl_begin / population_distinct_wl_begin give the
 *      tensors, graph_status and valid_out of population_sample_begin / population_distinct_begin, and d_wl_ids_out [G m] int64 equals
 *      ugs_wl_hash (populations whose adds gave no labels) or ugs_wl_hash_labeled (d_labels = L), with the population's iterations,
 *      followed by ugs_wl_lookup with the given table, over the nodes, edge_index and edge_ptr that the SAME call gives in mode 0
 *      ("sample"), where L[ptr[g] + v] is the label given for vertex v of the graph added under slots[g].  Bit for bit, for every
 *      batch composition, and whatever the call's own mode.  So a row of -1 (a failed slot with seeds, a graph with fewer than k
 *      vertices, the rows behind valid_out[g] of a distinct call) gets unknown_id, and so does a member with a start label outside
 *      [0, 2^32) (status 3).  Labels are fixed when the graph is added; nothing of the batch but its columns is read per step.
 *      Loops.  A digest depends on loop columns (item 2 of the law of ugs_wl_hash; in the labelled form a loop only makes the vertex
 *      its own neighbour), the adjacency fingerprint of a slot does not.  A WL population therefore keeps, per slot, a fingerprint of
 *      the set of vertices that have a loop column, and a _wl_begin with check != 0 compares it as well: a mismatch is UGS_E_BAD_ARG
 *      naming the first graph whose adjacency or loop set differs.  With check == 0 the ids are those of the added graph.  Calls
 *      without wl behave on a WL population exactly as on a plain one.
 *      create_wl(k, block_keys, iterations): as create; 0 <= iterations <= 8 and 1 <= k <= 32 (ugs_wl_hash's range), otherwise
 *      UGS_E_UNSUPPORTED.  No device work.
 *      add_wl: as add (which, on a WL population, is add_wl without labels), then the WL stage under the same exclusive lock: the
 *      stored members are written out as mode-0 rows with their edges by the enumeration's row and fill kernels, in chunks of at
 *      most 2^16 rows and 2^23 edge entries (under 256 MiB of scratch), each chunk is hashed by ugs_wl_hash / ugs_wl_hash_labeled,
 *      unchanged -- a stored digest is the digest of the sampler's own row, loops and duplicate columns included --, and the digests
 *      are numbered: one class per distinct digest, -1 for a member without one.  Class numbers are internal.  d_labels: DEVICE
 *      int64 [num_labels], the start label of every vertex of the call (num_labels = ptr[num_graphs], ptr[0] = 0), or NULL for the
 *      degree form; every add of one population uses the same form (UGS_E_BAD_ARG otherwise, before any device work).
 *      wl_stats: distinct digests held, rows hashed so far (add time only: a sample call hashes nothing).  wl_digests: *count_out =
 *      the number of distinct digests; if capacity >= it, digest_out [count, 2] holds them in ugs_wl_hash's format, ascending as
 *      128-bit numbers.  info's bytes include the class indices and the class table.
 *      _wl_begin: d_vocab_keys / d_vocab_ids / vocab_size / unknown_id as ugs_wl_lookup takes them (device arrays that outlive the
 *      call); vocab_token names the table: the population keeps, per token, the device array id_of_class (ugs_wl_lookup over its
 *      class table) and makes it again when the class table has grown, so equal tokens must mean equal tables.  d_wl_ids_out is a
 *      DEVICE array of G m int64, written on the job's stream before begin returns.  One more launch behind the draws
 *      (uni_pop_wl_ids: the row's draw index as the row kernels read it, cls[draw], id_of_class[cls]) and, with check, one for the
 *      loops; the outcome of that check travels in the status words read with the edge total.  UGS_E_BAD_ARG for a population made
 *      without iterations.  Finished by population_sample_finish. */
int ugs_uniform_population_create_wl(int k, int64_t block_keys, int iterations, ugs_uniform_population **pop_out);
int ugs_uniform_population_add_wl(ugs_uniform_population *pop, const int64_t *edge_index, int64_t row_stride, int64_t num_cols,
                                  const int64_t *ptr, int64_t num_graphs, int64_t max_rows, const int64_t *d_labels, int64_t num_labels,
                                  int64_t *slots_out, int32_t *graph_status);
int ugs_uniform_population_wl_stats(ugs_uniform_population *pop, int64_t *classes_out, int64_t *rows_hashed_out);
int ugs_uniform_population_wl_digests(ugs_uniform_population *pop, int64_t capacity, uint64_t *digest_out, int64_t *count_out);
int ugs_uniform_population_sample_wl_begin(ugs_uniform_population *pop, const int64_t *slots, const int64_t *edge_index,
                                           int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph,
                                           int mode, uint64_t seed, const uint64_t *seeds, int check, int32_t *graph_status,
                                           const uint64_t *d_vocab_keys, const int64_t *d_vocab_ids, int64_t vocab_size,
                                           int64_t unknown_id, uint64_t vocab_token, int64_t *d_wl_ids_out, ugs_job **job_out,
                                           int64_t *total_edges_out);
int ugs_uniform_population_distinct_wl_begin(ugs_uniform_population *pop, const int64_t *slots, const int64_t *edge_index,
                                             int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                                             int m_per_graph, int mode, const uint64_t *seeds, int check, int32_t *graph_status,
                                             int64_t *valid_out, const uint64_t *d_vocab_keys, const int64_t *d_vocab_ids,
                                             int64_t vocab_size, int64_t unknown_id, uint64_t vocab_token, int64_t *d_wl_ids_out,
                                             ugs_job **job_out, int64_t *total_edges_out);
/* Vertices per graph up to which ugs_uniform_* enumerates.  Default 64: every call behaves as it did before the wide form existed.
 * A caller whose graphs are larger (PROTEINS, IMDB-BINARY) raises it, to 1024 at most, once at start-up; nothing raises it
 * implicitly.  Results for graphs of at most 64 vertices never depend on it, and a call without wide graphs allocates and launches
 * nothing more.  Process-wide, under a mutex; a call reads it once.  Outside 64 ... 1024: UGS_E_BAD_ARG, value kept.  previous
 * may be NULL.  Initial value: UGS_UNIFORM_MAX_VERTICES in the environment, read at first use (invalid = ignored, reported under
 * UGS_DEBUG=1). */
int ugs_uniform_set_max_vertices(int n, int *previous);
int ugs_uniform_max_vertices(void);
/* Testing and measurement aid: graphs of up to this many vertices take the mask form (0 ... 64, default 64).  Below 64, smaller
 * graphs whose k fits the wide rule go through the wide kernels instead and give the same tensors; with 0 every such graph does. */
int ugs_uniform_set_mask_vertices(int n, int *previous);

/* ---- rwr_sampler.sample_batch(edge_index, ptr, m_per_graph, k, mode, seed, p_restart): replaces the reference's
 *      src/samplers/rwr_sampler/src/rwr_sampler.cpp:73-296 (random walk with restart) run with ONE OpenMP thread, its only
 *      deterministic setting (with more, the seeds and the row order depend on the schedule).
 *      The law, for each graph g in batch order, vertices [ptr[g], ptr[g+1]), n = ptr[g+1] - ptr[g]:
 *        1. adjacency (:31-71): columns in column order; a column belongs to the graph with ptr[g] <= u, v < ptr[g+1] (none:
 *           dropped); adj[u] gets v, then adj[v] gets u, so a loop puts u into adj[u] twice and duplicate columns stay;
 *        2. RNG (:17-28, :130): one SplitMix64 per graph seeded with seed + g; its draw i (1-based) is
 *           mix(seed + g + (i + 1) * 0x9e3779b97f4a7c15) mod 2^64; next_int(b) = u64 % b, next_double = (u64 >> 11) * 2^-53;
 *        3. n < k (n = 0 included): m rows of -1 without edges, no draws;
 *        4. per sample (:162-190): seed_node = next_int(n); while |chosen| < k and it < 10 n k: draw r; r < p_restart or adj[cur]
 *           empty: cur = seed_node (one draw); else cur = adj[cur][next_int(|adj[cur]|)] (a second draw); a vertex not seen
 *           before is appended to chosen.  Fewer than k vertices at the end: a row of -1 without edges, the stream goes on;
 *        5. a row holds ptr[g] + v for v in chosen order; its edges (:215-247): for u in chosen order, for v in adj[u] order with
 *           v chosen, (u, v), loops and duplicates included; mode 0 ("sample") numbers them by position in chosen, any other
 *           mode gives batch ids; edge_src is -1.  sample_ptr = [0, m, 2m, ..., G m].
 *      The whole computation runs on the device (ugs_rwr.hip): a stable half-edge sort builds the CSR, one workgroup per graph
 *      evaluates the walk at every draw offset of a window and follows the chain of real starts through it (the draws are a
 *      function of their index), and the chosen walks are run again for rows and edges.  Bit-exact.
 *      Same two-phase job protocol and stream rules as ugs_sample_batch_*; finish writes nodes[G*m,k], edge_index[2,total],
 *      edge_ptr[G*m+1], sample_ptr[G+1], edge_src[total].
 *      Errors: UGS_E_BAD_ARG for num_graphs < 0 (empty ptr), m < 0, a decreasing ptr, and the reference's checks k >= 1 and
 *      0 <= p_restart <= 1 (NaN fails); UGS_E_UNSUPPORTED for k > 64, a graph with n >= k and 10 n k > INT_MAX (the reference's
 *      int limit overflows), 2^30 columns or more, 2^31 - 1 vertices or more.  The library stays usable after any of them. */
int ugs_rwr_sample_batch_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                               int64_t num_graphs, int m_per_graph, int k, int mode, uint64_t seed, double p_restart,
                               ugs_job **job_out, int64_t *total_edges_out);
int ugs_rwr_sample_batch_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                                int64_t *edge_src, int dst_is_device);

/* ---- uniform_sampler.sample_graphs / rwr_sampler.sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode[, p_restart]): the
 *      batched form of the reference trainer's presample loop (gps/experiment.py:379-440), which calls the sampler once per graph
 *      with seed = cfg.seed + i.  Every graph g has its own generator seeds[g], so the graphs are independent.
 *      The law: graph g's block of m rows -- nodes rows [g m, (g+1) m), their edge entries, edge_ptr re-based -- equals what
 *      the matching ugs_*_sample_batch_begin gives for the same edge_index with the one-graph ptr {ptr[g], ptr[g+1]} and
 *      seed = seeds[g]: node ids are batch ids, edge_src holds batch column positions (uniform; -1 for rwr), columns outside
 *      the graph's range are dropped, both modes.  sample_ptr = [0, m, 2m, ..., G m].
 *      A graph whose one-graph call would fail with UGS_E_UNSUPPORTED does not fail this call: its block is m rows of -1 without
 *      edges, it consumes no draws, and graph_status[g] != 0 (0 for every other graph).  Those graphs are, for uniform, one of
 *      at least k vertices that ugs_uniform_sample_batch_begin refuses for its size (above), and one whose own |S_g| exceeds the 2^25 device budget; for rwr, one with
 *      n >= k and 10 n k > INT_MAX.  graph_status is a host array of num_graphs entries, written by begin.
 *      Errors of the call as a whole stay call errors: the argument errors and limits of ugs_*_sample_batch_begin (rwr: k > 64),
 *      and, for uniform, healthy graphs whose connected k-subsets TOGETHER exceed the budget (UGS_E_UNSUPPORTED; split the call).
 *      The library stays usable after any of them.  Finish with ugs_uniform_sample_batch_finish / ugs_rwr_sample_batch_finish.
 *      Uniform runs one draw workgroup per graph (its mt19937_64 in LDS) instead of sample_batch's single one; rwr only swaps the
 *      graph's seed seed + g for seeds[g]. */
int ugs_uniform_sample_graphs_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                                    int64_t num_graphs, int m_per_graph, int k, int mode, const uint64_t *seeds, int32_t *graph_status,
                                    ugs_job **job_out, int64_t *total_edges_out);
int ugs_rwr_sample_graphs_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                                int64_t num_graphs, int m_per_graph, int k, int mode, const uint64_t *seeds, double p_restart,
                                int32_t *graph_status, ugs_job **job_out, int64_t *total_edges_out);

/* ---- rwr_sampler.sample_batch / sample_graphs(..., streams="row"): random walk with restart with one generator per ROW, so that
 *      every walk is independent of every other.  The reference has no such mode; with more than one OpenMP thread it has no
 *      reproducible law at all (above).  This law is the project's own: same output distribution, reproducible, parallel by
 *      construction, and pinned to the reference row by row (below).
 *      The law is the one at ugs_rwr_sample_batch_begin with its points 1, 3, 4 and 5 unchanged (adjacency; n < k; the walk; rows,
 *      edges and sample_ptr) and this point 2.  Let sg be the graph's seed: seed + g (seeds == NULL), or seeds[g].  Row s of graph g
 *      (0 <= s < m) owns a SplitMix64 seeded with
 *          row_seed(sg, s) = mix((sg + (s + 1) * 0x9e3779b97f4a7c15) mod 2^64)
 *      which is output s of the graph's own generator in its counter form, 0-based: SplitMix's usual way of seeding children from
 *      a parent.  Output 0 is the one output the per-graph law never uses (its draws are 1-based).  The row's walk is the walk of
 *      point 4 on that stream from its first draw.  (sg + s * gamma itself would not do as a row seed: row s + 1 would then be
 *      the walk that starts one draw into row s's stream.)
 *      Consequences:
 *        - row (g, s) is bit for bit row 0 of ugs_rwr_sample_batch_begin for the same edge_index with the one-graph ptr
 *          {ptr[g], ptr[g+1]}, m = 1 and seed = row_seed(sg, s), node ids left as batch ids -- one call of the reference with one
 *          thread;
 *        - a row depends on (sg, s) and its graph only: not on m, not on other rows, and on other graphs only through the position
 *          g in seed + g.  The first m rows of a call with m' > m are the rows of the call with m;
 *        - a row whose result the law fixes without walking is written without walking, since no later row depends on its length:
 *          a seed vertex in a component of fewer than k vertices (a row of -1), and p_restart == 1.0 with k > 1 (every step
 *          restarts: every row of a graph with n >= k is -1);
 *        - edge_src is -1 and sample_ptr = [0, m, ..., G m].
 *      seeds == NULL: sg = seed + g; arguments, errors and limits of ugs_rwr_sample_batch_begin (k > 64 and a graph with n >= k
 *      and 10 n k > INT_MAX are refused); graph_status must be NULL.  seeds != NULL: sg = seeds[g] and the semantics of
 *      ugs_rwr_sample_graphs_begin: such a graph fails alone (m rows of -1, graph_status[g] != 0), graph_status is required.
 *      On the device (ugs_rwr.hip) the CSR is built as before; one kernel then walks every row, one row per lane, a workgroup
 *      serving rows of one graph from LDS.  Finish with ugs_rwr_sample_batch_finish. */
int ugs_rwr_sample_rows_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                              int64_t num_graphs, int m_per_graph, int k, int mode, uint64_t seed, const uint64_t *seeds,
                              double p_restart, int32_t *graph_status, ugs_job **job_out, int64_t *total_edges_out);

/* ---- rwr_sampler.GraphCache: the CSR of every dataset graph -- row starts, targets in (column, side) row order, doomed bytes --
 *      built once by the stages of ugs_rwr_sample_batch_begin and kept on one device; a sample call over any batch of added graphs
 *      runs only the walks, the scan and the fill.  A cache is fixed to one k: doomed[v] says "v's component has fewer than k
 *      vertices".
 *      create(k, reserve_vertices, reserve_columns): no device work; k as ugs_rwr_sample_batch_begin checks it.  The storage is
 *      allocated at the first add, on the calling thread's device, with room for at least the reservation (vertices: the graphs'
 *      vertices plus one entry per add), and grows by reallocation and a device-to-device copy to at least twice its size.  Each
 *      allocation is a generation: a job holds the one it walked on until it is finished or cancelled, so an add never invalidates
 *      a job in flight, and destroy may be called with jobs in flight.
 *      add(edge_index, ptr, G): a batch of graphs, vertices [ptr[g], ptr[g+1]).  Every column must lie inside one graph and the
 *      columns must come graph by graph, in the order of the graphs (UGS_E_BAD_ARG otherwise): each graph's columns are stored as
 *      given, in their order.  slots_out[g] is the graph's slot (never reused; adding a graph again gives a new one, the old
 *      bytes stay until destroy).  A graph with n >= k and 10 n k > INT_MAX gets a slot marked failed, status_out[g] = 1, and takes
 *      no storage.  Limits, UGS_E_UNSUPPORTED with the cache left as it was: the half-edges of all adds < 2^31 (row starts are
 *      32-bit offsets into one target array), vertices plus adds < 2^31, 2^30 columns per add.  Synchronous.  Adds are exclusive
 *      among themselves; any number of threads may sample meanwhile.
 *      info: slots, entries of the row-start array, half-edges held, bytes of the current generation, generations so far (any may
 *      be NULL).
 *      sample_begin.  THE CONTRACT.  Let B be the batch whose columns are, for g = 0 ... G-1 in order, the columns stored for
 *      slots[g], each shifted by ptr[g] -- what collating the added graphs in that order produces.  The call, finished with
 *      ugs_rwr_sample_batch_finish, gives bit for bit what these calls give on (B, ptr) with the cache's k:
 *        - seeds == NULL, row_streams == 0: ugs_rwr_sample_batch_begin (graph g seeded with seed + g, g the batch position);
 *        - seeds != NULL, row_streams == 0: ugs_rwr_sample_graphs_begin (seeds[g]);
 *        - row_streams != 0: ugs_rwr_sample_rows_begin in the matching form;
 *      all five tensors, and graph_status in the per-graph-seed forms (a failed slot: m rows of -1, graph_status[g] = 1; with
 *      seeds == NULL such a slot is UGS_E_UNSUPPORTED with the uncached call's text).  The walk, row and fill kernels are the
 *      uncached call's own: they read a graph only through its descriptor {lo, vbase, n, T}, the row starts and doomed bytes at
 *      vbase and the target array, so vbase = the slot's vertex offset in the store serves them unchanged.
 *      Before any device work: every slot exists, ptr[g+1] - ptr[g] is the slot's vertex count (UGS_E_BAD_ARG naming the graph and
 *      both counts), and, when edge_index is given or check != 0, num_cols equals the slots' column counts together
 *      (UGS_E_BAD_ARG "the batch has E columns, the added graphs have S").
 *      check != 0: the batch's edge_index goes up with the descriptors and one kernel compares every column e, of the graph g with
 *      coff[g] <= e < coff[g+1] (coff: prefix sums of the slots' column counts), with the stored column; the smallest g with a
 *      column that differs comes back in the read-back of the edge total, and the call fails with UGS_E_BAD_ARG "graph g of the
 *      batch differs from the graph added in its place".  The check is exact, not a fingerprint: it can never accept a batch that
 *      is not B.  It is stricter than the equality above needs -- it also refuses a batch whose columns are permuted in a way
 *      that leaves every adjacency row as it was (columns of different graphs interleaved, two columns without a common vertex
 *      swapped).  A failed slot stores no columns and its part of the batch is not compared: its rows are -1 whatever they are.
 *      check == 0: edge_index is not read and may be NULL (num_cols is then ignored); for a batch that is not B the result is
 *      that of B (never a fault: nothing of the batch but ptr is read).
 *      Host work is O(G); the blob holds descriptors, seeds, the check's columns and the walks' scratch -- no half-edge arrays,
 *      no sort scratch.  Same job protocol, stream rules and ugs_job_cancel as the other jobs. */
typedef struct ugs_rwr_cache ugs_rwr_cache;
int ugs_rwr_cache_create(int k, int64_t reserve_vertices, int64_t reserve_columns, ugs_rwr_cache **cache_out);
int ugs_rwr_cache_destroy(ugs_rwr_cache *cache);
int ugs_rwr_cache_add(ugs_rwr_cache *cache, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                      int64_t num_graphs, int64_t *slots_out, int32_t *status_out);
int ugs_rwr_cache_info(ugs_rwr_cache *cache, int64_t *graphs_out, int64_t *vertices_out, int64_t *half_edges_out, int64_t *bytes_out,
                       int64_t *generations_out);
int ugs_rwr_cache_sample_begin(ugs_rwr_cache *cache, const int64_t *slots, const int64_t *edge_index, int64_t row_stride,
                               int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode, uint64_t seed,
                               const uint64_t *seeds, double p_restart, int row_streams, int check, int32_t *graph_status,
                               ugs_job **job_out, int64_t *total_edges_out);

/* ---- ugs_sampler.GraphCache (ugs_graph_cache_*): every graph of a dataset preprocessed once, at one k, and kept on one device as
 *      one "plan of all added graphs" -- row pointer, (neighbour, rank) and (neighbour, column) entries, root records, viable lists --
 *      so that a sample call over any batch of added graphs runs only the walks, the scan and the fill.
 *      create(k, reserve_vertices, reserve_columns): no device work; k as ugs_sample_batch_begin checks it (k > 32: UGS_E_UNSUPPORTED
 *      "k > 32 is not supported by the HIP sampler").  The storage is allocated at the first add, on the calling thread's device, with
 *      room for at least the reservation, and grows by reallocation and a device-to-device copy to at least twice its size.  Each
 *      allocation is a generation: a job holds the one it walks on until it is finished or cancelled, so an add never invalidates a
 *      job in flight, and destroy may be called with jobs in flight.
 *      add(edge_index, ptr, G): a batch of graphs, vertices [ptr[g], ptr[g+1]).  Every column must lie inside one graph and the
 *      columns must come graph by graph, in the order of the graphs (UGS_E_BAD_ARG otherwise): each graph's columns are stored as
 *      given, in their order, as pairs of local ids.  Each graph is preprocessed on its own content at the cache's k by the stages
 *      an LRU miss of ugs_sample_batch_begin runs -- without reading or changing the LRU, the handle registry, the plan cache or the
 *      batch index: ugs_cache_stats is the same before and after.  A graph with n <= 0 or n < k keeps a slot and its columns and
 *      nothing else (m rows of -1, as in a batch).  slots_out[g] is the graph's slot (never reused; adding a graph again gives a
 *      new one, the old bytes stay until destroy).  Limits, UGS_E_UNSUPPORTED with the cache left as it was: the CSR entries of all
 *      adds < 2^31 - 1, the columns of all adds < 2^31 - 1.  Synchronous.  Adds are exclusive among themselves; any number of threads
 *      may sample meanwhile.
 *      info: slots, root records (vertices of the non-degenerate graphs), CSR entries, bytes of the current generation, generations
 *      so far (any may be NULL).
 *      sample_begin.  THE CONTRACT.  Let B be the batch whose columns are, for g = 0 ... G-1 in order, the columns stored for
 *      slots[g], each shifted by ptr[g] -- what collating the added graphs in that order produces.  The call, finished with
 *      ugs_sample_batch_finish, gives bit for bit what, after ugs_cache_clear, ugs_sample_batch_begin (seeds == NULL) or
 *      ugs_sample_graphs_begin (seeds != NULL: num_graphs C ints) gives on (B, ptr) with the cache's k, mode and seed, in all five
 *      tensors.  The walk, scan and fill kernels are the uncached call's own, code and argument layout: they reach a graph only
 *      through its descriptor {node_lo, rbase, vbase, viable_base, n, level, n_viable}, and a row's generator is keyed by the seed
 *      and the row's index inside its graph, so a descriptor whose bases point into the store serves them.  The store keeps a
 *      graph's columns numbered from 0; one small kernel behind the fill adds coff[g], the number of columns of the graphs ahead of
 *      g in the batch, to the edge_src entries of g's rows.
 *      THE DEVIATION.  The call never reads or changes the LRU, so it does not reproduce the reference's reuse of ANOTHER graph's
 *      preprocessing: a graph the LRU holds under a different k (the key ignores k), and two different graphs of more than 1000
 *      columns that share a strided key (include/cache.hpp:100-107).  Every graph gets the preprocessing of its own content at the
 *      cache's k, whatever the LRU holds -- which is what the uncached call gives on an empty LRU, except for the second case inside
 *      one batch.
 *      Before any device work: every slot exists, ptr[g+1] - ptr[g] is the slot's vertex count (UGS_E_BAD_ARG naming the graph and
 *      both counts), and, when edge_index is given or check != 0, num_cols equals the slots' column counts together
 *      (UGS_E_BAD_ARG "the batch has E columns, the added graphs have S").
 *      check != 0: the batch's edge_index goes up with the descriptors and one kernel compares every column e, of the graph g with
 *      coff[g] <= e < coff[g+1], with the stored column, exactly; the smallest g with a column that differs reaches the host ahead
 *      of the edge total, without a wait of its own, and the call fails with UGS_E_BAD_ARG "graph g of the batch differs from the
 *      graph added in its place".  It can never accept a batch that is not B; it also refuses a batch that merely permutes a
 *      graph's columns (edge_src would differ).  check == 0: edge_index is not read and may be NULL (num_cols is then ignored); for
 *      a batch that is not B the result is that of B (never a fault: nothing of the batch but ptr is read).
 *      Host work is O(G).  Padded rows and the first-pick table are not built for the store: a call whose tier has 64 lanes per walk
 *      reads rows through the row pointer.  Same job protocol, stream rules and ugs_job_cancel as the other jobs.
 *      last_launch: the names of the first-tier walk kernel and of the fill kernel of the calling thread's last sample call on this
 *      cache ("" if there was none, or no fill ran) -- a read-only aid like ugs_plan_last_launch / ugs_plan_last_fill. */
typedef struct ugs_graph_cache ugs_graph_cache;
int ugs_graph_cache_create(int k, int64_t reserve_vertices, int64_t reserve_columns, ugs_graph_cache **cache_out);
int ugs_graph_cache_destroy(ugs_graph_cache *cache);
int ugs_graph_cache_add(ugs_graph_cache *cache, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                        int64_t num_graphs, int64_t *slots_out);
int ugs_graph_cache_info(ugs_graph_cache *cache, int64_t *graphs_out, int64_t *vertices_out, int64_t *entries_out, int64_t *bytes_out,
                         int64_t *generations_out);
int ugs_graph_cache_sample_begin(ugs_graph_cache *cache, const int64_t *slots, const int64_t *edge_index, int64_t row_stride,
                                 int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode, int seed,
                                 const int32_t *seeds, int check, ugs_job **job_out, int64_t *total_edges_out);
int ugs_graph_cache_last_launch(ugs_graph_cache *cache, char *walk_buf, int walk_buf_len, char *fill_buf, int fill_buf_len);

/* ---- epsilon_uniform_sampler.GraphCache (ugs_eps_cache_*): the adjacency lists of every graph of a dataset -- what
 *      ugs_eps_sample_batch_begin builds on the host for every batch -- built once, by a kernel, and kept on one device, so that a
 *      sample call over any batch of added graphs runs only the walks, the scan and the fill.  The lists depend on neither k nor
 *      epsilon: one cache serves every value of both, and they are arguments of the call.
 *      create(reserve_vertices, reserve_columns): no device work.  The storage is allocated at the first add, on the calling
 *      thread's device, with room for at least the reservation (vertices: the graphs' vertices plus one entry per graph), and
 *      grows by reallocation and a device-to-device copy to at least twice its size.  Each allocation is a generation: a job holds
 *      the one it walked on until it is finished or cancelled, so an add never invalidates a job in flight, and destroy may be
 *      called with jobs in flight.
 *      add(edge_index, ptr, G): a batch of graphs, vertices [ptr[g], ptr[g+1]).  Every column must lie inside one graph and the
 *      columns must come graph by graph, in the order of the graphs (UGS_E_BAD_ARG otherwise): each graph's columns are stored as
 *      given, in their order, as pairs of local ids.  The columns go up and one kernel writes, behind everything the store holds,
 *      per graph n + 1 row offsets and per column two entries (neighbour, 2 * column inside the graph + side): THE ROW ORDER -- inside a
 *      vertex's row the half-edges stand in (column, side) order, the source side (side 0) before the destination side, and a loop
 *      column puts both its half-edges into the same row, source side first -- is that of the lists the uncached call builds.
 *      slots_out[g] is the graph's slot (never reused; adding a graph again gives a new one, the old bytes stay until destroy).
 *      Limits, UGS_E_UNSUPPORTED with the cache left as it was: the half-edges of all adds < 2^31, vertices plus graphs of all adds
 *      < 2^31, 2^30 columns per add.  Synchronous.  Adds are exclusive among themselves; any number of threads may sample meanwhile.
 *      info: slots, row-offset entries (vertices plus one per graph), half-edges held, bytes of the current generation, generations
 *      so far (any may be NULL).
 *      graph_csr: one slot's rows copied back from HBM (read-only, diagnostic: the counterpart of ugs_plan_graph_csr).  rowptr:
 *      num_nodes + 1 values relative to the graph's first entry; per entry the neighbour (local id) and 2 * (column inside the
 *      graph) + side.  rowptr holds node_capacity + 1 values, the entry arrays entry_capacity (UGS_E_CAPACITY if too small, with
 *      both counts reported); any pointer may be NULL.  Synchronises with the device.
 *      sample_begin.  THE CONTRACT.  Let B be the batch whose columns are, for g = 0 ... G-1 in order, the columns stored for
 *      slots[g], each shifted by ptr[g] -- what collating the added graphs in that order produces.  The call, finished with
 *      ugs_eps_sample_batch_finish, gives bit for bit what ugs_eps_sample_batch_begin (seeds == NULL: `seed` keys every row) or
 *      ugs_eps_sample_graphs_begin (seeds != NULL: num_graphs values; graph_status, if given, is written all zero) gives on
 *      (B, ptr) with the same m_per_graph, k, mode and epsilon, in all five tensors.  The walk kernel is the uncached call's own:
 *      it reaches a graph only through its descriptor {node_lo, rbase, n}, the row offsets and the two entry arrays, and a row's
 *      generator is keyed by the seed and the row's index, so a descriptor whose rbase points into the store serves it.  A stored
 *      row names columns inside its graph; the fill adds coff[g], the number of columns of the graphs ahead of g in the batch,
 *      when it writes edge_src (the uncached fill is the same kernel compiled without that addition).
 *      Same checks and texts as ugs_eps_sample_batch_begin for epsilon, m_per_graph and k, before any device work; also before any:
 *      every slot exists, ptr[g+1] - ptr[g] is the slot's vertex count (UGS_E_BAD_ARG naming the graph and both counts), and, when
 *      edge_index is given or check != 0, num_cols equals the slots' column counts together (UGS_E_BAD_ARG "the batch has E columns,
 *      the added graphs have S").
 *      check != 0: the batch's edge_index goes up with the descriptors and one kernel compares every column e, of the graph g with
 *      coff[g] <= e < coff[g+1], with the stored column, exactly; the smallest g with a column that differs comes back in the
 *      read-back of the edge total, and the call fails with UGS_E_BAD_ARG "graph g of the batch differs from the graph added in its
 *      place".  It can never accept a batch that is not B; it also refuses a batch that merely permutes a graph's columns (edge_src
 *      would differ).  check == 0: edge_index is not read and may be NULL (num_cols is then ignored); for a batch that is not B the
 *      result is that of B (never a fault: nothing of the batch but ptr is read).
 *      Host work is O(G); the blob holds descriptors, coff, seeds, the check's columns and the walks' scratch -- no adjacency.  Same
 *      job protocol, stream rules and ugs_job_cancel as the other jobs. */
typedef struct ugs_eps_cache ugs_eps_cache;
int ugs_eps_cache_create(int64_t reserve_vertices, int64_t reserve_columns, ugs_eps_cache **cache_out);
int ugs_eps_cache_destroy(ugs_eps_cache *cache);
int ugs_eps_cache_add(ugs_eps_cache *cache, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                      int64_t num_graphs, int64_t *slots_out);
int ugs_eps_cache_info(ugs_eps_cache *cache, int64_t *graphs_out, int64_t *vertices_out, int64_t *half_edges_out, int64_t *bytes_out,
                       int64_t *generations_out);
int ugs_eps_cache_graph_csr(ugs_eps_cache *cache, int64_t slot, int64_t node_capacity, int64_t entry_capacity, int64_t *num_nodes,
                            int64_t *num_entries, int64_t *rowptr, int32_t *nbr, int32_t *ecs);
int ugs_eps_cache_sample_begin(ugs_eps_cache *cache, const int64_t *slots, const int64_t *edge_index, int64_t row_stride,
                               int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph, int k, int mode, uint64_t seed,
                               const uint64_t *seeds, double epsilon, int check, int32_t *graph_status, ugs_job **job_out,
                               int64_t *total_edges_out);

/* ---- uniform_sampler.sample_distinct(edge_index, ptr, m_per_graph, k, seeds, mode) / PopulationCache.sample_distinct: sampling
 *      WITHOUT replacement from the finite population S_g -- m distinct connected k-subsets per graph, every ordered selection
 *      equally likely, and the whole population, in its order, when it has at most m sets (the "full bag": no sampling variance
 *      left).  The reference has no such mode; this law is the project's own, and it is counter-based.
 *      The law.  mix(z) is SplitMix64's finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *      z ^= z >> 31.  gamma = 0x9E3779B97F4A7C15.  All arithmetic mod 2^64.  Graph g has N = |S_g| sets in the population order of
 *      ugs_uniform_enumerate_begin (item 2 of the law of ugs_uniform_sample_batch_begin), the seed s = seeds[g], and m rows:
 *        - N <= 0 (k = 0, n < k, a graph refused for its size or with more sets than the budget / max_rows: graph_status[g] != 0 for
 *          the last two): m rows of -1, nothing consumed, as ugs_uniform_sample_graphs_begin does;
 *        - m >= N: rows 0 ... N-1 are the population indices 0 ... N-1 -- the rows ugs_uniform_enumerate_begin gives for the graph --
 *          and rows N ... m-1 are rows of -1;
 *        - m < N: a partial Fisher-Yates shuffle of the virtual identity array a[0 ... N-1].  For j = 0 ... m-1:
 *          r_j = the high 64 bits of the 128-bit product mix(mix(s) + (j+1) gamma) * (N - j);  t_j = j + r_j;  swap a[j] and a[t_j];
 *          row j is population index a[j].  There is no rejection step: the multiply-high maps 2^64 values onto N - j, so an outcome's
 *          probability is off by less than (N - j) / 2^64 < 2^-39 for N <= 2^25, far below what any test of m rows can see.
 *      The rows of a graph are distinct sets; row j depends only on (s, N) and the steps up to j, so a call with a smaller m gives a
 *      prefix.  A row with population index d is written exactly as the row a draw d gives in ugs_uniform_sample_graphs_begin
 *      (items 4 and 5 of that law); a row of -1 has no edges.  sample_ptr = [0, m, 2m, ..., G m].  valid_out[g] = min(m, max(N, 0)):
 *      the rows of graph g that are real, always its first ones.  valid_out and graph_status are host arrays of num_graphs entries
 *      written by begin; the population sizes come back with the status words that travel with the edge total (uncached) or are
 *      known from the slots (cached), so neither call has a read-back of its own for them.
 *      Limit: m_per_graph <= 4096 (UGS_E_UNSUPPORTED before any device work): one workgroup per graph (uni_draw_distinct) sorts the
 *      keys (t_j << 32) | j in LDS -- 32 KiB at the limit -- and reads "a[t_j] as the earlier steps left it" off the sorted keys
 *      (DESIGN.md section 10.3); there is no global-memory fallback.
 *      ugs_uniform_distinct_begin is ugs_uniform_sample_graphs_begin with these draws: it enumerates on the call, has the same
 *      argument errors, budget and per-graph failures, and is finished by ugs_uniform_sample_batch_finish.
 *      ugs_uniform_population_distinct_begin is ugs_uniform_population_sample_begin (seeds != NULL) with these draws: same slot,
 *      vertex-count and adjacency checks, under the population's shared lock, finished by ugs_uniform_population_sample_finish.
 *      With equal seeds the two give identical tensors, graph_status and valid_out.  ugs_sample_batch_finish takes either job.
 *      Own refusals, checked first: m_per_graph < 0, m_per_graph > 4096, and (num_graphs > 0) a NULL seeds, graph_status or valid_out. */
int ugs_uniform_distinct_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                               int m_per_graph, int k, int mode, const uint64_t *seeds, int32_t *graph_status, int64_t *valid_out,
                               ugs_job **job_out, int64_t *total_edges_out);
int ugs_uniform_population_distinct_begin(ugs_uniform_population *pop, const int64_t *slots, const int64_t *edge_index,
                                          int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph,
                                          int mode, const uint64_t *seeds, int check, int32_t *graph_status, int64_t *valid_out,
                                          ugs_job **job_out, int64_t *total_edges_out);

/* ---- apx_ugs_sampler.sample_batch(edge_index, ptr, m_per_graph, k, mode, seed, epsilon): replaces the reference's
 *      src/samplers/apx_ugs_sampler/src/apx_ugs_sampler.cpp:461-519.  First graph only;
 *      ptr[0]:ptr[1] is a range of edge COLUMNS (:15-33).  The reference draws everything from ONE sequential
 *      std::mt19937_64 stream, which has no parallel bit-exact form: this entry point is a HOST computation that consumes the
 *      same generator in the same order (bit-exact on the same toolchain).  It is not part of the GPU hot path.
 *      samples_out: capacity m_per_graph * k int64, sample s at samples_out[s*k .. s*k+k); *num_samples_out = S <= m_per_graph
 *      (failed samples are dropped, like the reference). */
int ugs_apx_sample_batch(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t ptr_len,
                         int m_per_graph, int k, uint64_t seed, double epsilon, int64_t *samples_out, int64_t *num_samples_out);

/* GPU variant of the same entry point: the same algorithm with one generator per (sample, trial) -- all samples and thousands of
 * trials run side by side, a sample's result is its accepted trial with the smallest index (deterministic in (graph, seed)).
 * Parity with the reference is statistical (same output law), not bit-wise.  2 <= k <= 8.
 * order_pos_out / est_out (optional, capacity order_capacity >= number of vertices): position of every vertex in the APX-DD order
 * and its bucket estimate, for the law check of the tests. */
int ugs_apx_gpu_sample_batch(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t ptr_len,
                             int m_per_graph, int k, uint64_t seed, double epsilon, int64_t *samples_out, int64_t *num_samples_out,
                             int32_t *order_pos_out, double *est_out, int64_t order_capacity);

/* ---- ugs_sampler.wl: Weisfeiler-Lehman graph hashes and vocabulary ids of sampled subgraphs (ugs_wl.hip) -- replaces the host loop
 *      of the reference's SS-GNN-WL consumer (src/gps/gps/models/ss_gnn_wl.py:210-247, src/gps/gps/utils/wl_vocab.py:21-67), which
 *      builds one networkx.Graph per sample, gives every vertex the attribute str(degree) and calls
 *      weisfeiler_lehman_graph_hash(G, node_attr='attr', iterations).  The digests are those of networkx 3.4.2, bit for bit.
 *      The law, for row i of nodes [rows, k] (any values) with the entries [edge_ptr[i], edge_ptr[i+1]) of edge_index:
 *        1. n = number of entries >= 0 in the row; the graph has the vertices 0 .. n-1;
 *        2. every entry e contributes the undirected edge {edge_index[0,e], edge_index[1,e]}: duplicates and reversed copies collapse,
 *           a loop (u,u) makes u its own neighbour once and counts 2 towards its degree (networkx.Graph);
 *        3. n = 0: status 1, no digest (the reference answers "unknown id" for such a row);
 *        4. an endpoint outside [0, n), or an edge_ptr range that is no range of [0, num_cols]: status 2, no digest.  THE ONE
 *           DEVIATION: the reference catches the KeyError networkx raises there and hashes a fallback string
 *           "deg_<sum>_edges_<count>"; no sampler of this library produces such a row in mode "sample";
 *        5. otherwise status 0 and: label[u] = str(deg u) in decimal; for t = 1 .. iterations:
 *           msg[u] = label[u] + "".join(sorted(label[v] for v in N(u))) -- Python STRING order, "10" < "2" --,
 *           label'[u] = blake2b(msg[u], digest_size=16).hexdigest() (unkeyed BLAKE2b, RFC 7693; 32 lowercase hex characters), and
 *           sorted(Counter(label').items()) is appended to a list `items`; the result is
 *           blake2b(str(tuple(items)), digest_size=16): items print as ('<32 hex>', <count>), joined by ", " inside one pair of
 *           parentheses, a single item gets a trailing comma "(('..', 2),)", iterations = 0 hashes "()".
 *      digest [rows, 2] uint64: bytes 0-7 and 8-15 of the digest as big-endian numbers (the hex string is "%016x%016x" of the two),
 *      zero where status != 0; status [rows] int32.  All pointers are DEVICE pointers.  1 <= k <= 32, 0 <= iterations <= 8, otherwise
 *      UGS_E_UNSUPPORTED.  This is the degree-labelled form (use_node_features_in_wl = false); ugs_wl_hash_labeled below is the
 *      node-feature form.  Edge attributes and weisfeiler_lehman_subgraph_hashes are not covered.
 *      One launch on the calling thread's stream (ugs_set_stream), no allocation, no synchronisation with the host. */
int ugs_wl_hash(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                const int64_t *d_edge_ptr, int64_t rows, int k, int iterations, uint64_t *d_digest, int32_t *d_status);
/* The node-feature form (use_node_features_in_wl = true; compute_wl_hash with node_features, wl_vocab.py:21-67, on the rows
 * extract_subgraph_from_batch cuts out, wl_vocab.py:70-107).  The law of ugs_wl_hash holds except for the start labels:
 *   a. label32(i) = the first four bytes of MD5(bytes of feature row i) (RFC 1321) as a big-endian number, i.e.
 *      int(hashlib.md5(x[i].numpy().tobytes()).hexdigest()[:8], 16); a row of zero bytes gives 0xd41d8cd9.  ugs_wl_feature_labels
 *      writes it, as int64, for num_rows rows of row_bytes bytes each, row i starting at d_x + i * row_stride_bytes (any byte
 *      alignment).  0 <= row_bytes < 2^29 (otherwise UGS_E_UNSUPPORTED), row_stride_bytes >= row_bytes, num_rows >= 0.
 *   b. the vertices of a row of nodes are its entries >= 0 in row order: vertex j is the j-th such entry, so an entry of -1 in the
 *      middle shifts the later vertices down (subgraph_nodes[valid_mask]); a duplicated id is two vertices with one label.  The
 *      start label of vertex j is "%08x" % d_labels[nodes[row, slot_j]]: 8 lowercase hex characters, whose string order is the
 *      numeric order of the 32-bit values.  From there on: msg[u] = label[u] + sorted neighbour labels, BLAKE2b-128 hex, Counter
 *      items, final string, as in 5. above.  There is no degree in this form: a loop only makes u its own neighbour.
 *      iterations = 0 still hashes "()".
 *   c. statuses 0, 1 and 2 as in ugs_wl_hash (a row with a bad endpoint is 2 whatever its labels); status 3, no digest: an entry
 *      >= num_labels, or a label outside [0, 2^32) -- the reference raises IndexError for the former.  Other rows are not disturbed.
 * d_labels [num_labels] int64 need not come from ugs_wl_feature_labels: any 32-bit categorical labels do.  All pointers are DEVICE
 * pointers; each function makes one launch on the calling thread's stream, allocates nothing and does not synchronise with the host. */
int ugs_wl_feature_labels(const void *d_x, int64_t row_bytes, int64_t row_stride_bytes, int64_t num_rows, int64_t *d_labels);
int ugs_wl_hash_labeled(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                        const int64_t *d_edge_ptr, int64_t rows, int k, int iterations, const int64_t *d_labels, int64_t num_labels,
                        uint64_t *d_digest, int32_t *d_status);
/* Vocabulary ids of digests (hash_to_id, wl_vocab.py:205-216): d_keys [vocab_size, 2] holds the vocabulary's digests in the form
 * above, ascending as 128-bit numbers and distinct, d_ids [vocab_size] their ids.  ids_out[i] = the id of digest i, or unknown_id
 * when it is not in the table or status[i] != 0.  Same stream rule; one launch, no allocation, no synchronisation. */
int ugs_wl_lookup(const uint64_t *d_digest, const int32_t *d_status, int64_t rows, const uint64_t *d_keys, const int64_t *d_ids,
                  int64_t vocab_size, int64_t unknown_id, int64_t *d_ids_out);

/* ---- ugs_sampler.rows.unique_rows: the repeated subgraphs of a sampler's output merged per graph, on the device -----------------
 * The inputs are the five tensors of any sampler here (or of PresampleCache.load): nodes [R, k], edge_index [2, Es] with rows
 * `in_stride` apart, edge_ptr [R + 1], sample_ptr [G + 1], edge_src [Es] (or NULL: then edge_src_u is not written), and the batch's
 * ptr [G + 1].  All pointers are DEVICE pointers.  THE LAW:
 *   1. Rows sample_ptr[g] .. sample_ptr[g+1]-1 belong to graph g.  The KEY of a row is its k entries in order (by = 0, "sequence")
 *      or sorted ascending (by = 1, "set").  An entry -1 is a value like any other: the all -1 placeholder rows of one graph merge.
 *   2. Row r is KEPT iff no row r' < r of the same graph has the same key.  Rows of different graphs never merge.
 *   3. The kept rows keep their relative order and are copied unchanged: their nodes row as it stands (not sorted), their span
 *      edge_ptr[r] .. edge_ptr[r+1]-1 of both rows of edge_index and of edge_src (the values untouched: every sampling mode works).
 *      edge_ptr_u [U + 1] and sample_ptr_u [G + 1] are the new prefix sums; a graph without rows keeps an empty span.
 *   4. count[u] is the number of original rows whose key equals kept row u's; inverse[r] is the position in the result of the kept
 *      row with r's key.  Hence inverse of a kept row is its own new position, count sums to R, and nodes_u[inverse] has the keys
 *      of nodes.
 *   5. The result does not depend on the launch shape, and repeated calls are bit-identical.
 * Keys are exact, not hashes: an entry v of graph g is coded as v - ptr[g] + 1 (0 for -1) in b = min(31, floor(128 / k)) bits of
 * one 128-bit word.  Limits: 1 <= k <= 32; ptr[g+1] - ptr[g] + 1 <= 2^b for every graph with rows; at most 4096 rows per graph;
 * R < 2^31, G < 2^31.
 * begin checks on the device, before anything is indexed by them: sample_ptr and edge_ptr start at 0, do not decrease and end at R
 * and at num_edges (Es); ptr does not decrease; every graph with rows is within the limits; every entry is -1 or inside
 * [ptr[g], ptr[g+1]).  A call that fails one of these returns UGS_E_BAD_ARG (UGS_E_UNSUPPORTED for a limit) with a message that
 * names the first offending index, graph or row, makes no job and leaves the library as it was.  Otherwise begin reports U and Eu
 * (one read-back) and the caller allocates nodes_u [U, k], edge_index_u [2, ld >= Eu], edge_ptr_u [U + 1], sample_ptr_u [G + 1],
 * edge_src_u [Eu], count [U], inverse [R]; finish writes them on the job's stream, waits for it as every finish does (the scratch
 * goes back to the pool) and frees the job.  The inputs must stay alive and unchanged from begin to finish;
 * ugs_job_cancel(job) gives the job up instead.  The scratch comes from the library's pool.
 * ugs_rows_last_launch: the dedup kernel forms of the calling thread's last begin -- "wave" (graphs of at most 64 rows, one wave
 * each), "workgroup" (65..4096 rows, one workgroup each, sorted in LDS), "wave+workgroup", or "none". */
int ugs_rows_unique_begin(const int64_t *d_nodes, int k, int64_t num_rows, const int64_t *d_edge_ptr, int64_t num_edges,
                          const int64_t *d_sample_ptr, int64_t num_graphs, const int64_t *d_ptr, int by, ugs_job **job_out,
                          int64_t *unique_rows_out, int64_t *unique_edges_out);
int ugs_rows_unique_finish(ugs_job *job, int64_t *d_nodes_u, const int64_t *d_edge_index_in, int64_t in_stride, const int64_t *d_edge_src_in,
                           int64_t *d_edge_index_u, int64_t ld, int64_t *d_edge_ptr_u, int64_t *d_sample_ptr_u, int64_t *d_edge_src_u,
                           int64_t *d_count, int64_t *d_inverse);
int ugs_rows_last_launch(char *buf, int buf_len);

/* ---- ugs_sampler.graphlets: the exact isomorphism class of every sampled subgraph (ugs_graphlet.hip, ugs_graphlet.cpp) -----------
 *      What the WL digest above stands in for, computed itself: a graph on n <= 8 vertices is 28 adjacency bits, and there are
 *      1, 2, 4, 11, 34, 156, 1044, 12346 graphs on 1 .. 8 vertices, so the complete vocabulary is a fixed table.
 *      The law, for row i of nodes [rows, k] (any values) with the entries [edge_ptr[i], edge_ptr[i+1]) of edge_index:
 *        1. items 1, 3 and 4 of ugs_wl_hash's law: n = number of entries >= 0 in the row, the graph has the vertices 0 .. n-1;
 *           n = 0: status 1; an endpoint outside [0, n), or an edge_ptr range that is no range of [0, num_cols]: status 2 (nothing
 *           of such a range is read).  Other rows are not disturbed;
 *        2. the graph is SIMPLE: every entry contributes the undirected pair {u, v}, duplicates and reversed copies collapse, and a
 *           loop (u, u) is dropped -- the one difference from WL's reading of the same row;
 *        3. pair (i, j), i < j, has bit position b(i, j) = j (j - 1) / 2 + i: the adjacency among the first n - 1 vertices is the
 *           low bits, the last vertex's neighbours are the top n - 1;
 *        4. for a permutation p of the n vertices, code(p) = sum of A[p(i), p(j)] << b(i, j);
 *        5. the CANONICAL CODE is the minimum of code(p) over all n! permutations;
 *        6. the row's KEY is (n << 28) | canonical code, as int64; -1 where status != 0;
 *        7. the CLASS ID is the rank of the key in the ascending list of all keys with 1 <= n' <= 8.  It does not depend on k: the
 *           ids of graphs on at most k vertices fill [0, C_k), C_k = 1, 3, 7, 18, 52, 208, 1252, 13598 for k = 1 .. 8.  A row with
 *           status != 0 gets the id C_k (the len(vocab) convention of the WL vocabulary).
 *      1 <= k <= 8, otherwise UGS_E_UNSUPPORTED.
 * ugs_graphlet_canon: all pointers are DEVICE pointers.  key_out [rows] int64, status_out [rows] int32.  d_table and d_class_out may
 *      both be NULL; otherwise d_table [table_len] is the ascending key table for n <= k (ugs_graphlet_table for n = 1 .. k, one
 *      after the other) and class_out [rows] receives the ids, table_len for a row with status != 0, in the same launch.  One launch
 *      on the calling thread's stream (ugs_set_stream), no allocation, no synchronisation with the host; rows = 0 is a no-op.
 * ugs_graphlet_table: HOST function, no device work.  *count_out = the number of graphs on exactly n vertices; if capacity >= it,
 *      keys_out holds their keys, ascending.  Built once per process and per n, under a mutex, by extending every (n-1)-class with
 *      a last vertex over all 2^(n-1) neighbour sets and canonicalising; item 3's layout makes that complete.
 * ugs_graphlet_canon_code: HOST function, the canonicaliser the table is built with and the same search the kernel runs:
 *      *out = the canonical code of the graph whose adjacency bits are `code` (bits above n (n - 1) / 2: UGS_E_BAD_ARG).
 * ugs_graphlet_search_stats: HOST function, the cost of that search for `code`: the complete codes it compares (1 for a graph
 *      without symmetry, 48 for the cube) and the search nodes it evaluates (n - 1 at the least). */
int ugs_graphlet_canon(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                       const int64_t *d_edge_ptr, int64_t rows, int k, const int64_t *d_table, int64_t table_len,
                       int64_t *d_key_out, int32_t *d_status_out, int64_t *d_class_out);
int ugs_graphlet_table(int n, int64_t *keys_out, int64_t capacity, int64_t *count_out);
int ugs_graphlet_canon_code(uint32_t code, int n, uint32_t *out);
int ugs_graphlet_search_stats(uint32_t code, int n, uint32_t *leaves_out, uint32_t *nodes_out);

/* ---- graphlets.orbit_ids: where every vertex of a row sits inside its class -- its automorphism orbit (centre or leaf of a star, end
 *      or middle of a path, triangle corner or tail of a paw).  Items 1 - 7 of ugs_graphlet_canon's law hold unchanged: vertices, n,
 *      statuses 0 / 1 / 2, the simple graph, the bit layout, the code of a permutation, key and class id.  Then:
 *        1. vertex j of a row is its j-th entry >= 0 in row order: an entry of -1 in the middle shifts the later vertices down, and a
 *           repeated id is two vertices;
 *        2. the ROOTED CODE of vertex v is the minimum of code(p) over the (n - 1)! permutations p with p(n - 1) = v; 0 for n = 1.  It
 *           does not depend on the labelling; u and v lie in one orbit of the automorphism group exactly when their rooted codes are
 *           equal; the minimum over v is the canonical code;
 *        3. the orbits of a class are numbered by ascending rooted code: the LOCAL INDEX of v is the number of distinct rooted codes of
 *           the row below v's.  The root's column is 2^deg - 1, so orbits come in order of degree first;
 *        4. the ORBIT ID is base[class id] + local index, base being the exclusive prefix sum of the orbit counts over all classes in
 *           key order.  It does not depend on k: the ids of graphs on at most k vertices fill [0, O_k),
 *           O_k = 1, 3, 9, 29, 119, 663, 5759, 85023 for k = 1 .. 8 (connected graphs on exactly k vertices: 1, 1, 3, 11, 58, 407,
 *           4306, 72489 orbits; 1 + 3 + 11 + 58 = 73 are the orbits of the graphlets on 2 .. 5 vertices);
 *        5. orbit_out [rows, k] int64: slot s holds the orbit id of the vertex that slot s is, O_k where the entry is < 0 and in
 *           every slot of a row with status != 0.  Other rows are not disturbed.
 *      1 <= k <= 8, otherwise UGS_E_UNSUPPORTED.  The numbering is this library's own.
 * ugs_graphlet_orbits: all pointers are DEVICE pointers.  d_table [table_len] as for ugs_graphlet_canon (needed: the id is found
 *      through the class), d_base [table_len + 1] the prefix sums of item 4 (ugs_graphlet_orbit_counts for n = 1 .. k summed up, the
 *      last entry being O_k).  d_key_out, d_status_out and d_class_out may each be NULL; where given they receive what
 *      ugs_graphlet_canon writes, bit for bit, in the same launch.  One launch on the calling thread's stream, no allocation, no
 *      synchronisation with the host; rows = 0 is a no-op.
 * ugs_graphlet_rooted_codes: HOST function.  out[v], v < n, = the rooted code of vertex v of the graph whose adjacency bits are `code`
 *      (bits above n (n - 1) / 2: UGS_E_BAD_ARG), by the search the kernel runs; out[v] = 0xffffffff for n <= v < 8.
 * ugs_graphlet_orbit_counts: HOST function, no device work.  *count_out = the number of graphs on exactly n vertices; if capacity >=
 *      it, counts_out[i] = the number of orbits of class i of ugs_graphlet_table(n).  Built once per process and n under the
 *      table's mutex. */
int ugs_graphlet_orbits(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                        const int64_t *d_edge_ptr, int64_t rows, int k, const int64_t *d_table, const int64_t *d_base, int64_t table_len,
                        int64_t *d_orbit_out, int64_t *d_key_out, int32_t *d_status_out, int64_t *d_class_out);
int ugs_graphlet_rooted_codes(uint32_t code, int n, uint32_t *out);
int ugs_graphlet_orbit_counts(int n, int64_t *counts_out, int64_t capacity, int64_t *count_out);

/* ---- graphlets.labelled_keys: the exact class of every row as a NODE-LABELLED graph (use_node_features_in_wl), and the orbits of the
 *      label-preserving automorphism group.  Two rows of one shape with different labels -- two molecule fragments with different
 *      atoms -- are different classes.  Items 1 - 6 of ugs_graphlet_canon's law hold unchanged: vertices, n, statuses 0 / 1 / 2, the
 *      simple graph, the bit layout and the code of a permutation.  Then:
 *        1. vertex j of a row is its j-th entry >= 0 in row order, and its LABEL is labels[entry]: an entry of -1 in the middle shifts
 *           the later vertices down, and a repeated id is two vertices with one label;
 *        2. status 3, checked after 1 and 2 (a row with a bad endpoint or a bad edge_ptr range is 2 whatever its labels, as in
 *           ugs_wl_hash_labeled): an entry >= num_labels, or a label outside [0, 4096).  Nothing is read outside labels
 *           [0, num_labels).  A row of status != 0 has both key words -1 and k in every orbit slot; other rows are not disturbed;
 *        3. a permutation p is LABEL-MONOTONE if label(p(i)) <= label(p(j)) for all positions i < j.  The LABELLED CANONICAL CODE is
 *           the minimum of code(p) over the label-monotone permutations.  With all labels equal it is the canonical code;
 *        4. the KEY is the 128-bit number K = n * 2^124 + code * 2^96 + sum over p < n of L[p] * 2^(12 p), L being the row's labels
 *           sorted ascending -- the label at canonical position p.  key_out[row] = (K >> 64, K & (2^64 - 1)) as int64 bit patterns:
 *           the [rows, 2] form of ugs_wl_hash's digests, which ugs_wl_lookup takes, ascending as 128-bit numbers.  The high word is
 *           negative as int64 for n = 8;
 *        5. two rows have equal keys exactly when an isomorphism of their graphs maps labels to equal labels.  The key is invertible:
 *           n, the code and the sorted labels are bit fields of it, and (code, L) in the identity order is a representative;
 *        6. the LABELLED ROOTED CODE of vertex u is the minimum of code(p) over the permutations with p(n - 1) = u that put the other
 *           n - 1 vertices in non-decreasing label order by position; 0 for n = 1.  u and v lie in one orbit of the label-preserving
 *           automorphism group exactly when label(u) = label(v) and their labelled rooted codes are equal;
 *        7. a row's orbits are numbered 0, 1, ... by ascending (label, labelled rooted code); orbit_out [rows, k] int64: slot s holds
 *           the number of the orbit of the vertex that slot s is, k where the entry is < 0 and in every slot of a row of
 *           status != 0.  With all labels equal it is ugs_graphlet_orbits' orbit id minus base[class id].
 *      1 <= k <= 8, otherwise UGS_E_UNSUPPORTED.  At most 4096 labels: 12 bits each in the key.
 * ugs_graphlet_labelled: all pointers are DEVICE pointers.  d_labels [num_labels] int64; num_labels = 0 with a NULL d_labels is legal,
 *      every row with an entry >= 0 is then status 3.  d_key_out [rows, 2] int64, d_status_out [rows] int32, d_orbit_out [rows, k]
 *      int64 or NULL.  Limits and refusals as ugs_graphlet_canon.  One launch on the calling thread's stream, no allocation, no
 *      synchronisation with the host; rows = 0 is a no-op.
 * ugs_graphlet_labelled_code: HOST function, the same search on a graph given by its adjacency bits `code` (bits above n (n - 1) / 2:
 *      UGS_E_BAD_ARG) and the labels of its vertices 0 .. n-1 (labels[v], v < n, outside [0, 4096): UGS_E_BAD_ARG; entries from n
 *      on are not read).  key_out[0..1] = the two key words of item 4.  rooted_out, unless NULL: rooted_out[v] = the labelled rooted
 *      code of vertex v, 0xffffffff for n <= v < 8. */
int ugs_graphlet_labelled(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                          const int64_t *d_edge_ptr, int64_t rows, int k, const int64_t *d_labels, int64_t num_labels,
                          int64_t *d_key_out, int32_t *d_status_out, int64_t *d_orbit_out);
int ugs_graphlet_labelled_code(uint32_t code, int n, const int32_t *labels, int64_t *key_out, uint32_t *rooted_out);

/* ---- ugs_sampler.graphlets.census(edge_index, ptr, k, limit): the exact k-graphlet histogram of every graph of a batch, counted
 *      where the sets are found: no set is stored, so the device memory of a call does not grow with the number of sets.
 *      The law.
 *        1. POPULATION.  Graphs, adjacency and the population S_g are items 1 and 2 of the law at ugs_uniform_sample_batch_begin:
 *           graph g owns the vertices ptr[g] ... ptr[g+1]-1; only columns with both endpoints inside g's range count; adjacency is
 *           symmetrised, a loop joins nothing and duplicate columns collapse; S_g is every connected k-subset of g, none for n < k.
 *           The order of S_g plays no part.
 *        2. CLASS OF A SET.  The class of a set is the class of its induced simple graph on k vertices: key (k << 28) | canonical
 *           code and class id as ugs_graphlet_canon defines them (the set's vertices in any order: the key does not depend on it).
 *        3. COLUMNS.  d_keys [W] holds the keys of the connected graphs on exactly k vertices, ascending: W = 1, 1, 2, 6, 21, 112,
 *           853, 11 117 for k = 1 ... 8 (graphlets.connected_classes(k) is their class ids, ascending alike).  counts[g, c] is the
 *           number of sets of S_g whose key is d_keys[c].  A connected set's key is always one of them.
 *        4. IDENTITY WITH THE RECIPE.  For every healthy graph, counts[g] equals the histogram of ugs_graphlet_canon's class ids over
 *           the rows of ugs_uniform_enumerate_begin for that graph, restricted to those columns, bit for bit; every other column of
 *           that histogram is 0; and the sum of counts[g] is |S_g|, ugs_uniform_count_graphs' count.
 *        5. STATUS.  graph_status (host, num_graphs entries) has ugs_uniform_count_graphs' meanings: 0 healthy; 1 a graph of at
 *           least k vertices that ugs_uniform_sample_batch_begin refuses for its size (more than 64 vertices and over the limit in
 *           force, or outside the wide rule); 2 a graph with more than `limit` sets.  A failed graph has a row of zeros and leaves
 *           every other graph exact.  There is no joint budget: nothing is sized by the total, healthy graphs may together exceed
 *           limit.
 *        6. REFUSALS.  k outside 1 ... 8: UGS_E_UNSUPPORTED.  limit outside 1 ... 2^32: UGS_E_BAD_ARG.  The work per graph is bounded
 *           by limit: a graph past it stops at its next flush, as in the count pass.  The other argument errors are those of
 *           ugs_uniform_count_graphs.  num_graphs = 0 and num_cols = 0 are valid.
 *        7. Both forms of the uniform sampler take part -- the 64-bit mask form for graphs of at most 64 vertices, the wide form for 65
 *           ... ugs_uniform_max_vertices() under k * b <= 64 -- and ugs_uniform_set_mask_vertices steers it as it steers the samplers.
 * ugs_graphlet_census: edge_index, ptr and graph_status are HOST pointers as in ugs_uniform_count_graphs; d_keys [num_keys] int64,
 *      d_code_col and d_counts_out [num_graphs, num_keys] int64 are DEVICE pointers.  d_code_col is the table of
 *      ugs_graphlet_census_table for this k, required for k <= 7 and NULL for k = 8 (a raw code of 28 bits has no table: the
 *      canonical search runs per set).  Synchronous, no job: column buckets, adjacency, one census pass (the count pass's search)
 *      and the clearing of failed rows on the calling thread's stream, then the status read-back.  The counts are added with integer
 *      atomics: exact in any order.
 * ugs_graphlet_census_table: d_code_col_out [2^(n (n-1) / 2)] uint16 on the device, 1 <= n <= 7 (UGS_E_UNSUPPORTED otherwise): entry
 *      `code` is the column (index into d_keys) of the graph whose adjacency bits in the identity order are `code`, 0xFFFF for a
 *      graph that is not connected.  One launch on the calling thread's stream, no synchronisation. */
int ugs_graphlet_census(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                        int k, int64_t limit, const int64_t *d_keys, int64_t num_keys, const uint16_t *d_code_col,
                        int64_t *d_counts_out, int32_t *graph_status);
int ugs_graphlet_census_table(int n, const int64_t *d_keys, int64_t num_keys, uint16_t *d_code_col_out);

/* ---- ugs_sampler.graphlets.vertex_census(edge_index, ptr, k, limit): the exact k-graphlet degree vector (GDV) of every vertex of a
 *      batch -- how often the vertex sits in each automorphism orbit of each connected k-graphlet -- counted where the sets are found:
 *      no set is stored.  The law.
 *        1. POPULATION.  As item 1 of ugs_graphlet_census: graphs, adjacency and S_g are those of ugs_uniform_sample_batch_begin.
 *        2. ORBIT OF A MEMBER.  The orbit of member u of a set is the orbit id ugs_graphlet_orbits gives to u in the set's induced simple
 *           graph on k vertices.  It does not depend on the order of the set.
 *        3. COLUMNS.  There are O = 1, 1, 3, 11, 58, 407, 4306 columns for k = 1 ... 7: column c is graphlets.connected_orbits(k)[c], the
 *           ids of the orbits of the connected graphs on exactly k vertices, ascending.  Equivalently: with W and the class columns of
 *           ugs_graphlet_census item 3, and obase [W + 1] the exclusive prefix sum of the orbit counts (ugs_graphlet_orbit_counts) of
 *           those W classes in key order, obase[W] = O, the column of a member is obase[class column of the set] + its LOCAL ORBIT
 *           INDEX: the number of distinct rooted codes (ugs_graphlet_orbits item 2) of the set's graph below the member's.
 *           gdv[v, c], v a vertex id of the batch (0 <= v < N = ptr[num_graphs]), is the number of sets of S_g, g the graph that owns
 *           v, that contain v and in which v's column is c.  Rows of vertices below ptr[0] are zero.
 *        4. IDENTITY WITH THE RECIPE.  For healthy graphs gdv equals graphlets.vertex_orbit_counts(nodes, orbit ids, N,
 *           connected_orbits(k)) over the rows of ugs_uniform_enumerate_begin and ugs_graphlet_orbits' ids of them, bit for bit.
 *        5. IDENTITY WITH THE CENSUS.  For every graph g and every column c, of orbit q: the sum over g's vertices of gdv[v, c] = (number
 *           of vertices of q) * ugs_graphlet_census' count of q's class in g.  The sum of row v is the number of sets that contain v.
 *        6. STATUS, LIMIT AND REFUSALS.  graph_status as ugs_graphlet_census item 5; all vertices of a failed graph have rows of zeros,
 *           every other vertex stays exact; no joint budget.  k = 8 and k outside 1 ... 8: UGS_E_UNSUPPORTED, before any device work
 *           (k = 8 would be 72 489 columns a vertex and a canonical search a set).  limit outside 1 ... 2^32, ptr[0] < 0:
 *           UGS_E_BAD_ARG.  The work per graph is bounded by limit as in the census.  The other argument errors are those of
 *           ugs_uniform_count_graphs.  num_graphs = 0 and num_cols = 0 are valid.  Both forms of the uniform sampler take part, as
 *           ugs_graphlet_census item 7 says.
 * ugs_graphlet_vertex_census: edge_index, ptr and graph_status are HOST pointers as in ugs_uniform_count_graphs; d_obase [num_keys + 1]
 *      int64 (item 3; num_keys = W, num_orbits = O = its last entry), d_table (ugs_graphlet_vertex_census_table for this k) and
 *      d_gdv_out [N, O] int64 are DEVICE pointers.  The pass reads no keys: the table holds the class columns.  Synchronous, no job:
 *      gdv is zeroed, then column buckets, adjacency, one pass (the count pass's search) and the clearing of failed graphs' rows on
 *      the calling thread's stream, then the status read-back.  The counts are added with integer atomics: exact in any order.
 * ugs_graphlet_vertex_census_table: d_table_out [2^(n (n-1) / 2)] uint32 on the device, 1 <= n <= 7 (UGS_E_UNSUPPORTED otherwise),
 *      d_keys [num_keys] the ascending keys of the connected graphs on exactly n vertices.  Entry `code` describes the graph whose
 *      adjacency bits in the identity order are `code`: bits 0 ... 9 its class column (index into d_keys), bits 10 + 3 p ... 12 + 3 p
 *      the local orbit index of vertex p, p < n; 0xFFFFFFFF for a graph that is not connected.  One launch on the calling thread's
 *      stream, no synchronisation.
 * ugs_graphlet_vertex_census_entry: HOST function, no device work: *out = that entry, computed by the same code
 *      (ugs_gl::vertex_entry in csrc/ugs_graphlet_common.h) from the host's own table of connected keys.  UGS_E_BAD_ARG for a code with
 *      bits above n (n-1) / 2. */
int ugs_graphlet_vertex_census(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                               int k, int64_t limit, int64_t num_keys, const int64_t *d_obase, int64_t num_orbits,
                               const uint32_t *d_table, int64_t *d_gdv_out, int32_t *graph_status);
int ugs_graphlet_vertex_census_table(int n, const int64_t *d_keys, int64_t num_keys, uint32_t *d_table_out);
int ugs_graphlet_vertex_census_entry(uint32_t code, int n, uint32_t *out);

/* ---- graphlets.census / vertex_census (..., form="csr"): the same two results for graphs of ANY size, searched over adjacency lists
 *      instead of bitmap rows.  The law.
 *        1. The results are those of ugs_graphlet_census items 1 ... 4 and of ugs_graphlet_vertex_census items 1 ... 5, with the same
 *           columns and tables; on every graph the bitmap form accepts, counts and gdv are equal to its results bit for bit.
 *        2. THE GRAPH IS THE CSR.  Item 1 of ugs_graphlet_census as a data structure: d_rowptr [num_vertices + 1] int64 and d_col
 *           [num_entries] int32 hold the neighbours of every vertex of the batch, global vertex ids.  PRECONDITIONS: d_ptr
 *           [num_graphs + 1] is non-decreasing, d_ptr[0] >= 0 and d_ptr[num_graphs] = num_vertices; d_rowptr is non-decreasing from 0
 *           to num_entries; every entry of row v lies in the vertex range of v's graph and differs from v (so a vertex below d_ptr[0]
 *           has an empty row); every row is strictly ascending; u in row v implies v in row u.  One validation launch checks all of
 *           it before the search reads through the CSR and reads nothing outside the three arrays, whatever they hold: a CSR that
 *           breaks a precondition is UGS_E_BAD_ARG, never a fault.  graphlets._simple_csr builds such a CSR from edge_index and ptr.
 *        3. NO SIZE REFUSAL.  graph_status is 0 (healthy) or 2 (more than `limit` sets: zeros, every other graph exact, no joint
 *           budget); 1 does not occur, and ugs_uniform_set_max_vertices / ugs_uniform_set_mask_vertices play no part.  A graph of
 *           fewer than k vertices is healthy with zeros.  limit is 1 ... 2^62 (UGS_E_BAD_ARG otherwise): the counters are 64-bit.  The
 *           work per graph is bounded by limit: a graph past it stops at its next flush, every 4096 sets of a lane.
 *        4. REFUSALS, in this order, before any device work: k outside 1 ... 8, and k = 8 (a raw code of 28 bits has no table, and a
 *           canonical search per set is no part of this form): UGS_E_UNSUPPORTED; limit; num_vertices >= 2^31, num_entries > 2^31 - 1,
 *           num_graphs >= 2^31 - 1: UGS_E_UNSUPPORTED; then the pointers.  num_graphs = 0 and num_entries = 0 are valid.
 * All pointers are DEVICE pointers except graph_status (host, num_graphs entries).  d_keys, d_code_col (required: k <= 7), d_obase and
 * d_table are those of ugs_graphlet_census and ugs_graphlet_vertex_census for this k; d_counts_out is [num_graphs, num_keys], d_gdv_out
 * [num_vertices, num_orbits].  Synchronous, no job, on the calling thread's stream: the output is zeroed, the validation launch and its
 * read-back, one search pass (one wave per CSR entry with col > row), the read-back of the graphs' set counts for the status and, in
 * a call where some graph failed, the clearing of those graphs.  The counts are added with integer atomics: exact in any order.
 * Nothing of the batch is copied: the call's own device memory is 8 bytes a graph. */
int ugs_graphlet_census_csr(const int64_t *d_ptr, int64_t num_graphs, const int64_t *d_rowptr, const int32_t *d_col,
                            int64_t num_vertices, int64_t num_entries, int k, int64_t limit, const int64_t *d_keys, int64_t num_keys,
                            const uint16_t *d_code_col, int64_t *d_counts_out, int32_t *graph_status);
int ugs_graphlet_vertex_census_csr(const int64_t *d_ptr, int64_t num_graphs, const int64_t *d_rowptr, const int32_t *d_col,
                                   int64_t num_vertices, int64_t num_entries, int k, int64_t limit, int64_t num_keys,
                                   const int64_t *d_obase, int64_t num_orbits, const uint32_t *d_table, int64_t *d_gdv_out,
                                   int32_t *graph_status);

/* Per-kernel timing with HIP events recorded on the launch stream (off by default).  get_timing synchronises the
 * recorded events, returns summed milliseconds and launch counts for [0] the first-tier walk kernel, [1] overflow
 * tiers + scan kernels, [2] the fill kernel since the last call, and clears them. */
int ugs_plan_set_timing(ugs_plan *plan, int on);
int ugs_plan_get_timing(ugs_plan *plan, double *ms_sum3, int64_t *launches3);

#ifdef __cplusplus
}
#endif
#endif /* UGS_MI355_H */
