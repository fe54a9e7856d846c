// ugs_device.h -- structures shared by the host library (ugs_host.cpp, ugs_jobs.cpp, ugs_side_*.cpp) and the gfx950 kernels (ugs_kernels.hip).
//
// HBM layout of a *plan* (one PyG batch, or one graph of the handle API), all arrays resident in device memory:
//
//   graphs  UgsGraphDesc[G]          one 48-byte descriptor per graph
//   rowptr  int64[sum(n_g + 1)]      ABSOLUTE offsets into adj/ecol (row r of graph g at rowptr[rbase_g + r])
//   adj     int2[nnz]                (w, rank(w)) per CSR entry, CSR order = reference build_csr order
//                                    (reference src/preproc.cpp:32-86).  rank(w) = index_of[w] is stored NEXT TO
//                                    the neighbour so the suffix filter `index_of[w] >= root_vi`
//                                    (reference src/sampler.cpp:62) costs no second (random) gather.
//   adjf    int2[nnz]                (w, ecol): the fill kernel's view of the same CSR -- neighbour and the value written to
//                                    edge_src for this entry (batch: column of the batch edge_index; handle API: column
//                                    of the graph's edge_index) side by side, so the edge column costs no extra gather
//   roots   UgsRootRec[sum(n_g)]     alias table row + both candidate root vertices in ONE 24-byte record, so the
//                                    root draw (reference include/sampler.hpp:72-77 + src/sampler.cpp:165-173) is one gather
//   viable  int2[...]                (vi, order[vi]) lists for relaxation levels 1/2 (reference src/sampler.cpp:121-150)
//   prow    int2[sum(n_g) << s]      PADDED ROWS for the one-walk-per-wave tiers (built on the device at the first such walk):
//                                    vertex v of graph g owns the 2^s entries at (vbase_g + v) << s -- entry 0 is the row's header
//                                    (CSR degree, absolute CSR position of the row's first entry), entries 1.. are the first
//                                    2^s - 1 (w, rank(w)) pairs of the row; longer rows continue in adj[].  A walk step then needs
//                                    ONE dependent memory round trip (the row, at an address computed from the vertex) instead
//                                    of two (row pointer, then row), and no line is fetched for a row-pointer pair.  Only the lines
//                                    a typical visited row fills are fetched with the header (prow_first entries); the block's
//                                    remaining lines follow for the rows that reach into them.
//   ord1    uint8[n << 6]            FIRST-PICK TABLE of a plan of ONE graph, behind the padded rows in their allocation and built with
//                                    them (ugs_build_ord1): byte r of vertex v = position, in the candidate list the scan of v's row
//                                    leaves when v is the root, of the candidate at iteration position r of the reference's
//                                    unordered_set built from that list -- defined for r < c <= 64.  Handed to the walk as
//                                    UgsWalkArgs::ord1, not as a member of UgsPlanDev (see there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define UGS_KMAX 32          // largest supported k (per-walk vertex list lives in LDS / registers)

struct UgsGraphDesc {
    int64_t node_lo;      // added to local vertex ids in the nodes output (batch: ptr[g])
    int64_t rbase;        // first rowptr entry of this graph
    int64_t vbase;        // first roots[] entry of this graph
    int64_t viable_base;  // first viable[] entry (levels 1, 2)
    int32_t n;            // vertices
    int32_t level;        // 0: alias-weighted roots; 1, 2: uniform over viable list; -1: degenerate (n <= 0 or n < k)
    int32_t n_viable;
    int32_t pad;
};

struct UgsRootRec {
    double prob;          // alias-table acceptance probability of order position vi
    int32_t alias;        // alias order position
    int32_t v_self;       // order[vi]
    int32_t v_alias;      // order[alias]
    int32_t pad;
};

struct UgsPlanDev {
    const UgsGraphDesc *graphs;
    const int64_t *rowptr;
    const int2 *adj;
    const int2 *adjf;
    const UgsRootRec *roots;
    const int2 *viable;
    int64_t num_graphs;
    const int2 *prow;        // padded rows (NULL until built; the 8-lane and global-memory tiers use rowptr + adj)
    int32_t prow_shift;      // log2(entries per padded row), 3..6
    int32_t prow_first;      // entries fetched before the degree is known (whole 128-byte lines); the rest of the block only if the row needs it
};

struct UgsWalkArgs {
    UgsPlanDev plan;
    int32_t m;               // samples per graph
    int32_t k;
    int32_t mode;            // UGS_MODE_* / UGS_EDGE_* (0 local, 1 flat, 2 global)
    int32_t pad;             // UGS_SMALL_CAP: first-tier launch of tier S in its 32-candidate form; UGS_WIDE_LANES: tier S with 16 lanes per walk (the two may be ORed)
    int64_t extra_node_off;  // handle API "global": base_offset
    uint64_t seed64;         // (uint64_t)(int64_t)seed
    const uint64_t *seed_ptr;// if not NULL the seed is read from here (captured HIP graphs: the value changes between replays)
    int64_t row_begin;       // first of the G*m rows produced by this call
    int64_t row_count;
    int64_t *nodes;          // [row_count, k]
    uint32_t *counts;        // [row_count] edge entries per row; top bit (UGS_COUNT_STAGED) = the row's items are in `stage`
    // overflow hand-off between tiers: rows whose candidate set outgrew the tier's LDS capacity
    const int64_t *in_list;  // NULL: process rows 0..row_count-1; else process in_list[0..*in_count)
    const uint32_t *in_count;
    int64_t *ovf_list;       // rows (relative to row_begin) handed to the next tier
    uint32_t *ovf_count;
    // global-memory workspace of the last tier (per-group slices)
    uint32_t *gws;
    int64_t gws_words_per_group;
    int64_t gws_groups;      // number of workspace slices = grid of the global tier
    int32_t gcap;            // candidate capacity of the global tier
    int32_t ghs;             // hash slots (power of two) of the global tier
    int32_t gbcap;           // bucket-table entries of the global tier
    int32_t gpcap;           // words of all materialised stage orders of the global tier
    // induced edges staged by the walk itself (one-walk-per-wave LDS tiers; NULL = off): the walk meets every induced edge
    // when it scans the row of the later endpoint, so complete rows leave their directed edge items here in OUTPUT order
    // and the fill kernel only expands them.  Rows that do not fit (or ran in a tier without staging) are flagged 0 and,
    // if they have edges, listed for the row-reading fill kernel.
    // dynamic work distribution: the first gridsize*groups items are taken statically, every further item index is
    // groups_total + atomicAdd(work_next, 1) (NULL: static striding).  A walk's cost varies (degrees, which stages of the order
    // get invalidated), so a static split ends with the unluckiest wave.
    unsigned long long *work_next;
    uint32_t *wsum;          // 8-lane tier, optional: [ceil(row_count / 8)] sum of the counts of every 8 consecutive rows (for ugs_fill_scan)
    uint2 *stage;            // [row_count, UGS_STAGE_ITEMS]: x = batch column, y = source local index | target local index << 8
    int64_t *ulist;          // rows (relative) with edges that are NOT staged
    uint32_t *ucount;
    // per-graph seeds (ugs_sample_graphs_begin; NULL = off): [plan.num_graphs] seed bases (uint64_t)(int64_t)seed_g -- the rows of graph
    // gi draw from seeds[gi] instead of seed64 / *seed_ptr.  Last member, and read only by the walk kernels' SEEDS instantiations
    // (ugs_launch_walk picks them when it is set): the kernels of every other call are the code they were without it.
    const uint64_t *seeds;
    // first-pick table of a single-graph plan (NULL = off): 64 bytes per plan vertex, built once with the padded rows
    // (ugs_build_ord1).  Byte r of vertex v = position in D of the candidate at iteration position r of the candidate list that the
    // scan of v's row leaves when v is the root (defined for r < c <= 64).  Read only by the launch-uniform walk (do_walk's UNI
    // instantiation); behind every other member, so that the argument offsets of every other kernel stay what they were.
    const uint8_t *ord1;
};
#define UGS_COUNT_STAGED 0x80000000u
#define UGS_STAGE_ENTRIES 32    /* undirected hits a walk can hold in LDS */
#define UGS_STAGE_ITEMS 64      /* directed items per row in the staging buffer */

struct UgsFillArgs {
    UgsPlanDev plan;
    int32_t m, k, mode, pad;
    int64_t extra_node_off;
    int64_t row_begin, row_count;
    const int64_t *nodes;
    const int64_t *edge_ptr;   // [row_count + 1]
    int64_t *edge_index;       // [2, ld]
    int64_t ld;
    int64_t *edge_src;
    const uint2 *stage;        // staging left by the walk of the same rows (NULL: every row is filled from its adjacency rows)
    const uint32_t *counts;    // the walk's per-row counts: their top bit says whether the row was staged
    const int64_t *ulist;      // with staging: the rows the row-reading kernel still has to do
    const uint32_t *ucount;
    // scan folded into the fill (small-batch step, ugs_fill_scan): the kernel turns the walk's per-row counts into edge_ptr itself --
    // tiles of 32 rows, a tile's offset from the sums of 8 rows the walk kernel left
    int64_t *edge_ptr_out;              // [row_count + 1], written by the kernel (NULL: edge_ptr above is read)
    const uint32_t *wsum;               // [ceil(row_count / 8)]: UgsWalkArgs::wsum of the walk of the same rows
    // ugs_fill_scan for the library's own jobs (the drop-in call): the edge buffers are ONE staging area of `packed_cap` int64 words and
    // the kernel lays the outputs out for the total it computes itself -- edge_index [2, total] and edge_src [total] behind it, what
    // the caller's tensors look like, so that they leave in one copy -- or writes nothing if 3 * total exceeds the capacity (the host
    // sees the total and fills the ordinary way).  The block that owns the last tile hands the total to the host as soon as it
    // knows it (pinned words, epoch protocol of the scan kernels), before it fills its rows.
    int64_t packed_cap;                 // 0: off (edge_index / ld / edge_src as given)
    int64_t *h_total;
    uint32_t *h_flag;
    uint32_t epoch;
};

struct UgsLaunchInfo {
    const char *name;
    int grid, block, lds_bytes;
};

// tiers of the walk kernel: candidate-set capacity held in LDS per walk, lanes per walk
enum { UGS_TIER_S = 0 /* cap 64, 8 lanes */, UGS_TIER_M = 1 /* cap 448, 64 lanes */, UGS_TIER_W = 2 /* cap 704, 64 lanes, half-size bucket table */,
       UGS_TIER_X = 3 /* cap 1024, 64 lanes */, UGS_TIER_V = 4 /* cap 1408, 64 lanes, third-size bucket table */, UGS_TIER_L = 5 /* cap 2048, 64 lanes */,
       UGS_TIER_G = 6 /* global-memory workspace, 64 lanes */ };
#define UGS_LDS_TIERS 6
static constexpr int UGS_TIER_CAP[UGS_LDS_TIERS] = {64, 448, 704, 1024, 1408, 2048};
static constexpr int UGS_TIER_LANES[UGS_LDS_TIERS] = {8, 64, 64, 64, 64, 64};                // lanes per walk
static constexpr int UGS_TIER_HASH_LIMIT[UGS_LDS_TIERS] = {96, 448, 896, 1536, 1792, 3072};  // TierCfg<CAP>::HLIMIT (static_assert in ugs_kernels.hip)
// a form of tier S with half the workspace, for plans whose walks cannot hold more than 32 candidates (UgsWalkArgs::pad = UGS_SMALL_CAP)
#define UGS_SMALL_CAP 32
// tier S with 16 lanes per walk instead of 8 (UgsWalkArgs::pad = UGS_WIDE_LANES): first-tier launches whose walks are all resident at
// once (row_count <= CUs x blocks per CU x 16) of plans whose walks cannot be handed on -- such a launch lasts as long as one walk
#define UGS_WIDE_LANES 16
#define UGS_SMALL_HASH_LIMIT 48

hipError_t ugs_launch_walk(const UgsWalkArgs &a, int tier, int device_cus, int share_percent, hipStream_t s, UgsLaunchInfo *info);
hipError_t ugs_launch_build_prow(const UgsPlanDev &plan, int64_t num_vertices, int2 *prow, int shift, int device_cus, hipStream_t s);
// first-pick table (UgsWalkArgs::ord1) of a plan of ONE graph whose padded rows are built: one wave per root.  c1 (or NULL): the
// candidates the root's row leaves, per plan vertex (-1: the row outgrows the 448-candidate tier); both arrays zeroed by the caller.
#define UGS_ORD1_BYTES 64
hipError_t ugs_launch_build_ord1(const UgsPlanDev &plan, int64_t num_vertices, uint8_t *ord1, int32_t *c1, int device_cus, hipStream_t s);
#define UGS_COLLATE_MAX_WORLD 64
hipError_t ugs_launch_collate_unpack(const void *d_msgs, int world, int64_t msg_bytes, const int64_t *row_off, int k, int node_b, int eidx_b,
                                     int esrc_b, int64_t rows_cap, int64_t edge_cap, const int64_t *section_off4, int64_t *d_nodes,
                                     int64_t *d_edge_index, int64_t ld, int64_t *d_edge_ptr, int64_t *d_edge_src, int64_t *d_max_total,
                                     hipStream_t s);
// out[i] = in[i] + base, i < n (a row chunk's edge_ptr moved to its place in the whole call's: ugs_sample_batch_stream)
hipError_t ugs_launch_rebase_edge_ptr(const int64_t *in, int64_t *out, int64_t n, int64_t base, hipStream_t s);
// device batch pass (ugs_batch.hip): slicing, LRU keys and CSR of a batch of small graphs; limits per graph of that path
#define UGS_BATCH_PASS_MAX_COLS 1000   /* a key covers every column up to here (reference include/cache.hpp:100 samples longer graphs) */
#define UGS_BATCH_PASS_COLS_CEIL 8192  /* the limit a caller may raise it to (ugs_set_batch_pass_max_cols): the large form of the pass's kernels */
#define UGS_BATCH_PASS_MAX_N 2048
#define UGS_BATCH_PASS_FUSED_WORK (4ll << 20)   /* G * E up to here: the build kernel slices the batch itself (one launch) */
int64_t ugs_batch_pass_fused_work();             /* the limit in force: UGS_BP_FUSED_WORK overrides it (testing aid: 0 = always two kernels) */
hipError_t ugs_launch_batch_pass(const int64_t *d_src, const int64_t *d_dst, int64_t E, const int64_t *d_ptr, int64_t G, int k,
                                 int32_t *d_owner, uint32_t *d_cnt_jminc_jmax, const int64_t *d_rstart, int64_t *d_rowptr, int2 *d_adj,
                                 int2 *d_adjf, int32_t *d_vrank, unsigned long long *d_bump, unsigned long long bump_base, uint32_t epoch, void *h_back,
                                 unsigned long long *d_done, unsigned long long done_base, int64_t max_cols, hipStream_t s);
/* what the pass hands back per call, in pinned host memory: keys[G] u64 | fp[2G] u64 | cnt[G] | jminc[G] | jmax[G] u32 | flag | done u32 */
#define UGS_BP_BACK_CNT(G) ((size_t)(G) * 24)
#define UGS_BP_BACK_FLAG(G) ((size_t)(G) * 36)
#define UGS_BP_BACK_BYTES(G) ((size_t)(G) * 36 + 16)
// Content fingerprint of a graph of more than UGS_BATCH_PASS_MAX_COLS columns -- there the reference's key samples the columns
// (include/cache.hpp:100-107), so equal keys no longer mean equal graphs.  128 bits over (n, #columns, every renumbered column
// with its position): two 64-bit sums of a mix of (t, u, v), so any thread may add any column; the build kernel and the host
// (ugs_host.cpp: graph_fingerprint) compute the same value.
__host__ __device__ inline unsigned long long ugs_fp_mix(unsigned long long x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}
__host__ __device__ inline void ugs_fp_seed(unsigned long long n, unsigned long long cols, unsigned long long &a, unsigned long long &b) {
    a = ugs_fp_mix(n * 0x9e3779b97f4a7c15ull + cols);
    b = ugs_fp_mix(cols * 0xc2b2ae3d27d4eb4full + n);
}
__host__ __device__ inline void ugs_fp_add(unsigned long long t, unsigned long long u, unsigned long long v, unsigned long long &a, unsigned long long &b) {
    const unsigned long long ht = ugs_fp_mix(t + 0x9e3779b97f4a7c15ull), p = (u << 32) | (v & 0xffffffffull);
    a += ugs_fp_mix(p ^ ht);
    b += ugs_fp_mix(p * 0xc2b2ae3d27d4eb4full + ((ht >> 7) | (ht << 57)));
}
// graphs of a device-built plan the LRU does not know (cold path): the rest of their preprocessing on the device (ugs_bp_roots)
#define UGS_BATCH_ROOTS_MAX_N 1024     /* larger unknown graphs are preprocessed on the host, as before */
struct UgsBpMissIn { int32_t g; int32_t pad; int64_t roots_off; int64_t via_off; };           // arena offsets (elements) reserved by the host
struct UgsBpMissOut { int32_t level, n_viable, nonzero, max_deg; double Z, sb_deg; };
hipError_t ugs_launch_batch_roots(const int64_t *d_ptr, const int64_t *d_rstart, const int64_t *d_rowptr, const int2 *d_adj, const int32_t *d_vrank,
                                  const UgsBpMissIn *h_in, UgsBpMissOut *h_out, int64_t misses, int k, UgsRootRec *d_roots, int2 *d_via,
                                  unsigned long long *d_done, unsigned long long done_base, uint32_t *h_done, uint32_t epoch, int64_t max_cols, hipStream_t s);
// h_total / h_flag (pinned host memory, or NULL): the kernel also hands the total to the host and signals with `epoch`
hipError_t ugs_launch_scan(const uint32_t *counts, int64_t rows, int64_t *edge_ptr, int64_t *block_tmp, hipStream_t s, int64_t *h_total = nullptr,
                           uint32_t *h_flag = nullptr, uint32_t epoch = 0);
hipError_t ugs_launch_fill(const UgsFillArgs &a, int wide, int device_cus, hipStream_t s, UgsLaunchInfo *info);
// scan + fill in one launch (8-lane tier, rows read from their adjacency)
hipError_t ugs_launch_fill_scan(const UgsFillArgs &a, int device_cus, hipStream_t s, UgsLaunchInfo *info);
int64_t ugs_fill_scan_tiles(int64_t rows);
int64_t ugs_scan_tmp_words(int64_t rows);
int64_t ugs_global_ws_words(int64_t gcap, int64_t gbcap, int64_t gpcap, int64_t ghs);
uint32_t ugs_chain_at_least(int64_t c, int *index_out);
uint32_t ugs_chain_value(int idx);
int64_t ugs_ord_words(int stages);

// ---- uniform_sampler (ugs_uniform.hip): exact uniform connected k-subgraph sampling; graphs of at most 64 vertices as 64-bit
//      masks, graphs of up to UGS_UNI_WIDE_MAX_N vertices (opt-in: ugs_uniform_set_max_vertices) as packed tuples ----
#define UGS_UNI_BUDGET ((int64_t)1 << 25)    /* connected k-subsets (64-bit masks) one call may hold on the device */
#define UGS_UNI_DISTINCT_MAX_M 4096          /* rows per graph of a distinct call: uni_draw_distinct sorts that many 8-byte keys in LDS */
#define UGS_UNI_NO_KEY (~0ull)               /* row key of a wide graph's row of -1 (k ascending fields never pack to all ones) */
struct UgsUniGraph {
    int64_t lo;           // ptr[g]
    int64_t vbase;        // first entry of this graph in the enumerated vertices (adj, items >> 6)
    int32_t n;            // vertices
    int32_t enumerable;   // 1: 1 <= k <= n <= 64, its subsets are enumerated as masks; 2: the wide form (UgsUniWide); 0: S_g is empty
};
struct UgsUniCall {
    int64_t G, E, nv, rows, budget;          // graphs, columns, enumerated vertices, G * m rows, mask budget
    int32_t m, k, mode;                      // mode 0: "sample" (row positions), otherwise batch ids
    uint64_t seed;
    const uint64_t *seeds;                   // [G] per-graph generators (ugs_uniform_sample_graphs_begin); nullptr: one for the call, or no draws
    int32_t distinct;                        // with seeds: graph g's m draws are distinct (uni_draw_distinct; ugs_uniform_distinct_begin), -1 past |S_g|
    int32_t per_graph;                      // the budget bounds every graph's own count (sample_graphs, count, enumerate), not the call's
    int64_t *gcount;                         // [G] per-graph subset count of the count pass (per_graph only; > budget: the graph failed)
    const int64_t *sptr;                     // [G + 1] enumerate only: exclusive scan of gsize in batch graph order (= sample_ptr); rows = sptr[G]
    const int64_t *src, *dst, *ptr;          // the batch, on the device: src[E], dst[E], ptr[G + 1]
    const UgsUniGraph *graphs;               // [G]
    const int32_t *vgraph;                   // [nv] graph of an enumerated vertex
    void *cub_tmp; size_t cub_bytes;         // hipCUB scratch (ugs_uniform_cub_bytes)
    uint32_t *ckey, *ckey2; int32_t *cval, *cval2;   // [E] column -> graph (G: none), before / after the stable sort
    int64_t *cstart;                         // [G + 1] graph g's columns at sorted positions [cstart[g], cstart[g+1])
    uint16_t *bpair;                         // [E] local endpoints u | v << 8 of a sorted column (enumerable graphs)
    uint64_t *adj;                           // [nv] neighbour mask of each enumerated vertex (no self bits)
    uint32_t *icount;                        // [nv * 64] subsets of item (root vertex, first extension w)
    int64_t *ioff;                           // [nv * 64 + 1] exclusive scan of icount
    int64_t *scan_tmp;                       // ugs_scan_tmp_words(max(nv * 64, rows))
    int32_t *seg_lo, *seg_hi;                // [nv] root buckets of the segmented radix sort (empty unless large)
    uint64_t *keys_a, *keys_b;               // [budget] subset keys ~brev(mask) and the sort's second buffer
    const uint64_t *keys_sorted;             // set by ugs_uniform_begin: keys_a or keys_b
    int64_t *gstart, *gsize;                 // [G] first key and |S_g|
    int32_t *nepos, *ne_list;                // [G] position among the graphs with S_g non-empty (-1: empty) / its inverse
    int32_t *draws;                          // [G * m] index into S_g of each draw (seeds: draw s of graph g at g * m + s); < 0: a row of -1
    uint64_t *rowmask;                       // [rows] subset of each row (0: a row of -1)
    uint32_t *ecount;                        // [rows] edge entries per row
    int64_t *status;                         // [4] running subset count, over-budget flag
    int64_t *nodes, *edge_ptr;               // outputs: [rows, k], [rows + 1]
};
// The wide graphs of a call (more than 64 vertices, or every graph the mask threshold sends here).  A set's sort key is its ascending
// tuple packed big-endian in fields of b = bit length of n - 1 bits (k <= 8, k b <= 64): ascending keys = the reference's order, the
// root is the first field.  The enumerated vertices of the mask graphs come first, [0, nv_mask), those of the wide graphs after them,
// [nv_mask, nv); a wide root has 64 items as a mask root has: item j holds the sets whose first extension vertex is the root's
// (j + 64 i)-th higher neighbour, so ioff[vi * 64] bounds the root bucket of either form.
#define UGS_UNI_WIDE_MAX_N 1024
#define UGS_UNI_WIDE_MAX_K 8
struct UgsUniWide {
    int64_t nv_mask;                         // enumerated vertices of the mask graphs (== nv: the call has no wide graph)
    int64_t adj_words;                       // words of wadj
    const int64_t *wbase;                    // [G] first word of graph g's bitmap in wadj; -1: not a wide graph
    uint64_t *wadj;                          // per wide graph n rows of W = ceil(n / 64) words: the neighbours of each vertex (no self bits)
    uint32_t *wpair;                         // [E] local endpoints u | v << 16 of a sorted column (wide graphs)
    int64_t *gsize_mask;                     // [G] gsize with the wide graphs at 0: what the mask form's row kernel sees
    uint64_t *rowkey;                        // [rows] key of a wide graph's row
};
size_t ugs_uniform_cub_bytes(int64_t E, int64_t nv, int64_t budget);
hipError_t ugs_uniform_begin(UgsUniCall &c, const UgsUniWide &w, hipStream_t s);
hipError_t ugs_uniform_fill(const UgsUniCall &c, const UgsUniWide &w, int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s);
// count: column buckets, adjacency and the count pass only (gcount; reads neither ioff nor a key array).  enumerate: enum_keys runs
// everything up to gstart / gsize; with sptr, rows, nodes, edge_ptr and ecount set, enum_rows writes one row per key and scans the
// edge counts, enum_fill the edges.
hipError_t ugs_uniform_count(UgsUniCall &c, const UgsUniWide &w, hipStream_t s);
hipError_t ugs_uniform_enum_keys(UgsUniCall &c, const UgsUniWide &w, hipStream_t s);
hipError_t ugs_uniform_enum_rows(const UgsUniCall &c, const UgsUniWide &w, hipStream_t s);
hipError_t ugs_uniform_enum_fill(const UgsUniCall &c, const UgsUniWide &w, int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s);
// ugs_graphlet_census (law in include/ugs_mi355.h): count's column buckets and adjacency, then the census pass in the count pass's
// place -- the same search, every completed set classified and counted into counts[g, column]; gcount as count leaves it; the row of a
// graph past the budget is cleared behind it.
struct UgsCensus {
    const uint16_t *code_col;                // [2^(k (k-1) / 2)] raw adjacency code -> column, 0xFFFF: not connected; nullptr: canonical search per set
    const int64_t *keys;                     // [W] ascending keys of the connected graphs on exactly k vertices: the columns
    int64_t W;
    unsigned long long *counts;              // [G, W]
};
hipError_t ugs_uniform_census(UgsUniCall &c, const UgsUniWide &w, const UgsCensus &z, hipStream_t s);
// ugs_graphlet_vertex_census (law in include/ugs_mi355.h): the same, per vertex -- every completed set adds one to k cells of gdv, the
// cell of member u being [ptr[g] + u, obase[column] + local orbit index of u's position]; the rows of a graph past the budget are
// cleared behind the pass.
struct UgsVertexCensus {
    const uint32_t *table;                   // [2^(k (k-1) / 2)] raw adjacency code -> ugs_gl::vertex_entry, k <= 7
    const int64_t *obase;                    // [W + 1] first column of each connected class's orbits; obase[W] = O
    int64_t W, O, N;                         // classes, columns, rows (= ptr[G])
    unsigned long long *gdv;                 // [N, O]
};
hipError_t ugs_uniform_vertex_census(UgsUniCall &c, const UgsUniWide &w, const UgsVertexCensus &z, hipStream_t s);

// ---- the population cache (ugs_uniform_population_*): the sorted keys of a graph kept on the device across calls ----
// A 64-bit fingerprint of a graph's adjacency: the sum over its non-zero bitmap words of a mix of (word, position), the bitmap being
// n rows of W = ceil(n / 64) words in either form (W = 1: the mask form's adj).  Independent of column order and duplicates.
// ugs_uniform_pop_store, behind enum_keys on the same stream: graph g's gsize[g] sorted keys go to dst[g] (nullptr: nothing to
// copy) and its fingerprint to fp_out[g] (0 for a graph that is not enumerated).
hipError_t ugs_uniform_pop_store(const UgsUniCall &c, const UgsUniWide &w, uint64_t *const *dst, uint64_t *fp_out, hipStream_t s);
struct UgsPopGraph {
    const uint64_t *keys; // the graph's |S_g| sorted keys in the population's storage (nullptr: S_g is empty or the graph failed)
    int64_t lo;           // ptr[g]
    uint64_t fp;          // fingerprint stored at add time
    int32_t n, form, b;   // vertices; 1: mask keys, 2: wide keys of b-bit fields, 0: no keys
};
// A sample call served from a population.  `c` carries what the shared kernels read (uni_colgraph, uni_bucket, uni_draw /
// uni_draw_graphs; with check: uni_adj / uni_wadj over c.graphs, c.adj, w.wbase, w.wadj); gsize comes from the host.  pair[p] =
// u | v << 16, the local endpoints of sorted column p; rowkey[row] = the row's mask (mask form; 0: a row of -1) or key (wide).
// status[2] = G - (first graph whose fingerprint differs), 0: none.
struct UgsPopCall {
    UgsUniCall c;
    UgsUniWide w;
    const UgsPopGraph *pg;                   // [G]
    uint32_t *pair;                          // [E]
    uint64_t *rowkey;                        // [rows]
    int32_t check, any_wide;                 // any_wide: some graph of the batch has wide keys to draw from
};
hipError_t ugs_uniform_pop_begin(UgsPopCall &p, hipStream_t s);
hipError_t ugs_uniform_pop_fill(const UgsPopCall &p, int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s);
// WL class indices (ugs_uniform_population_*_wl_*): every stored key has an int32 class index beside it (the class of its WL digest,
// -1: no digest), a slot also a fingerprint of its loop vertices -- the bitmap of the vertices with a loop column, reduced like an
// adjacency bitmap.  ugs_uniform_pop_loops, behind the column buckets of either kind of call: out[g] = graph g's loop fingerprint
// (add), or status[3] = G - (first enumerable graph whose fingerprint is not want[g]), 0: none (check).  ugs_uniform_pop_wl, behind
// ugs_uniform_pop_begin and before the status words are read: that check (p.check), then ids_out[row] = id_of_class[cls[g][draw]],
// unknown_id for a row of -1 or a class of -1.
struct UgsPopWl {
    const int32_t *const *cls;               // [G] the class indices of graph g's keys (nullptr: no keys)
    const uint64_t *lfp;                     // [G] loop fingerprint stored at add time
    const int64_t *id_of_class;              // [classes] vocabulary id of every class (ugs_wl_lookup over the class table)
    int64_t unknown_id;
    int64_t *ids_out;                        // [rows]
};
hipError_t ugs_uniform_pop_loops(const UgsUniCall &c, const uint64_t *want, uint64_t *out, hipStream_t s);
hipError_t ugs_uniform_pop_wl(const UgsPopCall &p, const UgsPopWl &q, hipStream_t s);

// ---- rwr_sampler (ugs_rwr.hip): random walk with restart, one SplitMix64 stream per graph, counter-based speculation ----
#define UGS_RWR_KMAX 64
struct UgsRwrGraph {
    int64_t lo;           // ptr[g]
    int64_t vbase;        // ptr[g] - ptr[0]: first vertex of the graph in the batch's CSR
    int32_t n;            // vertices
    int32_t T;            // iteration limit 10 n k of a walk (n >= k >= 1); 0: n < k, m rows of -1 and no draws
};
struct UgsRwrCall {
    int64_t G, E, NV, rows;                  // graphs, columns, batch vertices ptr[G] - ptr[0], G * m rows
    int32_t m, k, mode, spec;                // mode 0: "sample" (row positions), otherwise batch ids; window = spec * block offsets
    int32_t row_streams;                     // != 0: one generator per row (ugs_rwr_sample_rows_begin), set by ugs_rwr_row_streams with:
    int32_t row_wgs;                         //   workgroups of rwr_row_walks per graph
    int32_t row_lds_ints;                    //   CSR words of the largest graph that walks from LDS: the launch's dynamic LDS
    uint64_t seed;
    const uint64_t *seeds;                   // [G] generator of each graph (ugs_rwr_sample_graphs_begin); nullptr: seed + g
    double p;                                // p_restart
    const int64_t *src, *dst, *ptr;          // the batch, on the device: src[E], dst[E], ptr[G + 1]
    const UgsRwrGraph *graphs;               // [G]
    void *cub_tmp; size_t cub_bytes;         // hipCUB scratch (ugs_rwr_cub_bytes)
    uint32_t *hkey, *hkey2;                  // [2E] half-edge 2e + side: its source vertex - ptr[0] (NV: column dropped), before / after the sort
    int32_t *hval, *hval2;                   // [2E] the half-edge's target, local to its graph; sorted: the CSR targets
    int32_t *rs;                             // [NV + 1] CSR row starts (rows in (column, side) order of their half-edges)
    int32_t *parent, *csize;                 // [NV] union-find over the columns, component sizes at the roots
    uint8_t *doomed;                         // [NV] the vertex's component has fewer than k vertices: every walk seeded there fails
    int64_t *rstart;                         // [rows] draws of the graph's stream consumed before the row's walk (row streams: 0); -1: a row of -1
    uint32_t *ecount;                        // [rows] edge entries per row
    int64_t *scan_tmp;                       // ugs_scan_tmp_words(rows)
    int64_t *nodes, *edge_ptr;               // outputs: [rows, k], [rows + 1]
};
size_t ugs_rwr_cub_bytes(int64_t E);
// makes c a row-streams call; graphs[G] and half_edges[G] (twice the columns inside each graph) are host arrays
void ugs_rwr_row_streams(UgsRwrCall &c, const UgsRwrGraph *graphs, const int64_t *half_edges);
hipError_t ugs_rwr_begin(const UgsRwrCall &c, hipStream_t s);      // ugs_rwr_build, then ugs_rwr_walks
hipError_t ugs_rwr_build(const UgsRwrCall &c, hipStream_t s);      // rwr_init ... rwr_rowstart: rs, hval2 and doomed of the batch
hipError_t ugs_rwr_walks(const UgsRwrCall &c, hipStream_t s);      // the walks and the scan, from whatever rs, hval2 and doomed point at
// rwr_sampler.GraphCache: the store is one "batch of all added graphs".  An add occupies NV + 1 entries of
// rs (absolute offsets into tg) and of doomed, 2E of tg and E of cols; a graph's vbase is its vertex offset in rs.
struct UgsRwrStore {
    int32_t *rs, *tg; uint8_t *doomed; int2 *cols;       // the storage generation being written
    int64_t rs_base, tg_base, col_base;                  // where this add goes: behind everything the store holds
};
hipError_t ugs_rwr_store_append(const UgsRwrCall &c, const UgsRwrStore &st, hipStream_t s);     // after ugs_rwr_build(c)
struct UgsRwrCheck {
    int64_t E, G;
    const int64_t *src, *dst;                            // the batch's columns
    const UgsRwrGraph *graphs;                           // [G] (lo = ptr[g])
    const int64_t *coff, *col0;                          // [G + 1] prefix sums of the slots' column counts; [G] first stored column, -1: none
    const int2 *cols;                                    // the store's columns
    int32_t *first_bad;                                  // atomicMin of the graphs with a column that differs
};
hipError_t ugs_rwr_store_check(const UgsRwrCheck &k, hipStream_t s);
hipError_t ugs_rwr_fill(const UgsRwrCall &c, int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s);

// ---- ugs_sampler.GraphCache (ugs_store.hip): the store is one "plan of all added graphs".  An add lays its
//      chunk out as a plan of its own (columns local to each graph) and ugs_store_append moves that plan behind everything the store
//      holds: rowptr + adj_base, adj, adjf, root records, viable entries, and the chunk's columns narrowed to int2 pairs of local ids.
struct UgsStoreAppend {
    const int64_t *rowptr; const int2 *adj, *adjf; const UgsRootRec *roots; const int2 *viable;      // the chunk's plan
    const int64_t *col_u, *col_v;                                                                    // the chunk's columns, local ids
    int64_t n_rowptr, nnz, n_roots, n_viable, n_cols;                                                // entries of each of them
    int64_t *s_rowptr; int2 *s_adj, *s_adjf; UgsRootRec *s_roots; int2 *s_viable, *s_cols;           // the storage generation being written
    int64_t row_base, adj_base, root_base, via_base, col_base;                                       // where this add goes
};
hipError_t ugs_store_append(const UgsStoreAppend &a, hipStream_t s);
// The check of a cached call: column e of the batch, of the graph g with coff[g] <= e < coff[g+1], against stored column
// col0[g] + e - coff[g] after taking lo[g] = ptr[g] off both endpoints; first_bad = the smallest g with a column that differs.
struct UgsStoreCheck {
    int64_t E, G;
    const int64_t *src, *dst;                            // the batch's columns
    const int64_t *lo, *coff, *col0;                     // [G] ptr[g]; [G + 1] prefix sums of the slots' column counts; [G] first stored column
    const int2 *cols;                                    // the store's columns
    int32_t *first_bad;
};
hipError_t ugs_store_check(const UgsStoreCheck &c, hipStream_t s);
// edge_src of a cached call, behind its fill: the store's adjf holds columns local to their graph, so the entries
// [edge_ptr[r], edge_ptr[r+1]) of row r get coff[r / m] added -- the column's place in the batch.
hipError_t ugs_store_rebase_src(const int64_t *edge_ptr, int64_t *edge_src, const int64_t *coff, int64_t rows, int32_t m, hipStream_t s);

// ---- epsilon_uniform_sampler (ugs_eps.hip): one launcher for the walk (fill = 0: nodes and per-row counts) and the fill ----
struct UgsEpsLaunch {
    const UgsGraphDesc *graphs; const int64_t *rowptr; const int32_t *nbr; const int32_t *ecs; int64_t num_graphs;
    int32_t m, k, mode, max_attempts; uint64_t seed; double epsilon; int64_t rows;
    int64_t *nodes; uint32_t *counts; const int64_t *edge_ptr; int64_t *edge_index; int64_t *edge_src; int64_t ld;
    const uint64_t *seeds;        // device array [num_graphs]: one seed per graph (sample_graphs); null: `seed` for every row
    const int64_t *col_base;      // device array [num_graphs], fill only: added to the column an ecs entry names (a cached call, whose
                                  // rows hold columns local to their graph); null: ecs holds batch columns already
};
hipError_t ugs_eps_launch(const UgsEpsLaunch &l, int fill, int cus, hipStream_t s);
// epsilon_uniform_sampler.GraphCache (ugs_eps_cache.cpp): the adjacency of an add, built on the device behind
// everything the store holds.  Graph g of the add has vertices vptr[g] ... vptr[g+1] and the columns cptr[g] ... cptr[g+1] of
// cols[col_base ...] (pairs of local ids, already in the store); it gets the n + 1 rowptr entries from row_base + vptr[g] + g
// (absolute offsets into nbr / ecs) and the 2 (cptr[g+1] - cptr[g]) entries of nbr / ecs from adj_base + 2 cptr[g].  Within a vertex's
// row the half-edges stand in (column, side) order, source side first: the push_back order of eps_begin.
struct UgsEpsBuild {
    int64_t G;
    const int64_t *vptr, *cptr;                          // [G + 1] each, device
    int32_t *cursor;                                     // scratch [vptr[G]]: per-vertex write position, relative to the graph's entries
    int64_t *rowptr; int32_t *nbr, *ecs; const int2 *cols;      // the storage generation being written
    int64_t row_base, adj_base, col_base;                // where this add goes
};
hipError_t ugs_eps_build(const UgsEpsBuild &b, hipStream_t s);

// ---- ugs_sampler.rows.unique_rows (ugs_rows.hip; host: ugs_rows.cpp; law: include/ugs_mi355.h at ugs_rows_unique_begin) ----
// One call's arrays.  The inputs are the caller's; everything else is a piece of the job's blob.  A status word holds the lowest
// offending index of its kind, UGS_ROWS_NONE where there is none; a kernel behind the check runs only while words 0 and 1 say so,
// so nothing is ever indexed by a pointer-array value that the check has not passed.
#define UGS_ROWS_NONE 0x7f7f7f7f7f7f7f7fll
#define UGS_ROWS_MAX_PER_GRAPH 4096
enum { UGS_ROWS_ST_PTR = 0 /* index into sample_ptr (code 0), edge_ptr (1) or ptr (2): 4 index + code */, UGS_ROWS_ST_GRAPH = 1 /* graph over a limit */,
       UGS_ROWS_ST_ENTRY = 2 /* row with an entry outside its graph */, UGS_ROWS_ST_WORDS = 4 };
struct UgsRowsBack { int64_t U, Eu, st[UGS_ROWS_ST_WORDS - 1], big, small; };   // what begin reads back: totals, status, graphs in the workgroup and the wave form
struct UgsRowsCall {
    const int64_t *nodes, *edge_ptr, *sample_ptr, *ptr;      // inputs: [R, k], [R + 1], [G + 1], [G + 1]
    int64_t R, G, Es;
    int32_t k, by /* 0 sequence, 1 set */, bits;
    int64_t *status;                                         // [UGS_ROWS_ST_WORDS]
    uint4 *keys;                                             // [R]
    int32_t *rowg, *rep, *lrank, *cnt;                       // [R]: graph of the row; representative (a row); rank among its graph's kept rows and
                                                             //      run length (kept rows only)
    int64_t *eoff;                                           // [R]: edge entries of the kept rows before it in its graph (kept rows only)
    int64_t *ug, *eg;                                        // [G]: kept rows and their edge entries per graph
    int64_t *ubase, *ebase;                                  // [G + 1]: their exclusive scans
    int32_t *big, *nbig;                                     // [3][G] graphs of 65..256, ..1024, ..4096 rows, in any order; their numbers [3] and the number of graphs of 1..64 rows
    UgsRowsBack *back;
};
struct UgsRowsOut {
    const int64_t *edge_index_in; int64_t in_stride; const int64_t *edge_src_in;
    int64_t *nodes_u, *edge_index_u, *edge_ptr_u, *sample_ptr_u, *edge_src_u, *count, *inverse; int64_t ld;
};
hipError_t ugs_rows_dedup(const UgsRowsCall &c, hipStream_t s);                          // check, keys, both dedup forms, scan, `back`
hipError_t ugs_rows_compact(const UgsRowsCall &c, const UgsRowsOut &o, int64_t U, int64_t Eu, hipStream_t s);

// ---- device-side preprocessing stages (ugs_preproc.hip) ----
struct UgsDevPre;
size_t ugs_devpre_bytes(int64_t n, int64_t E);
hipError_t ugs_devpre_csr(UgsDevPre **out, const int64_t *h_src, const int64_t *h_dst, int64_t E, int64_t n, hipStream_t s, int64_t *h_rowptr, int64_t *nnz_out);
hipError_t ugs_devpre_roots(UgsDevPre *d, const int32_t *h_order, const int32_t *h_rank, int k, int32_t *h_sdeg, uint8_t *h_reach);
hipError_t ugs_devpre_download(UgsDevPre *d, int32_t *h_nbr, int32_t *h_col);
void ugs_devpre_free(UgsDevPre *d);
void ugs_devpre_trim(UgsDevPre *d);
size_t ugs_devpre_resident_bytes(const UgsDevPre *d);
hipError_t ugs_devpre_assemble(UgsDevPre *d, const int64_t *h_colmap, int64_t cols, int2 *adj, int2 *adjf, hipStream_t s);

// ---- what the .hip translation units and ugs_apx.cpp take from ugs_host.cpp (internal, not part of the C ABI; the host files
//      of the job path and the side samplers share more with it, through ugs_host_internal.h) ----
int ugs_internal_fail(int code, const char *msg);            // sets the calling thread's message, the one ugs_last_error() returns; returns code
int ugs_internal_ctx(int *device, hipStream_t *stream);      // the calling thread's device and stream (ugs_set_device / ugs_set_stream)
