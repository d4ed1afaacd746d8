// Definitions shared by the translation units that implement the forest operator (forest.hip,
// qring.hip).  Internal: not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <memory>
#include <type_traits>
#include <vector>

#include "common.h"

struct tahoe_qstate;  // quantised views + workspace, owned by qring.hip
struct tahoe_sstate;  // sparse (irregular) forest, owned by sparse.hip
struct tahoe_pstate;  // host-batch upload pipeline, owned by pipeline.hip
struct tahoe_wstate;  // float32 walk for wide rows, owned by widef.hip
struct tahoe_cstate;  // TreeSHAP path tables (TAHOE_CREATE_CONTRIBS), owned by contribs.hip
struct tahoe_istate;  // background of interventional TreeSHAP (tahoe_forest_set_background), owned by interventional.hip
struct tahoe_astate;  // Saabas node deltas (TAHOE_CREATE_APPROX_CONTRIBS), owned by approx.hip
struct tahoe_ostate;  // oblivious (symmetric) forest, owned by oblivious.hip
struct tahoe_vstate;  // vector-leaf forest, owned by vector.hip (its TreeSHAP tables by vector_shap.hip)
struct tahoe_pdstate; // cover fractions + workspace of TAHOE_CREATE_PARTIAL_DEPENDENCE, owned by partial_dependence.hip

namespace tahoe {

struct InnerNode {
    float thr;
    uint32_t meta;  // fid (30 bits, FID_MASK of Struct.h:57) | exchange << 30 | def_left << 31
};
constexpr uint32_t kMetaFidMask = 0x3fffffffu;
constexpr uint32_t kMetaExchange = 1u << 30;  // probability-guided re-layout: children stored swapped, condition inverted
static_assert(sizeof(InnerNode) == 8, "InnerNode must be 8 bytes");

constexpr int kBlock = 256;             // threads per workgroup of DIRECT / ROWTILE (4 waves)
constexpr int kWaves = kBlock / 64;
constexpr int kTileRows = 64;           // rows per ROWTILE workgroup = one wave of lanes
constexpr int kMaxLdsLevels = 8;        // ROWTILE: top levels staged per wave (255 nodes = 2040 B)
constexpr float kMissingEps = 1.0e-6f;  // BaseTahoeTest.h:451

// TILEBLOCK geometry
constexpr int kTopLevelsMax = 10;       // top levels kept in LDS (1023 nodes: 4 KiB thr + 2 KiB meta)
constexpr int kSlots = 4;               // trees in flight per workgroup
constexpr int kBlockFidBits = 9;        // bottom blocks pack 3 x (fid:9 | def_left:1) in one dword
constexpr int kBlockMaxCols = 1 << kBlockFidBits;

static inline int align16(int x) { return (x + 15) & ~15; }
static inline int top_nodes(int top_levels) { return (1 << top_levels) - 1; }
// A staged top is indexed by 1-based heap position (entry 0 unused), so that the two children of
// position i form the aligned pair (2i, 2i+1).
static inline int top_thr_bytes(int top_levels) { return align16((top_nodes(top_levels) + 1) * 4); }
static inline int top_stride_bytes(int top_levels)
{
    return top_thr_bytes(top_levels) + align16((top_nodes(top_levels) + 1) * 2);
}

}  // namespace tahoe

// Tuning knobs for experiments: environment variables read ONCE per handle, by open_handle (never on the predict path).  A field
// holds atoi of its variable (a bool: atoi != 0), or the default below when the variable is unset; a knob touches only the forms
// named beside it.  tools/README.md lists the same table.
struct tahoe_knobs {
    int lds_levels = INT_MAX;     // TAHOE_LDS_LEVELS: cap on ROWTILE's and TILEBLOCK's levels in LDS (dense; never raises the caps)
    int tile_rows = 0;            // TAHOE_TILE_ROWS = 64 / 128: rows per TILEBLOCK / TILERING tile (dense)
    int qring_walkers = 0;        // TAHOE_QRING_WALKERS = 15 / 12 / 8 / 4: walkers of QRING's 128-slot column form
    int qring_chains = 0;         // TAHOE_QRING_CHAINS = 2 / 3: force the tile form of QRING's region layout (dense and sparse)
    int qring_slices = 0;         // TAHOE_QRING_SLICES >= 1: force the tree slices per tile of QRING's SPLIT form
    int qring_groups = 0;         // TAHOE_QRING_GROUPS: at least this many tree groups
    int qring_wide_chains = 0;    // TAHOE_QRING_WIDE_CHAINS = 1: one tree group per walker of the wide-row form
    bool qring_wide = true;       // TAHOE_QRING_WIDE = 0: the GX form instead of the wide-row tiles
    bool qring_narrow = true;     // TAHOE_QRING_NARROW = 0: the general node layout
    bool qring_regions = true;    // TAHOE_QRING_REGIONS = 0: the 128-slot column layout instead of the region form
    bool qring_code8 = true;      // TAHOE_QRING_CODE8 = 0: u16 codes where u8 codes would serve
    bool qring_narrow128 = true;  // TAHOE_QRING_NARROW128 = 0: the 32-KiB region stride for forests of <= 128 features
    bool qring_top24 = true;      // TAHOE_QRING_TOP24 = 0: no packed tops (192-row u16 tiles stage the u32 tops always)
    bool quant_buckets = true;    // TAHOE_QUANT_BUCKETS = 0: no bucketed quantise kernel
    bool quant_multi = true;      // TAHOE_QUANT_MULTI = 0: the pair quantise kernels instead of the many-features ones
    bool sparse_qring = true;     // TAHOE_SPARSE_QRING = 0: a sparse handle keeps the float32 kernels only
    bool widef = true;            // TAHOE_WIDEF = 0: no float32 wide-row form of TILERING
    int wstream = -1;             // TAHOE_WSTREAM: 0 = never the row-streaming form, 1 = wherever it can be built, -1 = the shape rule
    int wstream_slab_mb = 1024;   // TAHOE_WSTREAM_SLAB_MB: cap of the row-streaming form's leaf-value workspace (at least 1 MiB)
    int approx_form = 0;          // TAHOE_APPROX_FORM: 1 = the LDS slab wherever one wave's slab fits, 2 = in place
    int csr_chunk_mb = 64;        // TAHOE_CSR_CHUNK_MB: cap of tahoe_forest_predict_csr's densify chunk (at least one 64-row tile)
    int csr_fused = -1;           // TAHOE_CSR_FUSED: under AUTO, 0 = never the fused CSR tile kernels, 1 = wherever one exists, -1 = the rule
    int columns_fused = -1;       // TAHOE_COLUMNS_FUSED: under AUTO, 0 = column batches always go through row-major chunks, else the rule
    int table_fused = -1;         // TAHOE_TABLE_FUSED: under AUTO, 0 = typed tables always go through row-major chunks, else the rule
    bool oblivious_shap_inplace = false;  // TAHOE_OBLIVIOUS_SHAP_INPLACE = 1: an oblivious handle's explanations accumulate in phi_dev
    int vector_shap_kb = 0;       // TAHOE_VECTOR_SHAP_KB = 1 / 2 / 4 / 8: force the class block of a vector-leaf handle's TreeSHAP kernels
    int pd_chunk_rows = 0;        // TAHOE_PD_CHUNK_ROWS >= 1: grid points per chunk of tahoe_forest_predict_partial_dependence (rounded up to 64s)
    int vector_shap_grid = -1;    // TAHOE_VECTOR_SHAP_GRID: ... 0 = a workgroup loops over its class blocks, 1 = gridDim.y runs over them, -1 = the rule
};

struct tahoe_forest {
    tahoe_forest_params p{};
    int depth = 0;        // De: depth of the normalised trees, max(p.depth, 2)
    size_t n_inner = 0;   // 2^De - 1
    size_t n_leaf = 0;    // 2^De
    int bits_bytes = 0;
    int strategy = TAHOE_STRATEGY_AUTO;
    int device = 0;
    int num_cus = 0;
    int lds_limit = 0;
    int lds_levels = 0;   // ROWTILE
    int top_levels = 0;   // TILEBLOCK: levels in LDS, min(De - 2, 10)
    bool has_blocks = false;
    tahoe::InnerNode *inner = nullptr;
    float *leaf_val = nullptr;
    uint32_t *leaf_orig = nullptr;
    unsigned char *top = nullptr;  // [T][top_stride]
    uint4 *blocks = nullptr;       // [T][2^(De-2)][2]
    int *error_flag = nullptr;     // [0] set by TILERING if a bounded spin ever times out; [1] by a CSR loader that skipped an
                                   // entry whose column id is outside [0, num_cols) (tahoe_forest_check reports and clears it)
    float *csr_chunk = nullptr;    // the row-major chunk of tahoe_forest_predict_csr's fallback (csr.hip) and of the column entry
                                   // points' (columns.hip): csr_chunk_rows x num_cols floats, one buffer for both
    size_t csr_chunk_rows = 0;
    tahoe_qstate *q = nullptr;     // QRING: rank-quantised forest + row workspace (qring.hip)
    tahoe_sstate *sp = nullptr;    // non-null: this handle is a sparse forest (sparse.hip); the dense views are unused
    tahoe_pstate *pipe = nullptr;  // tahoe_forest_predict_host: chunk buffers, streams, events (created on first use)
    tahoe_wstate *wf = nullptr;    // non-null: TILERING runs the wide-row float32 form (widef.hip)
    tahoe_cstate *cs = nullptr;    // non-null: created with TAHOE_CREATE_CONTRIBS (contribs.hip)
    tahoe_istate *iv = nullptr;    // non-null: a background is set (interventional.hip)
    tahoe_astate *ap = nullptr;    // non-null: created with TAHOE_CREATE_APPROX_CONTRIBS (approx.hip)
    tahoe_ostate *ob = nullptr;    // non-null: this handle is an oblivious forest (oblivious.hip); the dense views are unused,
                                   // num_classes is the leaf dimension K and class_trees = num_trees (every tree feeds every class)
    tahoe_vstate *vl = nullptr;    // non-null: this handle is a vector-leaf forest (vector.hip); num_classes and class_trees as with ob
    tahoe_pdstate *pd = nullptr;   // non-null: a sparse handle created with TAHOE_CREATE_PARTIAL_DEPENDENCE (partial_dependence.hip)
    size_t device_bytes = 0;
    // Multi-class handle (tahoe_forest_create_multiclass): the trees are stored class-major -- internal tree p belongs to class
    // p / class_trees and is original tree (p % class_trees) * num_classes + p / class_trees -- and every consumer writes
    // sums[row * num_classes + class].  1 / num_trees on every other handle.
    int num_classes = 1;
    int class_trees = 0;
    tahoe_knobs knobs;
    // Probability-guided re-layout (TAHOE_CREATE_PROB_RELAYOUT; Struct.h:1775-1825): subtrees swapped so that the likelier
    // child is the left one, nodes carry an exchange bit.  Served by DIRECT, ROWTILE and the NARROW form of QRING.
    bool relayout = false;
    size_t relayout_swaps = 0;
    // TAHOE_CREATE_NAN_MISSING: a NaN feature value is missing, beside the sentinel (is_missing_value<true>).  Served by DIRECT,
    // ROWTILE and QRING on a dense handle, by every strategy of a sparse one.
    bool nan_missing = false;
    // Profiling: one hipEvent pair per traversal launch, read back after the stream has drained.
    bool profiling = false;
    std::vector<hipEvent_t> ev_start, ev_mid, ev_stop;  // mid: between a pre-pass kernel and the walk kernel
    size_t prof_count = 0;  // launches recorded since profiling was (re-)enabled
    // Stages of tahoe_forest_predict_staged (tahoe_forest_set_stages): num_stages strictly ascending counts of boosting rounds
    // (trees per class), on the device; null = none set
    int32_t *stages_dev = nullptr;
    size_t num_stages = 0;
    // An oblivious or vector-leaf handle created with TAHOE_CREATE_STAGED: the three staged calls are served (every other handle
    // kind serves them without a flag)
    bool staged = false;
    // An oblivious or vector-leaf handle created with TAHOE_CREATE_CSR: the three CSR calls are served (every other handle kind
    // serves them without a flag)
    bool csr = false;
};

namespace tahoe {

// Ring flags: relaxed workgroup-scope accesses (plain ds_read/ds_write that the compiler neither caches
// in a register nor reorders across the asm memory barriers around them).
__device__ __forceinline__ uint32_t lds_flag_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_flag_store(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Hand-over of values through LDS inside one workgroup: the producer stores its values, then the flag (or bumps a counter);
// the consumer reads the flag, then the values.  Both sides rely on "the LDS performs one wave's operations in issue order"
// and need only keep the COMPILER from reordering (TAHOE_LDS_RELEASE / TAHOE_LDS_ACQUIRE = compiler barriers).  Building with
// -DTAHOE_RING_RELEASE_ACQUIRE (make RING_FENCES=1) drains the wave's LDS queue at both points instead, so that a suspected
// ring failure can be bisected in one run (costs ~2 % on K3).
#ifdef TAHOE_RING_RELEASE_ACQUIRE
#define TAHOE_LDS_RELEASE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define TAHOE_LDS_ACQUIRE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#else
#define TAHOE_LDS_RELEASE() asm volatile("" ::: "memory")
#define TAHOE_LDS_ACQUIRE() asm volatile("" ::: "memory")
#endif

// ---- the LDS tree ring ("The LDS tree ring") ----
// Walker waves hand the leaf values of tree t to one consumer wave, which adds them in tree order.  LDS: vals[RING][ROWS] f32 |
// ready[RING] (tree + 1 of the entry's values) | consumed (trees the consumer has added).  Every spin is bounded.
constexpr int kRingSpinLimit = 1 << 22;

// Where the three parts lie, for the host's LDS sizes and the kernels' pointers alike
struct RingLayout {
    int entries, rows;  // trees in flight, floats per tree
    __host__ __device__ constexpr long long ready_offset() const { return 4LL * entries * rows; }
    __host__ __device__ constexpr long long consumed_offset() const { return ready_offset() + 4LL * entries; }
    __host__ __device__ constexpr long long bytes() const { return consumed_offset() + 4; }
};

// A kernel's view of its ring at `base`
template <int RING, int ROWS>
struct LdsRing {
    float *vals;
    uint32_t *ready;
    uint32_t *consumed;
    __device__ __forceinline__ explicit LdsRing(unsigned char *base)
        : vals(reinterpret_cast<float *>(base)), ready(reinterpret_cast<uint32_t *>(vals + RING * ROWS)), consumed(ready + RING)
    {
    }
    // Consumer: trees before `upto` are added -- their entries are free once the wave's reads of them have completed
    __device__ __forceinline__ void release(int upto, int lane) const
    {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) lds_flag_store(consumed, (uint32_t)upto);
    }
};

// The other steps are statement macros over a view `ring` of RING entries: a helper function is optimised on its own before it is
// inlined, and comes out of that as other code than the same statements written in the kernel.
// Every flag 0 (nothing published, nothing consumed), by the workgroup's threads tid, before the first barrier
#define TAHOE_RING_RESET(ring, RING, tid)                   \
    {                                                       \
        if ((tid) < (RING)) (ring).ready[tid] = 0u;         \
        if ((tid) == (RING)) *(ring).consumed = 0u;         \
    }
// ... for rings of more entries than the workgroup has threads (NT)
#define TAHOE_RING_RESET_STRIDED(ring, RING, tid, NT)                    \
    {                                                                    \
        for (int e_ = (tid); e_ < (RING); e_ += (NT)) (ring).ready[e_] = 0u; \
        if ((tid) == 0) *(ring).consumed = 0u;                           \
    }
// Consumer: wait until trees t0 .. t0 + nb - 1 (nb <= 64) are published; a spin-out sets dead (the caller then stops)
#define TAHOE_RING_WAIT_READY(ring, RING, t0, nb, lane, SLEEP, dead)                                                          \
    {                                                                                                                       \
        int spins_ = 0;                                                                                                     \
        for (;;) {                                                                                                          \
            const bool ok_ = (lane) >= (nb) || lds_flag_load(&(ring).ready[((t0) + (lane)) % (RING)]) == (uint32_t)((t0) + (lane) + 1); \
            if (__ballot(ok_) == ~0ull) break;                                                                              \
            if (++spins_ > kRingSpinLimit) {                                                                                \
                dead = true;                                                                                                \
                break;                                                                                                      \
            }                                                                                                               \
            __builtin_amdgcn_s_sleep(SLEEP);                                                                                \
        }                                                                                                                   \
    }
// Walker: wait until the entry of tree t is free (tree t - RING consumed); a spin-out sets dead, and the walker still publishes
#define TAHOE_RING_WAIT_FREE(ring, RING, t, SLEEP, dead)                                   \
    if ((t) >= (RING)) {                                                                   \
        int spins_ = 0;                                                                    \
        while (lds_flag_load((ring).consumed) < (uint32_t)((t) - (RING) + 1)) {            \
            if (++spins_ > kRingSpinLimit) {                                               \
                dead = true;                                                               \
                break;                                                                     \
            }                                                                              \
            __builtin_amdgcn_s_sleep(SLEEP);                                               \
        }                                                                                  \
    }
// Walker, after storing tree t's values to vals[t % RING]: the values before the flag (a wave's LDS operations are performed in
// issue order), the flag from the lane(s) `leader`
#define TAHOE_RING_PUBLISH(ring, RING, t, leader)                                                  \
    {                                                                                              \
        TAHOE_LDS_RELEASE();                                                                       \
        if (leader) lds_flag_store(&(ring).ready[(t) % (RING)], (uint32_t)((t) + 1));              \
    }

// The error flag of a wave whose ring spin ran out
__device__ __forceinline__ void ring_dead(bool dead, int lane, int *error_flag)
{
    if (dead && lane == 0) atomicOr(error_flag, 1);
}

// ---- CSR rows (tahoe_forest_predict_csr; DESIGN.md, "CSR rows") ----
// Row r holds values[k] in column indices[k] for k in [indptr[r], indptr[r + 1]), the missing sentinel everywhere else.
struct CsrView {
    const int64_t *indptr = nullptr;  // rows + 1
    const int32_t *indices = nullptr;
    const float *values = nullptr;
    size_t nnz = 0;                   // entry ranges are clamped to [0, nnz]: no read outside indices / values
    int *bad_column = nullptr;        // raised when an entry names a column outside [0, num_cols); the entry is skipped
};
constexpr int kCsrLanes = 8;  // lanes that stride over one row's entries

// indptr[row] clamped to [0, nnz]; rows past the batch get the empty range at indptr[rows]
__device__ __forceinline__ int64_t csr_row_begin(const CsrView &csr, size_t row, size_t rows)
{
    const int64_t p = csr.indptr[row < rows ? row : rows];
    return p < 0 ? 0 : (p > (int64_t)csr.nnz ? (int64_t)csr.nnz : p);
}

// The fused loader of the 64-row float32 tile kernels (NT threads): tile[f * 64 + r] = missing everywhere (ds_write_b128, no
// global traffic), barrier, then the stored entries of rows row0 .. row0 + 63 over it.  range: 65 int64 of LDS scratch that
// nothing else uses before the caller's next barrier -- the tile's indptr values, read once per workgroup.  kCsrLanes lanes
// stride over a row, so a wave scatters 8 rows at once: a ds_write_b32 banks on (address / 4) % 32 = row % 32 here, whatever
// the column, and lanes of one row therefore serialise -- 8-way with 8 lanes per row where one row per wave would be 32-way --
// while each row's indices / values are still read as 32-byte runs.  The caller's barrier after this completes the tile.
template <int NT>
__device__ __forceinline__ void csr_stage_tile(float *tile, int64_t *range, int cols, size_t row0, size_t rows, const CsrView &csr,
                                               float missing, int tid)
{
    static_assert(NT > kTileRows && NT % kCsrLanes == 0, "one thread per indptr value of the tile");
    float4 *tile4 = reinterpret_cast<float4 *>(tile);
    const float4 m4 = make_float4(missing, missing, missing, missing);
    for (int i = tid; i < cols * (kTileRows / 4); i += NT) tile4[i] = m4;
    if (tid <= kTileRows) range[tid] = csr_row_begin(csr, row0 + tid, rows);
    __syncthreads();  // the fill lands before the scatter (s_waitcnt lgkmcnt(0) + s_barrier)
    const int sub = tid % kCsrLanes;
    bool bad = false;
    for (int r = tid / kCsrLanes; r < kTileRows; r += NT / kCsrLanes) {
        const int64_t end = range[r + 1];
        for (int64_t k = range[r] + sub; k < end; k += kCsrLanes) {
            const int32_t c = csr.indices[k];
            const float v = csr.values[k];
            if ((uint32_t)c < (uint32_t)cols) tile[c * kTileRows + r] = v;
            else bad = true;
        }
    }
    if (bad) atomicOr(csr.bad_column, 1);
}

// The one-wave form of csr_stage_tile, for the 64-thread tile kernels of oblivious and vector-leaf handles (lane = row): the same
// fill, barrier and 8-lanes-per-row scatter, with no LDS scratch -- lane r keeps the clamped entry range of row row0 + r in
// registers (the tile's 65 indptr values, read once per workgroup), and the kCsrLanes lanes that scatter row r get it by a wave
// shuffle; the LDS need stays the tile's.  8 passes of 8 rows: a wave does not wait on the longest row of its tile as it would
// with "lane owns its row", and each row's indices / values are read as 32-byte runs.  The scatter lands on words that other
// lanes filled and the walk reads words that other lanes scattered: a barrier before it (here) and one after it (the caller's).
__device__ __forceinline__ void csr_stage_tile_wave(float *tile, int cols, size_t row0, size_t rows, const CsrView &csr,
                                                    float missing, int lane)
{
    float4 *tile4 = reinterpret_cast<float4 *>(tile);
    const float4 m4 = make_float4(missing, missing, missing, missing);
    for (int i = lane; i < cols * (kTileRows / 4); i += kTileRows) tile4[i] = m4;
    const int64_t begin = csr_row_begin(csr, row0 + lane, rows);
    const int64_t end = csr_row_begin(csr, row0 + lane + 1, rows);
    __syncthreads();  // the fill lands before the scatter (s_waitcnt lgkmcnt(0); a one-wave workgroup needs no s_barrier beside it)
    const int sub = lane % kCsrLanes;
    bool bad = false;
    for (int r = lane / kCsrLanes; r < kTileRows; r += kTileRows / kCsrLanes) {
        const int64_t row_end = __shfl(end, r);  // (every lane is active here: the inner loop has reconverged)
        for (int64_t k = __shfl(begin, r) + sub; k < row_end; k += kCsrLanes) {
            const int32_t c = csr.indices[k];
            const float v = csr.values[k];
            if ((uint32_t)c < (uint32_t)cols) tile[c * kTileRows + r] = v;
            else bad = true;
        }
    }
    if (bad) atomicOr(csr.bad_column, 1);
}

// ---- column-major batches (tahoe_forest_predict_columns / _column_ptrs) ----
// Column c of the batch is ptrs[c][r] (a device table of num_cols device pointers) or, with ptrs null, base[c * stride + r], for
// r in [0, rows).  Passed to kernels by value; which of the two holds is uniform over a launch and every loader below asks for a
// wave-uniform c, so the table read is a scalar load.
struct ColsView {
    const float *const *ptrs = nullptr;
    const float *base = nullptr;
    size_t stride = 0;  // floats, >= rows
    __host__ __device__ __forceinline__ const float *col(int c) const { return ptrs ? ptrs[c] : base + (size_t)c * stride; }
};

// The fused column loader of the 64-row float32 tile kernels (NWAVES waves): wave w copies columns w, w + NWAVES, ...; lane r
// loads col(c)[row0 + r] -- 64 consecutive floats, 256 bytes, per wave-load -- or takes 0.0f past the batch, as the row-major
// loader does, and stores tile[c * 64 + r]: one ds_write_b32 per lane at a lane-linear address, no bank conflict.  Eight columns
// are in flight per wave before the first store: with one, a wave waited out a table read and a global load per column, and the
// loader lost to transposing the batch first (K5's forest on 480 features).  No scratch, no barrier of its
// own: the caller's barrier after the staging completes the tile.  Nothing outside [0, rows) of a column or [0, cols) of the
// table is read.
template <int NWAVES>
__device__ __forceinline__ void cols_stage_tile(float *tile, int cols, size_t row0, size_t rows, const ColsView &cv, int wave, int lane)
{
    constexpr int U = 8;
    const bool row_ok = row0 + lane < rows;
    for (int c0 = __builtin_amdgcn_readfirstlane(wave); c0 < cols; c0 += U * NWAVES) {  // (c in an SGPR: col(c) is a scalar load)
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * NWAVES;
            v[u] = 0.0f;
            if (c < cols && row_ok) v[u] = cv.col(c)[row0 + lane];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * NWAVES;
            if (c < cols) tile[c * kTileRows + lane] = v[u];
        }
    }
}

// ---- typed, nullable columns (tahoe_forest_predict_table) ----
// Column c of the batch is described by cols[c], a device copy of the caller's tahoe_column (tahoe_table_create has validated
// every field on the host).  Passed to kernels by value.
struct TableView {
    const tahoe_column *cols = nullptr;
};

// Row r of column c as the float32 the walks compare: the one place that reads a validity bit or converts a column element.
// A null is `missing` and the element under it is not read.  The bitmap is read by the byte that holds the row's bit and the data
// by the element: nothing outside [offset >> 3, (offset + rows - 1) >> 3] of validity or [offset, offset + rows) of data is touched
// for r in [0, rows).  The conversions are C's: round to nearest even from float64 and the 64-bit integers (a float32 subnormal
// result is kept, the kernels run with denormals on), float64 overflow to +-inf, NaN stays NaN, everything narrower is exact.
// Where c is wave-uniform the descriptor sits in SGPRs and the switch is a uniform branch.  N rows of one column at a time
// (out[n] = row r[n]): one switch around N loads, not N switches -- the quantise kernels keep several rows in flight per column,
// and a switch per load made quantize_pair_kernel spill.
template <class T, int N>
__device__ __forceinline__ void table_load_as(const tahoe_column &c, const size_t (&i)[N], const bool (&valid)[N], float missing,
                                              float (&out)[N])
{
#pragma unroll
    for (int n = 0; n < N; ++n) {
        out[n] = missing;
        if (valid[n]) out[n] = (float)static_cast<const T *>(c.data)[i[n]];
    }
}
template <int N>
__device__ __forceinline__ void table_load(const tahoe_column &c, const size_t (&r)[N], float missing, float (&out)[N])
{
    size_t i[N];
    bool valid[N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        i[n] = (size_t)c.offset + r[n];
        valid[n] = true;
        if (c.validity) valid[n] = ((c.validity[i[n] >> 3] >> (i[n] & 7u)) & 1u) != 0u;
    }
    switch (c.type) {
    case TAHOE_COL_FLOAT32: table_load_as<float>(c, i, valid, missing, out); break;
    case TAHOE_COL_FLOAT64: table_load_as<double>(c, i, valid, missing, out); break;
    case TAHOE_COL_FLOAT16: table_load_as<_Float16>(c, i, valid, missing, out); break;
    case TAHOE_COL_INT8: table_load_as<int8_t>(c, i, valid, missing, out); break;
    case TAHOE_COL_INT16: table_load_as<int16_t>(c, i, valid, missing, out); break;
    case TAHOE_COL_INT32: table_load_as<int32_t>(c, i, valid, missing, out); break;
    case TAHOE_COL_INT64: table_load_as<int64_t>(c, i, valid, missing, out); break;
    case TAHOE_COL_UINT8: table_load_as<uint8_t>(c, i, valid, missing, out); break;
    case TAHOE_COL_UINT16: table_load_as<uint16_t>(c, i, valid, missing, out); break;
    case TAHOE_COL_UINT32: table_load_as<uint32_t>(c, i, valid, missing, out); break;
    default: table_load_as<uint64_t>(c, i, valid, missing, out); break;  // TAHOE_COL_UINT64 (create refuses every other code)
    }
}
// ... one row
__device__ __forceinline__ float table_load(const tahoe_column &c, size_t r, float missing)
{
    const size_t rr[1] = {r};
    float out[1];
    table_load<1>(c, rr, missing, out);
    return out[0];
}

// hipFuncAttributeMaxDynamicSharedMemorySize is per function and process-wide, not per handle: always raise it to
// the device limit (less the kernel's static LDS), so that handles of different shapes can coexist in one process.
inline hipError_t allow_max_lds(const void *fn, int limit)
{
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, fn);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, limit - (int)a.sharedSizeBytes);
}

// The launch switch over (write leaf indices) x (multi-class): calls fn(wl, mc) with std::true_type / std::false_type for the
// runtime pair, so that a launch site names its kernel once, as kernel<decltype(wl)::value, ..., decltype(mc)::value>.
// with_leaf serves the kernels that have no multi-class flag.
template <class Fn>
inline void with_leaf_mc(bool leaf, bool mc, Fn &&fn)
{
    if (mc) {
        if (leaf) fn(std::true_type{}, std::true_type{});
        else fn(std::false_type{}, std::true_type{});
    } else if (leaf) {
        fn(std::true_type{}, std::false_type{});
    } else {
        fn(std::false_type{}, std::false_type{});
    }
}
// ... x (NaN is missing: TAHOE_CREATE_NAN_MISSING): fn(wl, mc, nanm)
template <class Fn>
inline void with_leaf_mc_nanm(bool leaf, bool mc, bool nanm, Fn &&fn)
{
    with_leaf_mc(leaf, mc, [&](auto wl, auto mc_c) {
        if (nanm) fn(wl, mc_c, std::true_type{});
        else fn(wl, mc_c, std::false_type{});
    });
}
template <class Fn>
inline void with_leaf(bool leaf, Fn &&fn)
{
    if (leaf) fn(std::true_type{});
    else fn(std::false_type{});
}
// allow_max_lds for both leaf-index instantiations of one kernel form: kern(wl) returns the kernel's address for wl as above.
template <class Kern>
inline hipError_t allow_max_lds_leaf(Kern &&kern, int limit)
{
    const hipError_t e = allow_max_lds(reinterpret_cast<const void *>(kern(std::false_type{})), limit);
    return e != hipSuccess ? e : allow_max_lds(reinterpret_cast<const void *>(kern(std::true_type{})), limit);
}

// A process that drives several GPUs (one handle per device) calls predict with any device current: the launches
// must be issued with the handle's device current.  Restores the caller's device on scope exit.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int want)
    {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != want && hipSetDevice(want) == hipSuccess) prev = cur;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// hipMalloc max(n, 1) elements, counted in *total (the handle's device_bytes), and copy the n elements of src there
template <typename T>
inline hipError_t upload(T **dst, const T *src, size_t n, size_t *total)
{
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(dst), bytes);
    if (e != hipSuccess) return e;
    *total += bytes;
    if (n) e = hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
}
template <typename T>
inline hipError_t upload(T **dst, const std::vector<T> &src, size_t *total)
{
    return upload(dst, src.data(), src.size(), total);
}
// TAHOE_ERR_HIP, "<what> failed: <HIP error>", unless e is hipSuccess
inline tahoe_status hip_status(hipError_t e, const char *what)
{
    return e == hipSuccess ? TAHOE_OK : fail(TAHOE_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
}

// ---- creating a handle (forest.hip); every refusal of a bad argument comes before the first HIP call ----
// The owner of a handle under construction: a failed create destroys what it has built so far, a finished one is released.
struct ForestDeleter {
    void operator()(tahoe_forest *f) const { tahoe_forest_destroy(f); }
};
using ForestPtr = std::unique_ptr<tahoe_forest, ForestDeleter>;
// check_params (BaseTahoeTest.h:490-516), the rules of dense and sparse forests alike; have_nodes: the caller passed its node
// array(s), named `nodes` in the refusal
tahoe_status check_params(const tahoe_forest_params *p, int num_classes, bool have_nodes, const char *nodes);
// The class and output rules of tahoe_forest_create_multiclass and tahoe_sparse_forest_create_ex
tahoe_status check_classes(const tahoe_forest_params *p, int num_classes);
// A handle on the current device with what dense and sparse handles share: params, classes, device limits, the error flag, knobs
tahoe_status open_handle(const tahoe_forest_params *p, int num_classes, ForestPtr &f);
// The last step of every create: the SHAP builds the flags ask for (contribs(), then approx()), then the handle goes to *out
template <class Contribs, class Approx>
inline tahoe_status finish_create(ForestPtr &f, unsigned flags, tahoe_forest **out, Contribs &&contribs, Approx &&approx)
{
    tahoe_status s = TAHOE_OK;
    if (flags & TAHOE_CREATE_CONTRIBS) s = contribs();
    if (s == TAHOE_OK && (flags & TAHOE_CREATE_APPROX_CONTRIBS)) s = approx();
    if (s == TAHOE_OK) *out = f.release();
    return s;
}
// The refusals of TAHOE_CREATE_NAN_MISSING, for every create and before a device is touched.  unserved: the handle kind of a create
// that does not take the flag at all, else null: the flag is then refused beside the explanation and partial-dependence flags,
// whose kernels do not implement the rule
inline tahoe_status check_nan_missing_flags(unsigned flags, const char *unserved)
{
    if (!(flags & TAHOE_CREATE_NAN_MISSING)) return TAHOE_OK;
    if (unserved) return fail(TAHOE_ERR_INVALID_ARG, "TAHOE_CREATE_NAN_MISSING is not served on %s handle", unserved);
    if (flags & (TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_APPROX_CONTRIBS | TAHOE_CREATE_CAT_CONTRIBS | TAHOE_CREATE_PARTIAL_DEPENDENCE))
        return fail(TAHOE_ERR_INVALID_ARG, "TAHOE_CREATE_NAN_MISSING does not combine with TAHOE_CREATE_CONTRIBS, _APPROX_CONTRIBS, "
                                           "_CAT_CONTRIBS or _PARTIAL_DEPENDENCE (flags 0x%x): those kernels do not implement the rule",
                    flags);
    return TAHOE_OK;
}
// TAHOE_OK when handle f can run `strategy` (a valid TAHOE_STRATEGY_*), else the refusal (TAHOE_ERR_UNSUPPORTED) saying why.
// AUTO always resolves to an available strategy.
tahoe_status strategy_available(const tahoe_forest *f, int strategy);
// tahoe_forest_predict on device rows (forest.hip).  With csr the rows come from there through the fused loader of the tile
// kernel of csr_strategy (a value csr_fused_strategy returned) and `data` is not read.
// With cols the rows come from column-major buffers instead (`data` is not read) through the kernel of csr_strategy (a value
// columns_fused_strategy returned): QRING's quantise pass or a tile kernel's column loader.
// With table they come from typed, nullable columns through QRING's quantise pass (csr_strategy is what table_fused_strategy
// returned: QRING).
tahoe_status predict_rows(tahoe_forest *f, float *preds, const float *data, size_t rows, hipStream_t stream,
                          const CsrView *csr = nullptr, int csr_strategy = 0, const ColsView *cols = nullptr,
                          const TableView *table = nullptr);
// The strategy whose fused CSR kernel serves a batch of `rows` rows with nnz stored entries (ROWTILE, or TILEBLOCK on a sparse
// handle; ROWTILE on an oblivious or vector-leaf handle of TAHOE_CREATE_CSR), or -1: the batch is densified in chunks and takes the handle's own path (csr.hip)
int csr_fused_strategy(const tahoe_forest *f, size_t rows, size_t nnz);
void csr_destroy(tahoe_forest *f);
// The row-major chunk buffer both fallbacks stage into (csr.hip): rows per chunk under TAHOE_CSR_CHUNK_MB, and the buffer grown to
// hold min(rows, cap) rows (`fn` names the caller in a refusal)
size_t csr_chunk_cap(const tahoe_forest *f);
tahoe_status csr_reserve_chunk(tahoe_forest *f, size_t rows, const char *fn);
// One event triple for a whole chunked call (staging kernels included) instead of one per chunk: the inner launches are not timed
struct ProfilingPause {
    tahoe_forest *f;
    bool was;
    explicit ProfilingPause(tahoe_forest *f_) : f(f_), was(f_->profiling) { f->profiling = false; }
    ~ProfilingPause() { f->profiling = was; }
};
// The strategy whose kernel reads a batch of `rows` rows straight from columns (QRING: the quantise pass; ROWTILE, or TILEBLOCK
// on a sparse handle: the tile loader), or -1: the batch is transposed in chunks and takes the handle's own path (columns.hip)
int columns_fused_strategy(const tahoe_forest *f, size_t rows);
// ... straight from a typed table (tahoe_forest_predict_table): QRING where the handle runs QRING on a batch of this size (the
// quantise pass converts as it loads), or -1: chunks (table.hip)
int table_fused_strategy(const tahoe_forest *f, size_t rows);

// Is feature value x a missing value?  The one definition, for the float32 walks and the quantise pass alike.  NANM: the handle
// was created with TAHOE_CREATE_NAN_MISSING -- any NaN is missing beside the sentinel's band.  The two tests
// stay two compares: !(fabsf(x - missing) > eps) would also call +inf missing under missing = +inf (inf - inf is NaN) and
// everything missing under missing = NaN.  Without NANM this is the compare every kernel has always made.
template <bool NANM = false>
__device__ __forceinline__ bool is_missing_value(float x, float missing)
{
    const bool band = fabsf(x - missing) <= kMissingEps;
    if constexpr (NANM) return band || x != x;
    else return band;
}
// The branch rule of infer_one_tree, BaseTahoeTest.h:450-453: 1 = right child.
template <bool NANM = false>
__device__ __forceinline__ uint32_t go_right(float x, float thr, bool def_left, float missing)
{
    const bool is_missing = is_missing_value<NANM>(x, missing);
    const bool cond = is_missing ? !def_left : (x >= thr);
    return cond ? 1u : 0u;
}
// ... at a categorical split (tahoe_sparse_forest_create_cat).  pool[off] = members_left << 31 | nwords, the split's nwords
// bitset words follow it; pool_words bounds the word read (an empty or short set may sit at the pool's end).  Below 2^24 a
// float32 is exact and (uint32_t)x truncates, so x < 32 * nwords <=> (c >> 5) < nwords; NaN fails x >= 0.0f.
template <bool NANM = false>
__device__ __forceinline__ uint32_t go_right_cat(float x, const uint32_t *__restrict__ pool, uint32_t off, uint32_t pool_words,
                                                 bool def_left, float missing)
{
    const bool is_missing = is_missing_value<NANM>(x, missing);
    const bool in = x >= 0.0f && x < 16777216.0f;
    const uint32_t c = in ? (uint32_t)x : 0u;
    const uint32_t wi = off + 1u + (c >> 5);
    const uint32_t head = pool[off];
    const uint32_t word = wi < pool_words ? pool[wi] : 0u;  // issued beside the header read: one round trip
    const bool member = in && (c >> 5) < (head & 0xfffffu) && ((word >> (c & 31u)) & 1u) != 0u;
    const bool cond = is_missing ? !def_left : (member != ((head >> 31) != 0u));
    return cond ? 1u : 0u;
}
// The device copy of a categorical handle's sparse nodes (sparse.hip builds it): a categorical split carries kSCat in `bits`
// (its fid then has 29 bits, num_cols <= 2^29) and its pool entry's index in `val`
constexpr int32_t kSCat = (int32_t)(1u << 29);
constexpr int32_t kSCatFidMask = (int32_t)((1u << 29) - 1u);
// ... on a heap record: the stored children are swapped where the exchange bit is set (Struct.h:1060-1063: cond = !cond)
template <bool NANM = false>
__device__ __forceinline__ uint32_t go_right_meta(float x, float thr, uint32_t meta, float missing)
{
    return go_right<NANM>(x, thr, (meta >> 31) != 0, missing) ^ ((meta >> 30) & 1u);
}
// The argument checks of tahoe_categorical_splits, shared by the creates that take them (sparse.hip)
tahoe_status check_cat_args(const tahoe_categorical_splits *c, int num_nodes);

// The split record of an oblivious handle (oblivious.hip, oblivious_shap.hip): an InnerNode {thr, fid | def_left << 31} whose bit
// 30 -- the exchange bit of a heap record, which no oblivious handle sets -- says "category set" (tahoe_oblivious_forest_create_cat).
// Such a record has a 28-bit fid (num_cols <= 2^28 on a handle with sets) and one of two kinds:
//   inline  (bit 29 clear): the set's only word sits where thr was (nwords <= 1; an empty set is the word 0), bit 28 = members_left
//   pooled  (bit 29 set):   thr's bits are the index of the set's header in the handle's pool, laid out as go_right_cat reads it
// The record sits at a wave-uniform address, so the kind is wave-uniform and the branch on it diverges nowhere.
constexpr uint32_t kObCat = 1u << 30;
constexpr uint32_t kObCatPooled = 1u << 29;
constexpr uint32_t kObCatLeft = 1u << 28;
constexpr uint32_t kObCatFidMask = (1u << 28) - 1u;
__host__ __device__ __forceinline__ uint32_t ob_split_fid(uint32_t meta)
{
    return meta & ((meta & kObCat) ? kObCatFidMask : kMetaFidMask);
}
// The bit level l adds to the leaf index: the one definition of the branch rule of an oblivious level, for the walk and for every
// explanation kernel.  CAT == false is a handle without sets: go_right_meta and nothing else.
template <bool CAT>
__device__ __forceinline__ uint32_t ob_split_bit(const InnerNode n, float x, float missing, const uint32_t *__restrict__ pool,
                                                 uint32_t pool_words)
{
    if (!CAT || !(n.meta & kObCat)) return go_right_meta(x, n.thr, n.meta, missing);
    const bool def_left = (n.meta >> 31) != 0u;
    if (n.meta & kObCatPooled) return go_right_cat(x, pool, __float_as_uint(n.thr), pool_words, def_left, missing);
    // go_right_cat on a set of one word held in a register: x < 32 <=> (uint32_t)x < 32 for the x >= 0 that pass
    const bool is_missing = fabsf(x - missing) <= kMissingEps;
    const bool in = x >= 0.0f && x < 32.0f;
    const uint32_t c = in ? (uint32_t)x : 0u;
    const bool member = in && ((__float_as_uint(n.thr) >> c) & 1u) != 0u;
    const bool cond = is_missing ? !def_left : (member != ((n.meta & kObCatLeft) != 0u));
    return cond ? 1u : 0u;
}

// Multi-class handles store the trees class-major: internal tree p (class p / class_trees) is original tree
// (p % class_trees) * num_classes + p / class_trees.  Leaf indices are written in the original numbering.
__device__ __forceinline__ int mc_orig_tree(int p, int num_classes, int class_trees)
{
    const int c = p / class_trees;
    return (p - c * class_trees) * num_classes + c;
}

// QRING entry points (qring.hip).  h_real[i] != 0 marks heap records that exist in the original tree
// (padding below an early leaf is not real and contributes no threshold).
tahoe_status qring_build(tahoe_forest *f, const std::vector<InnerNode> &h_inner, const std::vector<unsigned char> &h_real,
                         const std::vector<float> &h_leaf);
void qring_destroy(tahoe_forest *f);
int qring_walkers(const tahoe_forest *f);  // walker waves the kernel would use; 0 = strategy unavailable
long long qring_lds_bytes(const tahoe_forest *f);
// mid_event (optional) is recorded between the quantise kernel and the walk kernel
tahoe_status qring_launch(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data, size_t rows,
                          hipStream_t stream, hipEvent_t mid_event, const float *sums_in = nullptr, const ColsView *cols = nullptr,
                          const TableView *table = nullptr);
tahoe_status qring_reserve(tahoe_forest *f, size_t rows);
int qwide_rows(const tahoe_forest *f);   // rows per tile of the wide-row form; 0 = not used
int qwide_chains(const tahoe_forest *f); // ... and the trees a lane walks at once (1 or 3)
bool qring_lds_tile(const tahoe_forest *f);
bool qring_regions(const tahoe_forest *f);  // region form: tiles of 192 (or 128) rows as 64-row regions
bool qring_six16(const tahoe_forest *f);    // ... <= 128 features: 16-KiB region stride, 384-row tiles also on u16 codes
bool qring_code8(const tahoe_forest *f);    // ... on u8 codes (<= 254 thresholds per feature): tiles of 384 rows as 128-row regions
int qring_groups(const tahoe_forest *f);  // tree groups with separate quantisation (1 for most forests)
int qring_form(const tahoe_forest *f, size_t rows);  // TAHOE_FORM_* of the launch for a batch of `rows` rows

// sparse forests (sparse.hip)
bool sparse_tile_fits(const tahoe_forest *f);
tahoe_status sparse_launch(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data, size_t rows,
                           hipStream_t stream, int strategy, const float *sums_in = nullptr, const CsrView *csr = nullptr,
                           const ColsView *cols = nullptr, const TableView *table = nullptr);
int sparse_top_waves(const tahoe_forest *f);
// tahoe_forest_predict_staged on a sparse handle: the walk of `strategy` (DIRECT, ROWTILE or TILEBLOCK) with the stage stores to
// out[rows][num_stages][num_classes]; sparse_allow_staged_lds lets those kernels take the device's LDS (set_stages calls it)
tahoe_status sparse_launch_staged(tahoe_forest *f, float *out, const float *data, size_t rows, hipStream_t stream, int strategy);
tahoe_status sparse_allow_staged_lds(const tahoe_forest *f);
bool sparse_q_available(const tahoe_forest *f);  // the walk on quantised codes (strategy QRING on a sparse handle)
bool sparse_has_cats(const tahoe_forest *f);     // categorical splits (tahoe_sparse_forest_create_cat): no QRING
void sparse_destroy(tahoe_forest *f);
void sparse_device_views(const tahoe_forest *f, const tahoe_sparse_node **nodes, const int32_t **trees);  // the stored nodes and roots
void sparse_cat_view(const tahoe_forest *f, const uint32_t **pool, uint32_t *pool_words);  // the split pool (null / 0: no splits)
void pipeline_destroy(tahoe_forest *f);
// TILERING for rows too wide for a 64-row float32 tile (widef.hip)
tahoe_status widef_build(tahoe_forest *f, const std::vector<InnerNode> &h_inner, const std::vector<unsigned char> &h_real,
                         const std::vector<float> &h_leaf);
int widef_rows(const tahoe_forest *f);  // rows per tile; 0 = unavailable
long long widef_lds_bytes(const tahoe_forest *f);   // LDS per workgroup of the form the launch takes
int widef_stream_slots(const tahoe_forest *f);      // row slots of the row-streaming form; 0 = the tile form runs
int widef_stream_levels(const tahoe_forest *f);     // ... and the levels of all trees it keeps in LDS
float widef_stream_tie_estimate(const tahoe_forest *f);  // estimated share of key compares that tie (0 when the form was never sized)
tahoe_status widef_launch(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data, size_t rows, hipStream_t stream,
                          const float *sums_in);
void widef_destroy(tahoe_forest *f);
tahoe_status widef_reserve(tahoe_forest *f, size_t rows);

// per-feature contributions (contribs.hip).  contribs_validate runs on the caller's nodes before any device is touched;
// contribs_build builds the path tables of a validated forest from the caller's nodes (not the re-laid-out ones).
tahoe_status contribs_validate(const tahoe_dense_node *nodes, const tahoe_forest_params *p);
tahoe_status contribs_build(tahoe_forest *f, const tahoe_dense_node *nodes);
// ... the same for a sparse forest whose structure check has passed: covers[i] is the cover of nodes[i]; with path_limit the
// validation also refuses (TAHOE_ERR_UNSUPPORTED) a leaf whose path has more than 31 distinct features; without check_covers
// covers is not read (it may be null) and the path check alone runs
tahoe_status contribs_validate_sparse(const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers,
                                      const tahoe_forest_params *p, bool path_limit, bool check_covers = true);
// The bias column of tahoe_forest_predict_contribs (bias[c], float64 on the host, rounded once) and the AVG divisor (div[c]) of
// every class, from the caller's validated trees; f->p, num_classes and class_trees must be set
void contribs_bias(const tahoe_forest *f, const tahoe_dense_node *nodes, std::vector<float> &bias, std::vector<float> &div);
void contribs_bias_sparse(const tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers,
                          std::vector<float> &bias, std::vector<float> &div);
// cats: the categorical splits of the caller's nodes (TAHOE_CREATE_CAT_CONTRIBS), or null; their path elements carry category sets
tahoe_status contribs_build_sparse(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers,
                                   const tahoe_categorical_splits *cats = nullptr);
void contribs_destroy(tahoe_forest *f);
// oblivious forests (oblivious.hip): strategy ROWTILE = oblivious_tile_kernel, DIRECT = oblivious_direct_kernel
bool oblivious_tile_fits(const tahoe_forest *f);
// csr (optional; a handle of TAHOE_CREATE_CSR, strategy ROWTILE, predictions only): the tile is staged from there, `data` is not read
tahoe_status oblivious_launch(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data, size_t rows, hipStream_t stream,
                              int strategy, const float *sums_in, const CsrView *csr = nullptr);
// tahoe_forest_predict_staged on a handle created with TAHOE_CREATE_STAGED: the same walk (DIRECT or ROWTILE) with the stage stores
// to out[rows][num_stages][K]; oblivious_allow_staged_lds lets its tile kernel take the device's LDS (set_stages calls it)
tahoe_status oblivious_launch_staged(tahoe_forest *f, float *out, const float *data, size_t rows, hipStream_t stream, int strategy);
tahoe_status oblivious_allow_staged_lds(const tahoe_forest *f);
void oblivious_destroy(tahoe_forest *f);
// ... its explanations (oblivious_shap.hip).  oblivious_serves: was the handle created with `flag` (TAHOE_CREATE_CONTRIBS,
// TAHOE_CREATE_APPROX_CONTRIBS or TAHOE_CREATE_INTERACTIONS)?  oblivious_predict_shap: the call of one of the first two flags on
// such a handle, oblivious_predict_interactions: that of the third; entry checks included (fn: the call's name)
bool oblivious_serves(const tahoe_forest *f, unsigned flag);
tahoe_status oblivious_predict_shap(tahoe_forest *f, unsigned flag, float *phi_dev, const float *data_dev, size_t rows,
                                    hipStream_t stream, const char *fn);
tahoe_status oblivious_predict_interactions(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                            const char *fn);
// ... its interventional TreeSHAP (TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL, which oblivious_serves answers too): the bodies of
// tahoe_forest_set_background and tahoe_forest_predict_contribs_interventional on such a handle, after the refusals of a NULL handle,
// a missing flag and (set_background) a NULL background
tahoe_status oblivious_set_background(tahoe_forest *f, const float *bg_dev, size_t bg_rows, hipStream_t stream);
tahoe_status oblivious_predict_interventional(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                              const char *fn);
// The refusal of the entry points an oblivious handle does not serve (fn: the entry point's name); TAHOE_OK on every other handle
inline tahoe_status refuse_oblivious(const tahoe_forest *f, const char *fn)
{
    if (!f->ob) return TAHOE_OK;
    return fail(TAHOE_ERR_UNSUPPORTED, "%s: not served on an oblivious handle (tahoe_oblivious_forest_create)", fn);
}
// vector-leaf forests (vector.hip): strategy ROWTILE = vector_tile_kernel, DIRECT = vector_direct_kernel
bool vector_tile_fits(const tahoe_forest *f);
// (csr: as oblivious_launch's)
tahoe_status vector_launch(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data, size_t rows, hipStream_t stream,
                           int strategy, const CsrView *csr = nullptr);
// ... and the same pair for a vector-leaf handle created with TAHOE_CREATE_STAGED
tahoe_status vector_launch_staged(tahoe_forest *f, float *out, const float *data, size_t rows, hipStream_t stream, int strategy);
tahoe_status vector_allow_staged_lds(const tahoe_forest *f);
void vector_destroy(tahoe_forest *f);
// ... its TreeSHAP (vector_shap.hip).  vector_serves_contribs: was the handle created with TAHOE_CREATE_CONTRIBS?
// vector_predict_contribs: tahoe_forest_predict_contribs on such a handle, entry checks included (fn: the call's name)
bool vector_serves_contribs(const tahoe_forest *f);
tahoe_status vector_predict_contribs(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                     const char *fn);
// ... its interventional TreeSHAP (vector_iv.hip).  vector_serves_interventional: was the handle created with
// TAHOE_CREATE_INTERVENTIONAL?  vector_predict_interventional: the launch of tahoe_forest_predict_contribs_interventional on such a
// handle with a background, after the entry checks (fn: the call's name); vector_iv_allow_lds: its kernel may take the device's LDS
bool vector_serves_interventional(const tahoe_forest *f);
tahoe_status vector_predict_interventional(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                           const char *fn);
hipError_t vector_iv_allow_lds(const tahoe_forest *f);
// ... its SHAP interaction values (vector_inter.hip).  vector_serves_interactions: was the handle created with
// TAHOE_CREATE_VECTOR_INTERACTIONS?  vector_predict_interactions: tahoe_forest_predict_interactions on such a handle, entry checks
// included (fn: the call's name)
bool vector_serves_interactions(const tahoe_forest *f);
tahoe_status vector_predict_interactions(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                         const char *fn);
// The refusal of the entry points a vector-leaf handle does not serve (fn: the entry point's name); TAHOE_OK on every other handle
inline tahoe_status refuse_vector(const tahoe_forest *f, const char *fn)
{
    if (!f->vl) return TAHOE_OK;
    return fail(TAHOE_ERR_UNSUPPORTED, "%s: not served on a vector-leaf handle (tahoe_vector_forest_create)", fn);
}
// ... of the three staged entry points: both refusals give way on a handle created with TAHOE_CREATE_STAGED
inline tahoe_status refuse_unstaged(const tahoe_forest *f, const char *fn)
{
    if (f->staged) return TAHOE_OK;
    if (const tahoe_status s = refuse_oblivious(f, fn)) return s;
    return refuse_vector(f, fn);
}
// ... of the three CSR entry points: both refusals give way on a handle created with TAHOE_CREATE_CSR
inline tahoe_status refuse_no_csr(const tahoe_forest *f, const char *fn)
{
    if (f->csr) return TAHOE_OK;
    if (const tahoe_status s = refuse_oblivious(f, fn)) return s;
    return refuse_vector(f, fn);
}
// The first refusal of every TreeSHAP entry point (fn: its name): TAHOE_ERR_UNSUPPORTED unless the handle has path tables
inline tahoe_status need_path_tables(const tahoe_forest *f, const char *fn)
{
    if (f->cs) return TAHOE_OK;
    if (const tahoe_status s = refuse_oblivious(f, fn)) return s;
    if (const tahoe_status s = refuse_vector(f, fn)) return s;
    if (f->sp)
        return fail(TAHOE_ERR_UNSUPPORTED, "%s: a sparse handle created without TAHOE_CREATE_CONTRIBS has no node covers and no path "
                                           "tables (tahoe_sparse_forest_create_ex)", fn);
    return fail(TAHOE_ERR_UNSUPPORTED, "%s: the handle was created without TAHOE_CREATE_CONTRIBS and has no path tables", fn);
}
// ... of the two interventional entry points: the path tables, a vector-leaf handle's bins of TAHOE_CREATE_INTERVENTIONAL, or an
// oblivious handle's tables of TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL
inline tahoe_status need_background_tables(const tahoe_forest *f, const char *fn)
{
    if (vector_serves_interventional(f) || oblivious_serves(f, TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL)) return TAHOE_OK;
    return need_path_tables(f, fn);
}
// TAHOE_ERR_INVALID_ARG unless the output of a SHAP entry point, rows x classes x (num_cols + 1)^k floats, fits in size_t
inline tahoe_status check_shap_out(const tahoe_forest *f, size_t rows, int k, const char *fn)
{
    const size_t F1 = (size_t)f->p.num_cols + 1, limit = SIZE_MAX / sizeof(float);
    size_t per_row = (size_t)f->num_classes;
    bool over = false;
    for (int i = 0; i < k && !over; ++i) {
        over = per_row > limit / F1;
        per_row *= F1;
    }
    if (over || rows > limit / per_row)
        return fail(TAHOE_ERR_INVALID_ARG, "%s: rows x classes x (num_cols + 1)%s floats overflow size_t (rows %zu)", fn,
                    k == 2 ? "^2" : "", rows);
    return TAHOE_OK;
}
// interventional TreeSHAP (interventional.hip): frees the background, if any
void interventional_destroy(tahoe_forest *f);
// ... masks[b][r] <- the ballot of bin b's lanes whose element background row r follows (background_mask_kernel<false>: elements
// without category sets), for the `bins` > 0 bins at elems; rank-0 lanes give 0, so a root element's .x is never read as a bound
void launch_background_masks(unsigned long long *masks, const float *bg_dev, size_t bg_rows, int num_cols, size_t bins,
                             const uint4 *elems, float missing, hipStream_t stream);
// Saabas contributions (approx.hip).  approx_build runs on a dense handle's final layout (h_inner / h_real after re-layout,
// internal tree order) and the caller's validated nodes; approx_build_sparse on the caller's validated sparse trees.
tahoe_status approx_build(tahoe_forest *f, const tahoe_dense_node *nodes, const std::vector<InnerNode> &h_inner,
                          const std::vector<unsigned char> &h_real);
tahoe_status approx_build_sparse(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers);
void approx_destroy(tahoe_forest *f);
// partial dependence (partial_dependence.hip).  pd_validate_sparse: the checks of TAHOE_CREATE_PARTIAL_DEPENDENCE on the caller's
// structure-checked trees -- covers, their float32 sums, no leaf deeper than 32 edges -- before a device is touched;
// pd_build_sparse: the per-node cover fractions in the stored node order and the workspace, both counted in device_bytes
tahoe_status pd_validate_sparse(const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers, const tahoe_forest_params *p);
tahoe_status pd_build_sparse(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers);
void pd_destroy(tahoe_forest *f);
// The node means of one sparse-layout tree of n nodes (tn, with its covers tc), bottom-up in float64: children lie after their
// parent; leaf(i) is the value of leaf i.  The one definition behind the deltas of approx_build_sparse and of a vector-leaf
// handle (vector_approx.hip), which must agree in every bit.
template <class Leaf>
inline void saabas_means(const tahoe_sparse_node *tn, const float *tc, size_t n, std::vector<double> &E, Leaf &&leaf)
{
    E.assign(n, 0.0);
    for (size_t i = n; i-- > 0;) {
        if (tn[i].bits < 0) {
            E[i] = (double)leaf(i);
            continue;
        }
        const size_t l = (size_t)tn[i].left_idx;
        const double wl = tc[l], wr = tc[l + 1];
        E[i] = (wl * E[l] + wr * E[l + 1]) / (wl + wr);
    }
}
// ... and the delta a child c of node i carries
inline float saabas_delta(const std::vector<double> &E, size_t c, size_t i) { return (float)(E[c] - E[i]); }
// Saabas contributions on a vector-leaf handle (vector_approx.hip).  vector_serves_approx: was the handle created with
// TAHOE_CREATE_VECTOR_APPROX?  vector_predict_approx: tahoe_forest_predict_contribs_approx on such a handle, entry checks included
bool vector_serves_approx(const tahoe_forest *f);
tahoe_status vector_predict_approx(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                   const char *fn);
// The bias column of a vector-leaf handle (bias[k]; contribs.hip): what tahoe_forest_predict_contribs and _predict_contribs_approx
// both write, from the caller's validated trees and covers; div[k] as contribs_bias's
void contribs_bias_vector(const tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *leaf_values,
                          const float *covers, std::vector<float> &bias, std::vector<float> &div);

}  // namespace tahoe
