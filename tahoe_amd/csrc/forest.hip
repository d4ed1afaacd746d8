// Forest handle, device layout and traversal kernels for gfx950 (MI355X).
//
// What this replaces in the reference (file:line into sampathrg/Tahoe):
//   dense_forest / dense_adaptive_forest  (init, infer, predict)     Struct.h:802-861, :1710-2210
//   the walkers infer_one_tree_* and kernels infer_k_* / infer_adaptive_reorg_*   Struct.h:359-1704
//   cub::BlockReduce / DeviceSegmentedReduce call sites (table 2b of SURVEY.md)  -> ordered
//     per-row accumulation through LDS (no tree-parallel float reduction, see "sum order")
//   transform_k                                                      Struct.h:196-209
//
// Device layout, built once at create ("perfect-tree" normalisation):
//   Every tree is normalised to a perfect binary tree of depth De = max(depth, 2): a leaf found
//   above the bottom level is pushed down -- all bottom-level descendants inherit its value and
//   remember its original heap index.  A walk is then exactly De compare-and-step iterations with
//   no leaf test, so the 64 lanes of a wave never diverge.  Three views of the same tree t:
//     (1) heap records          inner[t][2^De - 1] {float thr; uint32 meta}, meta = fid | exchange<<30 | def_left<<31
//                               leaf_val[t][2^De] float, leaf_orig[t][2^De] uint32 (original heap index)
//     (2) top, SoA (<=10 levels) top[t]: thr[2^L] float | meta[2^L] uint16 (fid | def_left<<15), indexed by
//                               1-based heap position: staged whole into LDS by the TILEBLOCK kernel
//     (3) bottom blocks          blk[t][2^(De-2)] 32 B: {thr0, thr1, thr2, 3 x (fid:9 | def_left:1)} {leaf0..3}
//                               = the subtree of the last two inner levels and its four leaves, fetched
//                               with two 16-byte gathers that share one cache line
//   Views (2) and (3) exist when num_cols <= 512 (9-bit feature ids).
//
// Sum order: the CPU predictor adds leaf values in tree order 0..T-1 in float32
// (BaseTahoeTest.h:462-466).  Every kernel here adds them in exactly that order per row, so the raw
// sums are bit-identical to the CPU's, not merely within tolerance.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <mutex>
#include <vector>

#include "forest_internal.h"

namespace tahoe {

// ------------------------------------------------------------------------------------------------
// (go_right, the branch rule, lives in forest_internal.h)
template <bool NANM = false>
__device__ __forceinline__ uint32_t step(uint32_t idx, float thr, uint32_t meta, float x, float missing)
{
    return 2u * idx + 1u + go_right_meta<NANM>(x, thr, meta, missing);
}

// ------------------------------------------------------------------------------------------------
// DIRECT: lane = row; nodes and features come straight from global memory.  Works for any shape.
// Analogue of infer_adaptive_reorg_* (Struct.h:1196-1240).
// MC (multi-class handle, trees class-major): the sum is stored to sums[row * num_classes + c] at the end of class c's
// trees and restarts from 0.0f; leaf indices go to the original tree's column.
// STAGED (tahoe_forest_predict_staged): `sums` is out[rows][S][num_classes] and stages[0..S) the strictly ascending counts of
// trees per class after which the running sum is stored -- to sums[(row * S + si) * num_classes + cls], without resetting it
// -- by a stage cursor si that goes back to 0 at a class end; the final per-class / per-row store is not done.
// NANM (TAHOE_CREATE_NAN_MISSING): the branch rule counts a NaN as missing (is_missing_value<true>).  A template flag, here and
// in rowtile_kernel, so that the instantiations without it stay the code they were.
template <bool WRITE_LEAF, bool MC = false, bool STAGED = false, bool NANM = false>
__global__ void __launch_bounds__(kBlock) direct_kernel(const InnerNode *__restrict__ inner,
                                                        const float *__restrict__ leaf_val,
                                                        const uint32_t *__restrict__ leaf_orig,
                                                        const float *__restrict__ data, float *sums,
                                                        uint32_t *__restrict__ leaf_out, const float *sums_in, size_t rows, int cols,
                                                        int num_trees, int depth, float missing, int num_classes,
                                                        const int32_t *__restrict__ stages, int S)
{
    static_assert(!STAGED || !WRITE_LEAF, "no staged leaf indices");
    const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    const float *x = data + row * (size_t)cols;
    const size_t n_inner = ((size_t)1 << depth) - 1;
    const size_t n_leaf = (size_t)1 << depth;
    float sum = sums_in ? sums_in[row] : 0.0f;  // continues a running sum (tree shards chained in order)
    const int ctrees = MC ? num_trees / num_classes : 0;
    int cls = 0, cend = ctrees;  // MC: class of tree t and the end of its trees
    int si = 0, cbeg = 0, send = STAGED ? stages[0] : 0;  // STAGED: the cursor, the class's first tree, the tree after the stage's last
    for (int t = 0; t < num_trees; ++t) {
        const InnerNode *tree = inner + (size_t)t * n_inner;
        uint32_t idx = 0;
        for (int l = 0; l < depth; ++l) {
            const InnerNode n = tree[idx];
            idx = step<NANM>(idx, n.thr, n.meta, x[n.meta & kMetaFidMask], missing);
        }
        const size_t b = (size_t)t * n_leaf + (idx - (uint32_t)n_inner);
        sum += leaf_val[b];
        if (WRITE_LEAF) leaf_out[MC ? row * (size_t)num_trees + (t - cls * ctrees) * num_classes + cls : row * (size_t)num_trees + t] = leaf_orig[b];
        if constexpr (STAGED) {
            if (t + 1 == send) {
                sums[(row * (size_t)S + si) * (size_t)(MC ? num_classes : 1) + cls] = sum;
                ++si;
                send = si < S ? cbeg + stages[si] : -1;
            }
        }
        if (MC && t + 1 == cend) {
            if (!STAGED && sums) sums[row * (size_t)num_classes + cls] = sum;
            sum = 0.0f;
            ++cls;
            cend += ctrees;
            if constexpr (STAGED) {
                si = 0;
                cbeg = t + 1;
                send = cbeg + stages[0];
            }
        }
    }
    if (!MC && !STAGED && sums) sums[row] = sum;
}

// ------------------------------------------------------------------------------------------------
// ROWTILE: one workgroup owns 64 rows, kept feature-major in LDS (tile[fid][row]) so that lane = row
// reads hit 32 distinct banks for any per-lane fid.  The four waves split the trees round-robin
// (wave w walks trees w, w+4, ...); each wave stages the top `lds_levels` levels of its current
// tree in a private LDS slot (prefetched into registers during the previous walk) and reads deeper
// levels from global memory.  Leaf values are exchanged through LDS once per round of four trees and
// added by the row's owner lane in tree order.  Any num_cols whose 64-row tile fits LDS.
//
// Dynamic LDS: [cols][64] float | kWaves slots of slot_nodes InnerNode | [2][kWaves][64] float.
// MC: the owner lane stores its sum at the end of every class (direct_kernel).
// CSR: the tile is staged from csr by csr_stage_tile (forest_internal.h) and `data` is not read.
// STAGED: direct_kernel's stage cursor, kept by the owner lanes; a stage can end at any of a round's four trees.
// COLS: the tile is staged from column-major buffers by cols_stage_tile (forest_internal.h) and `data` is not read.
template <bool WRITE_LEAF, bool MC = false, bool CSR = false, bool STAGED = false, bool COLS = false, bool NANM = false>
__global__ void __launch_bounds__(kBlock) rowtile_kernel(const InnerNode *__restrict__ inner,
                                                         const float *__restrict__ leaf_val,
                                                         const uint32_t *__restrict__ leaf_orig,
                                                         const float *__restrict__ data, float *sums,
                                                         uint32_t *__restrict__ leaf_out, const float *sums_in, size_t rows, int cols,
                                                         int num_trees, int depth, int lds_levels, float missing,
                                                         int vec4_ok, int num_classes, CsrView csr,
                                                         const int32_t *__restrict__ stages, int S, ColsView cv)
{
    static_assert(!STAGED || (!WRITE_LEAF && !CSR), "staged output: predictions from dense rows");
    static_assert(!COLS || (!CSR && !WRITE_LEAF && !STAGED), "column-major rows: predictions only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int slot_nodes = (1 << lds_levels) - 1;            // nodes of the staged top
    const int slot_stride = (slot_nodes + 1) & ~1;           // keep 16-byte alignment of each slot
    float *tile = reinterpret_cast<float *>(smem);
    InnerNode *slots = reinterpret_cast<InnerNode *>(smem + (size_t)cols * kTileRows * sizeof(float));
    float *vals = reinterpret_cast<float *>(slots + (size_t)kWaves * slot_stride);
    InnerNode *slot = slots + (size_t)wave * slot_stride;

    const size_t row0 = (size_t)blockIdx.x * kTileRows;
    const size_t row = row0 + lane;
    const bool row_ok = row < rows;

    // ---- stage the row tile, transposed to feature-major ----
    if constexpr (CSR) {
        csr_stage_tile<kBlock>(tile, reinterpret_cast<int64_t *>(vals), cols, row0, rows, csr, missing, threadIdx.x);
    } else if constexpr (COLS) {
        cols_stage_tile<kWaves>(tile, cols, row0, rows, cv, wave, lane);
    } else {
        const float *src = data + (row_ok ? row : row0) * (size_t)cols;
        if (vec4_ok) {
            const float4 *src4 = reinterpret_cast<const float4 *>(src);
            for (int f4 = wave; f4 < cols / 4; f4 += kWaves) {
                float4 v = row_ok ? src4[f4] : make_float4(0.f, 0.f, 0.f, 0.f);
                tile[(4 * f4 + 0) * kTileRows + lane] = v.x;
                tile[(4 * f4 + 1) * kTileRows + lane] = v.y;
                tile[(4 * f4 + 2) * kTileRows + lane] = v.z;
                tile[(4 * f4 + 3) * kTileRows + lane] = v.w;
            }
        } else {
            for (int f = wave; f < cols; f += kWaves) tile[f * kTileRows + lane] = row_ok ? src[f] : 0.0f;
        }
    }

    const size_t n_inner = ((size_t)1 << depth) - 1;
    const size_t n_leaf = (size_t)1 << depth;
    // Each lane carries up to ceil(slot_nodes / 64) records of the next tree's top in registers.
    constexpr int kMaxPref = ((1 << kMaxLdsLevels) + 63) / 64;  // 4
    uint2 pref[kMaxPref];
    auto prefetch_top = [&](int t) {
        const uint2 *g = reinterpret_cast<const uint2 *>(inner + (size_t)t * n_inner);
#pragma unroll
        for (int k = 0; k < kMaxPref; ++k) {
            const int i = k * 64 + lane;
            pref[k] = (i < slot_nodes) ? g[i] : make_uint2(0u, 0u);
        }
    };
    auto commit_top = [&]() {
        uint2 *s = reinterpret_cast<uint2 *>(slot);
#pragma unroll
        for (int k = 0; k < kMaxPref; ++k) {
            const int i = k * 64 + lane;
            if (i < slot_nodes) s[i] = pref[k];
        }
    };
    if (wave < num_trees) {
        prefetch_top(wave);
        commit_top();
    }
    __syncthreads();  // tile and every wave's first slot are in LDS

    float sum = 0.0f;  // meaningful in lanes 0..15: row 16*wave + lane of the tile
    if (sums_in && lane < 16 && row0 + 16 * wave + lane < rows) sum = sums_in[row0 + 16 * wave + lane];
    const int ctrees = MC ? num_trees / num_classes : 0;
    int cls = 0, cend = ctrees;  // MC: class being summed and the end of its trees
    int si = 0, cbeg = 0, send = STAGED ? stages[0] : 0;  // STAGED: the cursor, the class's first tree, the tree after the stage's last
    const int rounds = (num_trees + kWaves - 1) / kWaves;
    for (int r = 0; r < rounds; ++r) {
        const int t = r * kWaves + wave;
        float v = 0.0f;
        if (t < num_trees) {
            const bool more = t + kWaves < num_trees;
            if (more) prefetch_top(t + kWaves);
            uint32_t idx = 0;
            for (int l = 0; l < lds_levels; ++l) {
                const InnerNode n = slot[idx];
                const float x = tile[(n.meta & kMetaFidMask) * kTileRows + lane];
                idx = step<NANM>(idx, n.thr, n.meta, x, missing);
            }
            const InnerNode *tree = inner + (size_t)t * n_inner;
            for (int l = lds_levels; l < depth; ++l) {
                const InnerNode n = tree[idx];
                const float x = tile[(n.meta & kMetaFidMask) * kTileRows + lane];
                idx = step<NANM>(idx, n.thr, n.meta, x, missing);
            }
            const size_t b = (size_t)t * n_leaf + (idx - (uint32_t)n_inner);
            v = leaf_val[b];
            if (WRITE_LEAF) {
                if (row_ok)
                    leaf_out[MC ? row * (size_t)num_trees + mc_orig_tree(t, num_classes, num_trees / num_classes) : row * (size_t)num_trees + t] = leaf_orig[b];
            }
            if (more) commit_top();  // this wave's reads of the slot are done (in-order LDS)
        }
        float *vb = vals + (size_t)(r & 1) * kWaves * kTileRows;
        vb[wave * kTileRows + lane] = v;
        __syncthreads();
        if (lane < 16) {
            const int rr = 16 * wave + lane;
            const int nt = min(kWaves, num_trees - r * kWaves);
            if constexpr (STAGED) {
                const size_t orow = row0 + rr;
                for (int j = 0; j < nt; ++j) {
                    sum += vb[j * kTileRows + rr];  // tree order
                    const int done = r * kWaves + j + 1;
                    if (done == send) {
                        if (orow < rows) sums[(orow * (size_t)S + si) * (size_t)(MC ? num_classes : 1) + cls] = sum;
                        ++si;
                        send = si < S ? cbeg + stages[si] : -1;
                    }
                    if (MC && done == cend) {
                        sum = 0.0f;
                        ++cls;
                        cend += ctrees;
                        si = 0;
                        cbeg = done;
                        send = cbeg + stages[0];
                    }
                }
            } else if (MC) {
                const size_t orow = row0 + rr;
                for (int j = 0; j < nt; ++j) {
                    sum += vb[j * kTileRows + rr];  // tree order
                    if (r * kWaves + j + 1 == cend) {
                        if (sums && orow < rows) sums[orow * (size_t)num_classes + cls] = sum;
                        sum = 0.0f;
                        ++cls;
                        cend += ctrees;
                    }
                }
            } else {
                for (int j = 0; j < nt; ++j) sum += vb[j * kTileRows + rr];  // tree order
            }
        }
    }
    if (!MC && !STAGED && sums && lane < 16) {
        const size_t orow = row0 + 16 * wave + lane;
        if (orow < rows) sums[orow] = sum;
    }
}

// ------------------------------------------------------------------------------------------------
// TILEBLOCK: the K3-shaped strategy (num_cols <= 512).
//   * ROWS (128 or 64) rows of the batch live feature-major in LDS for the whole kernel.
//   * kSlots = 4 trees are in flight; slot s is walked by ROWS/64 waves (one per 64-row group).
//     A slot holds the tree's top `top_levels` levels as SoA (thr float | meta uint16): one
//     ds_read_b32 + one ds_read_u16 per visit, feature read conflict-free by layout.
//   * Levels below the LDS top and above the last two come from the heap records in global memory
//     (only when De > 12); the last two levels and the leaves come from one 32-byte block.
//   * The next round's tops are prefetched into registers while the current trees are walked and
//     committed to LDS between the two barriers of a round; leaf values cross LDS once per round
//     and are added by the row's owner lane in tree order (bit-exact float32 sums).
// Dynamic LDS: [cols][ROWS] float | kSlots x top_stride bytes | [2][kSlots][ROWS] float.
template <int ROWS, bool WRITE_LEAF>
__global__ void __launch_bounds__(kSlots *ROWS)
    tileblock_kernel(const unsigned char *__restrict__ top, const uint4 *__restrict__ blocks,
                     const InnerNode *__restrict__ inner, const uint32_t *__restrict__ leaf_orig,
                     const float *__restrict__ data, float *sums, uint32_t *__restrict__ leaf_out,
                     const float *sums_in, size_t rows, int cols, int num_trees, int depth, int top_levels, int top_stride, float missing,
                     int vec4_ok)
{
    constexpr int RG = ROWS / 64;            // waves per slot (row groups)
    constexpr int NT = kSlots * ROWS;        // threads
    constexpr int NW = NT / 64;              // waves
    constexpr int OWN = ROWS / NW;           // rows each wave accumulates (16)
    constexpr int kChunksMax = (4096 + 2048) / 16;
    constexpr int PF = (kChunksMax + ROWS - 1) / ROWS;  // 16-byte chunks a lane prefetches (3 or 6)

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: wave-uniform branches below
    const int slot_id = wave / RG;
    const int rgrp = wave % RG;
    const int rloc = rgrp * 64 + lane;       // row within the tile
    const int sl = rgrp * 64 + lane;         // lane index within the slot's group of RG waves

    float *tile = reinterpret_cast<float *>(smem);
    unsigned char *slots = smem + (size_t)cols * ROWS * sizeof(float);
    float *vals = reinterpret_cast<float *>(slots + (size_t)kSlots * top_stride);
    unsigned char *slot = slots + (size_t)slot_id * top_stride;
    // slot = thr[2^L] float | meta[2^L] uint16, both indexed by 1-based heap position (entry 0 unused)
    const float *s_thr = reinterpret_cast<const float *>(slot);
    const uint16_t *s_meta = reinterpret_cast<const uint16_t *>(slot + (((4 << top_levels) + 15) & ~15));
    const int n_chunks = top_stride >> 4;

    const size_t row0 = (size_t)blockIdx.x * ROWS;
    const size_t row = row0 + rloc;
    const bool row_ok = row < rows;

    // ---- stage the row tile, transposed to feature-major (conflict-free: bank = row % 32) ----
    {
        const int trow = tid % ROWS, tpart = tid / ROWS;  // kSlots parts stride over the features
        const size_t grow = row0 + trow;
        const bool ok = grow < rows;
        const float *src = data + (ok ? grow : row0) * (size_t)cols;
        if (vec4_ok) {
            const float4 *src4 = reinterpret_cast<const float4 *>(src);
            for (int f4 = tpart; f4 < cols / 4; f4 += kSlots) {
                const float4 v = ok ? src4[f4] : make_float4(0.f, 0.f, 0.f, 0.f);
                tile[(4 * f4 + 0) * ROWS + trow] = v.x;
                tile[(4 * f4 + 1) * ROWS + trow] = v.y;
                tile[(4 * f4 + 2) * ROWS + trow] = v.z;
                tile[(4 * f4 + 3) * ROWS + trow] = v.w;
            }
        } else {
            for (int f = tpart; f < cols; f += kSlots) tile[f * ROWS + trow] = ok ? src[f] : 0.0f;
        }
    }

    // Next round's top: PF 16-byte chunks per lane, held in registers while the current tree is walked.
    // Named registers (not an array): an indexed array ends up in scratch memory.
    uint4 pf0 = {}, pf1 = {}, pf2 = {}, pf3 = {}, pf4 = {}, pf5 = {};
    static_assert(PF == 3 || PF == 6, "prefetch registers are written out for 3 or 6 chunks per lane");
    auto prefetch_top = [&](int t) {
        const uint4 *g = reinterpret_cast<const uint4 *>(top + (size_t)t * top_stride);
        const int last = n_chunks - 1;  // clamped: branch-free and in bounds
        pf0 = g[min(0 * ROWS + sl, last)];
        pf1 = g[min(1 * ROWS + sl, last)];
        pf2 = g[min(2 * ROWS + sl, last)];
        if constexpr (PF == 6) {
            pf3 = g[min(3 * ROWS + sl, last)];
            pf4 = g[min(4 * ROWS + sl, last)];
            pf5 = g[min(5 * ROWS + sl, last)];
        }
    };
    auto commit_top = [&]() {
        uint4 *s = reinterpret_cast<uint4 *>(slot);
        if (0 * ROWS + sl < n_chunks) s[0 * ROWS + sl] = pf0;
        if (1 * ROWS + sl < n_chunks) s[1 * ROWS + sl] = pf1;
        if (2 * ROWS + sl < n_chunks) s[2 * ROWS + sl] = pf2;
        if constexpr (PF == 6) {
            if (3 * ROWS + sl < n_chunks) s[3 * ROWS + sl] = pf3;
            if (4 * ROWS + sl < n_chunks) s[4 * ROWS + sl] = pf4;
            if (5 * ROWS + sl < n_chunks) s[5 * ROWS + sl] = pf5;
        }
    };
    if (slot_id < num_trees) {
        prefetch_top(slot_id);
        commit_top();
    }
    __syncthreads();

    const size_t n_inner = ((size_t)1 << depth) - 1;
    const uint32_t n_blocks = 1u << (depth - 2);
    const uint32_t first_block_node = n_blocks - 1;  // heap index of the first node of level depth-2
    float sum = 0.0f;                                // lanes 0..OWN-1: row OWN*wave + lane of the tile
    if (sums_in && lane < OWN && row0 + OWN * wave + lane < rows) sum = sums_in[row0 + OWN * wave + lane];
    const int rounds = (num_trees + kSlots - 1) / kSlots;
    for (int r = 0; r < rounds; ++r) {
        const int t = r * kSlots + slot_id;
        const bool more = t + kSlots < num_trees;
        float v = 0.0f;
        if (t < num_trees) {
            if (more) prefetch_top(t + kSlots);
            // Top levels from LDS, 1-based heap positions: the children of position i are the aligned
            // pair (2i, 2i+1), read together with the current node's feature -> one LDS round trip
            // per level.
            uint32_t i = 1;
            if (top_levels > 0) {
                float thr = s_thr[1];
                uint32_t m = s_meta[1];
                for (int l = 0; l < top_levels - 1; ++l) {
                    const float x = tile[(m & 0x7fffu) * ROWS + rloc];
                    const float2 t2 = *reinterpret_cast<const float2 *>(&s_thr[2 * i]);
                    const uint32_t m2 = *reinterpret_cast<const uint32_t *>(&s_meta[2 * i]);
                    const uint32_t c = go_right(x, thr, (m >> 15) != 0, missing);
                    i = 2u * i + c;
                    thr = c ? t2.y : t2.x;
                    m = c ? (m2 >> 16) : (m2 & 0xffffu);
                }
                const float x = tile[(m & 0x7fffu) * ROWS + rloc];
                i = 2u * i + go_right(x, thr, (m >> 15) != 0, missing);
            }
            uint32_t idx = i - 1;  // 0-based heap index on level top_levels
            if (top_levels < depth - 2) {  // deep trees only (De > 12): heap records from global memory
                const InnerNode *tree = inner + (size_t)t * n_inner;
                for (int l = top_levels; l < depth - 2; ++l) {
                    const InnerNode n = tree[idx];
                    const float x = tile[(n.meta & kMetaFidMask) * ROWS + rloc];
                    idx = step(idx, n.thr, n.meta, x, missing);
                }
            }
            const uint32_t b = idx - first_block_node;
            const uint4 *bp = blocks + ((size_t)t * n_blocks + b) * 2;
            const uint4 na = bp[0];  // thr0, thr1, thr2, packed metas
            const uint4 nb = bp[1];  // four leaf values
            // Both 16-byte loads are issued here, whole: without the pins the compiler sinks single
            // dwords of them into the branches of go_right and pays a second global round trip.
            asm volatile("" ::"v"(na.x), "v"(na.y), "v"(na.z), "v"(na.w));
            asm volatile("" ::"v"(nb.x), "v"(nb.y), "v"(nb.z), "v"(nb.w));
            const uint32_t m = na.w;
            const float x0 = tile[(m & 0x1ffu) * ROWS + rloc];
            const float x1 = tile[((m >> 10) & 0x1ffu) * ROWS + rloc];
            const float x2 = tile[((m >> 20) & 0x1ffu) * ROWS + rloc];
            const uint32_t c0 = go_right(x0, __uint_as_float(na.x), ((m >> 9) & 1u) != 0, missing);
            const uint32_t c1l = go_right(x1, __uint_as_float(na.y), ((m >> 19) & 1u) != 0, missing);
            const uint32_t c1r = go_right(x2, __uint_as_float(na.z), ((m >> 29) & 1u) != 0, missing);
            const uint32_t c1 = c0 ? c1r : c1l;
            const uint32_t lo = c1 ? nb.y : nb.x, hi = c1 ? nb.w : nb.z;
            v = __uint_as_float(c0 ? hi : lo);
            if (WRITE_LEAF) {
                if (row_ok)
                    leaf_out[row * (size_t)num_trees + t] =
                        leaf_orig[(size_t)t * ((size_t)n_blocks * 4) + (size_t)b * 4 + 2 * c0 + c1];
            }
        }
        float *vb = vals + (size_t)(r & 1) * kSlots * ROWS;
        vb[slot_id * ROWS + rloc] = v;
        __syncthreads();  // (A) every walk of this round has finished reading its slot
        if (t < num_trees && more) commit_top();
        if (lane < OWN) {
            const int rr = OWN * wave + lane;
            const int nt = min(kSlots, num_trees - r * kSlots);
            for (int j = 0; j < nt; ++j) sum += vb[j * ROWS + rr];  // tree order
        }
        __syncthreads();  // (B) the next round's tops are in LDS
    }
    if (sums && lane < OWN) {
        const size_t orow = row0 + OWN * wave + lane;
        if (orow < rows) sums[orow] = sum;
    }
}

// ------------------------------------------------------------------------------------------------
// TILERING: TILEBLOCK's data path with the waves decoupled.  No workgroup barrier inside the tree loop.
//   * NWALK walker waves, each with a private LDS slot for the top of its current tree; walker w walks
//     trees w, w+NWALK, ... for all ROWS rows of the tile (K = ROWS/64 interleaved chains per lane), and
//     prefetches the next top into registers meanwhile.  Waves drift freely, so one wave's global
//     gather latency is covered by the others' LDS walks.
//   * One consumer wave adds the leaf values in tree order (bit-exact float32 sums), handed over through the LDS tree ring
//     (forest_internal.h; DESIGN.md, "The LDS tree ring").
// Dynamic LDS: [cols][ROWS] float | NWALK x top_stride | ring.

template <int ROWS>
struct RingGeom {
    static constexpr int RING = (ROWS == 64) ? 32 : 8;   // ring entries (trees)
    static constexpr int BATCH = (ROWS == 64) ? 8 : 4;   // trees the consumer takes per poll
};

template <int ROWS, int NWALK, bool WRITE_LEAF>
__global__ void __launch_bounds__((NWALK + 1) * 64)
    tilering_kernel(const unsigned char *__restrict__ top, const uint4 *__restrict__ blocks,
                    const InnerNode *__restrict__ inner, const uint32_t *__restrict__ leaf_orig,
                    const float *__restrict__ data, float *sums, uint32_t *__restrict__ leaf_out,
                    const float *sums_in, size_t rows, int cols, int num_trees, int depth, int top_levels, int top_stride, float missing,
                    int vec4_ok, int *__restrict__ error_flag)
{
    constexpr int K = ROWS / 64;
    constexpr int NT = (NWALK + 1) * 64;
    constexpr int RING = RingGeom<ROWS>::RING;
    constexpr int BATCH = RingGeom<ROWS>::BATCH;
    static_assert(BATCH <= RING && BATCH <= 64, "consumer batch must fit the ring");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    float *tile = reinterpret_cast<float *>(smem);
    unsigned char *slots = smem + (size_t)cols * ROWS * sizeof(float);
    const LdsRing<RING, ROWS> ring(slots + (size_t)NWALK * top_stride);

    const size_t row0 = (size_t)blockIdx.x * ROWS;

    // ---- stage the row tile, transposed to feature-major; reset the ring ----
    if (vec4_ok) {
        const int n4 = cols / 4;
        for (int e = tid; e < ROWS * n4; e += NT) {
            const int trow = e % ROWS, f4 = e / ROWS;
            const size_t grow = row0 + trow;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (grow < rows) v = reinterpret_cast<const float4 *>(data + grow * (size_t)cols)[f4];
            tile[(4 * f4 + 0) * ROWS + trow] = v.x;
            tile[(4 * f4 + 1) * ROWS + trow] = v.y;
            tile[(4 * f4 + 2) * ROWS + trow] = v.z;
            tile[(4 * f4 + 3) * ROWS + trow] = v.w;
        }
    } else {
        for (int e = tid; e < ROWS * cols; e += NT) {
            const int trow = e % ROWS, f = e / ROWS;
            const size_t grow = row0 + trow;
            tile[f * ROWS + trow] = grow < rows ? data[grow * (size_t)cols + f] : 0.0f;
        }
    }
    TAHOE_RING_RESET(ring, RING, tid);

    if (wave == NWALK) {
        // ================= consumer: ordered accumulation =================
        __syncthreads();
        float sum[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const size_t irow = row0 + k * 64 + lane;
            sum[k] = (sums_in && irow < rows) ? sums_in[irow] : 0.0f;
        }
        bool dead = false;
        for (int t0 = 0; t0 < num_trees && !dead; t0 += BATCH) {
            const int nb = min(BATCH, num_trees - t0);
            TAHOE_RING_WAIT_READY(ring, RING, t0, nb, lane, 2, dead);
            if (dead) break;
            TAHOE_LDS_ACQUIRE();  // the values are read after the flags
            for (int j = 0; j < nb; ++j) {
                const int e = (t0 + j) % RING;
#pragma unroll
                for (int k = 0; k < K; ++k) sum[k] += ring.vals[e * ROWS + k * 64 + lane];  // tree order
            }
            ring.release(t0 + nb, lane);
        }
        ring_dead(dead, lane, error_flag);
        if (sums) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const size_t orow = row0 + k * 64 + lane;
                if (orow < rows) sums[orow] = sum[k];
            }
        }
        return;
    }

    // ================= walkers =================
    unsigned char *slot = slots + (size_t)wave * top_stride;
    const float *s_thr = reinterpret_cast<const float *>(slot);
    const uint16_t *s_meta = reinterpret_cast<const uint16_t *>(slot + (((4 << top_levels) + 15) & ~15));
    const int n_chunks = top_stride >> 4;

    // Next tree's top: six 16-byte chunks per lane (6 KiB per slot), named registers (an indexed array
    // would live in scratch memory).
    uint4 pf0 = {}, pf1 = {}, pf2 = {}, pf3 = {}, pf4 = {}, pf5 = {};
    auto prefetch_top = [&](int t) {
        const uint4 *g = reinterpret_cast<const uint4 *>(top + (size_t)t * top_stride);
        const int last = n_chunks - 1;  // clamped: branch-free and in bounds
        pf0 = g[min(0 * 64 + lane, last)];
        pf1 = g[min(1 * 64 + lane, last)];
        pf2 = g[min(2 * 64 + lane, last)];
        pf3 = g[min(3 * 64 + lane, last)];
        pf4 = g[min(4 * 64 + lane, last)];
        pf5 = g[min(5 * 64 + lane, last)];
    };
    auto commit_top = [&]() {
        uint4 *s = reinterpret_cast<uint4 *>(slot);
        if (0 * 64 + lane < n_chunks) s[0 * 64 + lane] = pf0;
        if (1 * 64 + lane < n_chunks) s[1 * 64 + lane] = pf1;
        if (2 * 64 + lane < n_chunks) s[2 * 64 + lane] = pf2;
        if (3 * 64 + lane < n_chunks) s[3 * 64 + lane] = pf3;
        if (4 * 64 + lane < n_chunks) s[4 * 64 + lane] = pf4;
        if (5 * 64 + lane < n_chunks) s[5 * 64 + lane] = pf5;
    };
    if (wave < num_trees) {
        prefetch_top(wave);
        commit_top();
    }
    __syncthreads();  // the tile, the ring state and (own wave) the first top are in LDS

    const size_t n_inner = ((size_t)1 << depth) - 1;
    const uint32_t n_blocks = 1u << (depth - 2);
    const uint32_t first_block_node = n_blocks - 1;
    bool dead = false;
    for (int t = wave; t < num_trees && !dead; t += NWALK) {
        const bool more = t + NWALK < num_trees;
        if (more) prefetch_top(t + NWALK);
        // K interleaved chains: chain k walks row k*64 + lane.  1-based heap positions; the children
        // of position i are the aligned pair (2i, 2i+1), read together with the node's feature.
        uint32_t i[K];
#pragma unroll
        for (int k = 0; k < K; ++k) i[k] = 1;
        if (top_levels > 0) {
            float thr[K];
            uint32_t m[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                thr[k] = s_thr[1];
                m[k] = s_meta[1];
            }
            for (int l = 0; l < top_levels - 1; ++l) {
                float x[K];
                float2 t2[K];
                uint32_t m2[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    x[k] = tile[(m[k] & 0x7fffu) * ROWS + k * 64 + lane];
                    t2[k] = *reinterpret_cast<const float2 *>(&s_thr[2 * i[k]]);
                    m2[k] = *reinterpret_cast<const uint32_t *>(&s_meta[2 * i[k]]);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const uint32_t c = go_right(x[k], thr[k], (m[k] >> 15) != 0, missing);
                    i[k] = 2u * i[k] + c;
                    thr[k] = c ? t2[k].y : t2[k].x;
                    m[k] = c ? (m2[k] >> 16) : (m2[k] & 0xffffu);
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float x = tile[(m[k] & 0x7fffu) * ROWS + k * 64 + lane];
                i[k] = 2u * i[k] + go_right(x, thr[k], (m[k] >> 15) != 0, missing);
            }
        }
        float v[K];
        uint32_t bsel[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint32_t idx = i[k] - 1;  // 0-based heap index on level top_levels
            if (top_levels < depth - 2) {  // deep trees only (De > 12): heap records from global memory
                const InnerNode *tree = inner + (size_t)t * n_inner;
                for (int l = top_levels; l < depth - 2; ++l) {
                    const InnerNode n = tree[idx];
                    const float x = tile[(n.meta & kMetaFidMask) * ROWS + k * 64 + lane];
                    idx = step(idx, n.thr, n.meta, x, missing);
                }
            }
            bsel[k] = idx - first_block_node;
        }
        uint4 na[K], nb[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint4 *bp = blocks + ((size_t)t * n_blocks + bsel[k]) * 2;
            na[k] = bp[0];  // thr0, thr1, thr2, packed metas
            nb[k] = bp[1];  // four leaf values
            // whole 16-byte loads, issued here (the compiler otherwise sinks single dwords into branches)
            asm volatile("" ::"v"(na[k].x), "v"(na[k].y), "v"(na[k].z), "v"(na[k].w));
            asm volatile("" ::"v"(nb[k].x), "v"(nb[k].y), "v"(nb[k].z), "v"(nb[k].w));
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t m = na[k].w;
            const float x0 = tile[(m & 0x1ffu) * ROWS + k * 64 + lane];
            const float x1 = tile[((m >> 10) & 0x1ffu) * ROWS + k * 64 + lane];
            const float x2 = tile[((m >> 20) & 0x1ffu) * ROWS + k * 64 + lane];
            const uint32_t c0 = go_right(x0, __uint_as_float(na[k].x), ((m >> 9) & 1u) != 0, missing);
            const uint32_t c1l = go_right(x1, __uint_as_float(na[k].y), ((m >> 19) & 1u) != 0, missing);
            const uint32_t c1r = go_right(x2, __uint_as_float(na[k].z), ((m >> 29) & 1u) != 0, missing);
            const uint32_t c1 = c0 ? c1r : c1l;
            const uint32_t lo = c1 ? nb[k].y : nb[k].x, hi = c1 ? nb[k].w : nb[k].z;
            v[k] = __uint_as_float(c0 ? hi : lo);
            if (WRITE_LEAF) {
                const size_t row = row0 + k * 64 + lane;
                if (row < rows)
                    leaf_out[row * (size_t)num_trees + t] =
                        leaf_orig[(size_t)t * ((size_t)n_blocks * 4) + (size_t)bsel[k] * 4 + 2 * c0 + c1];
            }
        }
        // ---- hand the leaf values to the consumer ----
        TAHOE_RING_WAIT_FREE(ring, RING, t, 2, dead);
        const int e = t % RING;
#pragma unroll
        for (int k = 0; k < K; ++k) ring.vals[e * ROWS + k * 64 + lane] = v[k];
        TAHOE_RING_PUBLISH(ring, RING, t, lane == 0);
        if (more) commit_top();  // this wave's reads of its slot are done (in-order LDS)
    }
    ring_dead(dead, lane, error_flag);
}

// transform_k (Struct.h:196-209) with the CPU predictor's arithmetic (BaseTahoeTest.h:467-472):
// AVG divides by num_trees (the reference's GPU epilogue multiplies by 1/T instead).
// sigmoid: 1 / (1 + expf(-r)), except where expf(-r) overflows (r < -88.72): 1 / inf would flush the subnormal tail (down to
// r = -103.97) to 0; there 1 + e^-r has long rounded to e^-r, so the value is expf(r).
__device__ __forceinline__ float sigmoid_value(float r)
{
    const float e = expf(-r);
    return e == INFINITY ? expf(r) : 1.0f / (1.0f + e);
}

__device__ __forceinline__ float transform_value(float r, int output, int num_trees, float threshold, float global_bias)
{
    if ((output & TAHOE_OUT_AVG) != 0) r = r / (float)num_trees;
    r += global_bias;
    if ((output & TAHOE_OUT_SIGMOID) != 0) r = sigmoid_value(r);
    if ((output & TAHOE_OUT_THRESHOLD) != 0) r = r > threshold ? 1.0f : 0.0f;
    return r;
}

__global__ void transform_kernel(float *preds, size_t n, int output, int num_trees, float threshold,
                                 float global_bias)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    preds[i] = transform_value(preds[i], output, num_trees, threshold, global_bias);
}

// Epilogue of a multi-class handle, one thread per row of preds[rows][num_classes]: per element AVG (by the trees of a
// class), bias and sigmoid with transform_kernel's arithmetic, then the row-wise softmax m = max z, e = expf(z - m),
// p = e / sum(e) with the sum taken in class order.
__global__ void transform_mc_kernel(float *preds, size_t rows, int num_classes, int output, int class_trees, float global_bias)
{
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    float *p = preds + row * (size_t)num_classes;
    float m = -INFINITY;
    for (int c = 0; c < num_classes; ++c) {
        float r = p[c];
        if ((output & TAHOE_OUT_AVG) != 0) r = r / (float)class_trees;
        r += global_bias;
        if ((output & TAHOE_OUT_SIGMOID) != 0) r = sigmoid_value(r);
        p[c] = r;
        m = fmaxf(m, r);
    }
    if ((output & TAHOE_OUT_SOFTMAX) == 0) return;
    float s = 0.0f;
    for (int c = 0; c < num_classes; ++c) {
        const float e = expf(p[c] - m);
        p[c] = e;
        s += e;
    }
    for (int c = 0; c < num_classes; ++c) p[c] = p[c] / s;
}

// transform_mc_kernel's statements on the classes of one (row, stage).  That kernel keeps them written out: routed through
// this function it compiles to other (equivalent) code, and the pre-existing kernels stay as they were, instruction for
// instruction; per element it is transform_value, which both share.
__device__ __forceinline__ void transform_classes(float *p, int num_classes, int output, int class_trees, float global_bias)
{
    float m = -INFINITY;
    for (int c = 0; c < num_classes; ++c) {
        const float r = transform_value(p[c], output & ~TAHOE_OUT_THRESHOLD, class_trees, 0.0f, global_bias);
        p[c] = r;
        m = fmaxf(m, r);
    }
    if ((output & TAHOE_OUT_SOFTMAX) == 0) return;
    float s = 0.0f;
    for (int c = 0; c < num_classes; ++c) {
        const float e = expf(p[c] - m);
        p[c] = e;
        s += e;
    }
    for (int c = 0; c < num_classes; ++c) p[c] = p[c] / s;
}

// Epilogue of tahoe_forest_predict_staged, one thread per (row, stage) of out[rows][S][num_classes]: what transform_kernel
// (num_classes == 1) or transform_mc_kernel does on a handle of the first stages[s] trees of every class, whose AVG divides
// by (float)stages[s]; the softmax runs over the classes of one (row, stage), in class order.
__global__ void transform_staged_kernel(float *out, size_t n, int S, int num_classes, int output, const int32_t *__restrict__ stages,
                                        float threshold, float global_bias)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int stage_trees = stages[i % (size_t)S];
    if (num_classes == 1)
        out[i] = transform_value(out[i], output, stage_trees, threshold, global_bias);
    else
        transform_classes(out + i * (size_t)num_classes, num_classes, output, stage_trees, global_bias);
}

// ------------------------------------------------------------------------------------------------
static int rowtile_lds_bytes(int cols, int lds_levels)
{
    const int slot_nodes = (1 << lds_levels) - 1;
    const int slot_stride = (slot_nodes + 1) & ~1;
    return cols * kTileRows * (int)sizeof(float) + kWaves * slot_stride * (int)sizeof(InnerNode) +
           2 * kWaves * kTileRows * (int)sizeof(float);
}

static bool rowtile_fits(const tahoe_forest *f)
{
    return f->p.num_cols >= 1 && (long long)rowtile_lds_bytes(f->p.num_cols, f->lds_levels) <= f->lds_limit;
}

static long long tileblock_lds_bytes(const tahoe_forest *f, int tile_rows)
{
    return (long long)f->p.num_cols * tile_rows * 4 + (long long)kSlots * top_stride_bytes(f->top_levels) +
           2LL * kSlots * tile_rows * 4;
}

// Rows per TILEBLOCK tile: 128 when it fits LDS, else 64, else 0 (strategy unavailable).
static int tileblock_rows(const tahoe_forest *f)
{
    if (!f->has_blocks || f->p.num_cols < 1) return 0;
    if (const int r = f->knobs.tile_rows)  // TAHOE_TILE_ROWS
        if ((r == 64 || r == 128) && tileblock_lds_bytes(f, r) <= f->lds_limit) return r;
    if (tileblock_lds_bytes(f, 128) <= f->lds_limit) return 128;
    if (tileblock_lds_bytes(f, 64) <= f->lds_limit) return 64;
    return 0;
}

static long long tilering_lds_bytes(const tahoe_forest *f, int tile_rows)
{
    const int nwalk = tile_rows == 64 ? 8 : 4;
    const int ring = tile_rows == 64 ? RingGeom<64>::RING : RingGeom<128>::RING;
    return (long long)f->p.num_cols * tile_rows * 4 + (long long)nwalk * top_stride_bytes(f->top_levels) +
           RingLayout{ring, tile_rows}.bytes();
}

// Rows per TILERING tile: 64 (8 walkers x 1 chain) or 128 (4 walkers x 2 chains); 0 = unavailable.
static int tilering_rows(const tahoe_forest *f)
{
    if (!f->has_blocks || f->p.num_cols < 1) return 0;
    if (const int r = f->knobs.tile_rows)  // TAHOE_TILE_ROWS
        if ((r == 64 || r == 128) && tilering_lds_bytes(f, r) <= f->lds_limit) return r;
    if (tilering_lds_bytes(f, 64) <= f->lds_limit) return 64;
    return 0;
}

static int resolve_strategy(const tahoe_forest *f, size_t rows)
{
    if (f->ob) {  // oblivious handle: ROWTILE = one wave per 64-row float32 tile, DIRECT = features from global memory
        if (f->strategy != TAHOE_STRATEGY_AUTO) return f->strategy;
        return oblivious_tile_fits(f) ? TAHOE_STRATEGY_ROWTILE : TAHOE_STRATEGY_DIRECT;
    }
    if (f->vl) {  // vector-leaf handle: the same two forms
        if (f->strategy != TAHOE_STRATEGY_AUTO) return f->strategy;
        return vector_tile_fits(f) ? TAHOE_STRATEGY_ROWTILE : TAHOE_STRATEGY_DIRECT;
    }
    if (f->sp) {  // sparse handle: QRING = quantised 192-row tile + tree tops in LDS, TILEBLOCK = 64-row float32 tile + tree
                  // tops, ROWTILE = tile only, DIRECT = neither
        if (f->strategy == TAHOE_STRATEGY_DIRECT) return TAHOE_STRATEGY_DIRECT;
        if (f->strategy == TAHOE_STRATEGY_ROWTILE) return TAHOE_STRATEGY_ROWTILE;
        // the quantise pass over rows x cols pays when there is walking to do per feature value (the dense rule, with ten
        // levels standing in for the unknown path length) and the batch gives every CU a 128-row tile or so -- below that
        // the float32 kernel's 64-row tiles fill more of the chip (tools/selector_sparse.py, profiles/r02/selector_sparse.json)
        if (sparse_q_available(f) &&
            (f->strategy == TAHOE_STRATEGY_QRING ||
             (f->strategy == TAHOE_STRATEGY_AUTO && 20LL * f->p.num_trees >= 13LL * f->p.num_cols && rows >= (size_t)64 * (size_t)std::max(f->num_cus, 1))))
            return TAHOE_STRATEGY_QRING;
        if (sparse_top_waves(f) > 0) return TAHOE_STRATEGY_TILEBLOCK;
        return sparse_tile_fits(f) ? TAHOE_STRATEGY_ROWTILE : TAHOE_STRATEGY_DIRECT;
    }
    if (f->strategy != TAHOE_STRATEGY_AUTO) return f->strategy;  // (a multi-class handle refuses the float32 tile forms)
    // QRING pays a quantise pass over rows x cols to make every (row, tree, level) step ~3x cheaper.  Fitted on the
    // enumeration of tools/selector_check.py (profiles/r01/selector_vs_enumeration.json): it loses to ROWTILE on
    // very shallow trees (the whole tree sits in ROWTILE's LDS top, no pre-pass) and to the float32 tile kernels
    // when there is little walking per feature value (trees x depth < 6.5 x cols).  On ten shapes it was not fitted
    // on (--holdout) it picks the fastest strategy on 8 and stays within 1.16x on the other two.
    // (round 4: only while there is little of it -- trees x depth <= 1024.  With 384-row tiles on narrow / few-threshold forests QRING
    // overtook ROWTILE on large shallow forests: 2000 trees x depth 3 x 32 features 0.85 against 0.99 ms, 800 x 4 x 100 0.38 against 0.58,
    // while 100 x 4 x 16 and 30 x 3 x 8 stay with ROWTILE, profiles/r04/selector_*.json)
    const bool shallow = f->depth <= 4 && rowtile_fits(f) && (long long)f->p.num_trees * f->depth <= 1024;
    if (f->num_classes > 1) {  // the same rule over the forms that serve a multi-class handle
        if (shallow) return TAHOE_STRATEGY_ROWTILE;
        if (qring_walkers(f) > 0) return TAHOE_STRATEGY_QRING;
        return rowtile_fits(f) ? TAHOE_STRATEGY_ROWTILE : TAHOE_STRATEGY_DIRECT;
    }
    // (wide rows whose quantised form walks three trees per lane: that form is ~1.25 x faster, the float32 form pays off later)
    const long long per_col = qwide_chains(f) == 3 ? 10 : 13;
    const bool little_work = 2LL * f->p.num_trees * f->depth < per_col * f->p.num_cols &&
                             (tilering_rows(f) > 0 || widef_rows(f) > 0 || tileblock_rows(f) > 0 || rowtile_fits(f));
    if (shallow) return TAHOE_STRATEGY_ROWTILE;
    if (qring_walkers(f) > 0 && !little_work) return TAHOE_STRATEGY_QRING;
    if (tilering_rows(f) > 0 || widef_rows(f) > 0) return TAHOE_STRATEGY_TILERING;
    if (tileblock_rows(f) > 0) return TAHOE_STRATEGY_TILEBLOCK;
    return rowtile_fits(f) ? TAHOE_STRATEGY_ROWTILE : TAHOE_STRATEGY_DIRECT;
}

tahoe_status strategy_available(const tahoe_forest *f, int strategy)
{
    if (f->ob) {
        if (strategy > TAHOE_STRATEGY_ROWTILE || (strategy == TAHOE_STRATEGY_ROWTILE && !oblivious_tile_fits(f)))
            return fail(TAHOE_ERR_UNSUPPORTED, "an oblivious forest runs AUTO, DIRECT or ROWTILE (a 64-row tile of %d columns in %d B "
                                               "of LDS)", f->p.num_cols, f->lds_limit);
        return TAHOE_OK;
    }
    if (f->vl) {
        if (strategy > TAHOE_STRATEGY_ROWTILE || (strategy == TAHOE_STRATEGY_ROWTILE && !vector_tile_fits(f)))
            return fail(TAHOE_ERR_UNSUPPORTED, "a vector-leaf forest runs AUTO, DIRECT or ROWTILE (a 64-row tile of %d columns in %d B "
                                               "of LDS)", f->p.num_cols, f->lds_limit);
        return TAHOE_OK;
    }
    if (f->sp) {
        if (strategy == TAHOE_STRATEGY_QRING && sparse_has_cats(f))
            return fail(TAHOE_ERR_UNSUPPORTED,
                        "QRING does not serve categorical splits: its 4-byte node word (code << 16 | def_left << 15 | fid << 7) "
                        "and its rank quantiser have no room for a category-set test; use AUTO, TILEBLOCK, ROWTILE or DIRECT");
        if ((strategy > TAHOE_STRATEGY_TILEBLOCK && strategy != TAHOE_STRATEGY_QRING) ||
            (strategy == TAHOE_STRATEGY_ROWTILE && !sparse_tile_fits(f)) ||
            (strategy == TAHOE_STRATEGY_TILEBLOCK && sparse_top_waves(f) == 0) ||
            (strategy == TAHOE_STRATEGY_QRING && !sparse_q_available(f)))
            return fail(TAHOE_ERR_UNSUPPORTED,
                        "a sparse forest runs AUTO, DIRECT, ROWTILE (a 64-row tile fits LDS), TILEBLOCK (tile + tree tops in LDS; "
                        "trees of <= 65535 nodes, num_cols <= 32767) or QRING (quantised tile + tree tops; also num_cols <= 256)");
        return TAHOE_OK;
    }
    if (f->nan_missing && (strategy == TAHOE_STRATEGY_TILEBLOCK || strategy == TAHOE_STRATEGY_TILERING))
        return fail(TAHOE_ERR_UNSUPPORTED, "a dense handle created with TAHOE_CREATE_NAN_MISSING runs AUTO, DIRECT, ROWTILE or QRING: "
                                           "the TILEBLOCK and TILERING kernels do not implement that rule");
    if (f->num_classes > 1 && (strategy == TAHOE_STRATEGY_TILEBLOCK || strategy == TAHOE_STRATEGY_TILERING))
        return fail(TAHOE_ERR_UNSUPPORTED, "a multi-class handle runs AUTO, DIRECT, ROWTILE or QRING (no float32 tile forms)");
    if (strategy == TAHOE_STRATEGY_ROWTILE && !rowtile_fits(f))
        return fail(TAHOE_ERR_UNSUPPORTED, "ROWTILE needs %d B of LDS for %d columns; device offers %d",
                    rowtile_lds_bytes(f->p.num_cols, f->lds_levels), f->p.num_cols, f->lds_limit);
    if (strategy == TAHOE_STRATEGY_TILEBLOCK && tileblock_rows(f) == 0)
        return fail(TAHOE_ERR_UNSUPPORTED, "TILEBLOCK needs num_cols <= %d and a 64-row tile that fits %d B of LDS",
                    kBlockMaxCols, f->lds_limit);
    if (strategy == TAHOE_STRATEGY_TILERING && tilering_rows(f) == 0 && widef_rows(f) == 0)
        return fail(TAHOE_ERR_UNSUPPORTED, "TILERING needs a 64-row tile (num_cols <= %d) or an 8-row tile that fits %d B of LDS",
                    kBlockMaxCols, f->lds_limit);
    if (strategy == TAHOE_STRATEGY_QRING && qring_walkers(f) == 0)
        return fail(TAHOE_ERR_UNSUPPORTED,
                    "QRING needs <= 32767 distinct thresholds per feature, num_cols <= 32767 and a 128-row u16 tile in LDS");
    return TAHOE_OK;
}

template <int ROWS>
static void launch_tileblock(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *sums_in, const float *data, size_t rows,
                             hipStream_t stream, int vec4_ok)
{
    const unsigned grid = (unsigned)((rows + ROWS - 1) / ROWS);
    const int lds = (int)tileblock_lds_bytes(f, ROWS);
    const int stride = top_stride_bytes(f->top_levels);
    with_leaf(leaf_out != nullptr, [&](auto wl) {
        hipLaunchKernelGGL((tileblock_kernel<ROWS, decltype(wl)::value>), dim3(grid), dim3(kSlots * ROWS), lds, stream, f->top,
                           f->blocks, f->inner, f->leaf_orig, data, sums, leaf_out, sums_in, rows, f->p.num_cols,
                           f->p.num_trees, f->depth, f->top_levels, stride, f->p.missing, vec4_ok);
    });
}

template <int ROWS, int NWALK>
static void launch_tilering(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *sums_in, const float *data, size_t rows,
                            hipStream_t stream, int vec4_ok)
{
    const unsigned grid = (unsigned)((rows + ROWS - 1) / ROWS);
    const int lds = (int)tilering_lds_bytes(f, ROWS);
    const int stride = top_stride_bytes(f->top_levels);
    with_leaf(leaf_out != nullptr, [&](auto wl) {
        hipLaunchKernelGGL((tilering_kernel<ROWS, NWALK, decltype(wl)::value>), dim3(grid), dim3((NWALK + 1) * 64), lds, stream,
                           f->top, f->blocks, f->inner, f->leaf_orig, data, sums, leaf_out, sums_in, rows, f->p.num_cols,
                           f->p.num_trees, f->depth, f->top_levels, stride, f->p.missing, vec4_ok, f->error_flag);
    });
}

// sums_in (optional, may be `sums` itself): running float32 sums of the trees BEFORE this forest -- every kernel then
// continues that sum in tree order instead of starting from 0.0f (tahoe_forest_predict_accumulate).
// csr (optional): the rows come from there through the fused loader of csr_strategy's tile kernel; `data` is not read.
// cols (optional, never with csr, predictions only): the rows come from column-major buffers and `data` is not read;
// csr_strategy is then what columns_fused_strategy returned -- QRING (the quantise pass reads the columns), ROWTILE, or
// TILEBLOCK on a sparse handle (the tile loader does).
// table (optional, never with csr or cols, predictions only): the rows come from typed, nullable columns through QRING's
// quantise pass; csr_strategy is what table_fused_strategy returned.
static tahoe_status launch_traversal(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data,
                                     size_t rows, hipStream_t stream, const float *sums_in = nullptr, const CsrView *csr = nullptr,
                                     int csr_strategy = 0, const ColsView *cols = nullptr, const TableView *table = nullptr)
{
    if (rows == 0) return TAHOE_OK;
    DeviceGuard on_device(f->device);
    const int strategy = (csr || cols || table) ? csr_strategy : resolve_strategy(f, rows);
    if (table && (csr || cols || leaf_out || sums_in || f->ob || f->vl || strategy != TAHOE_STRATEGY_QRING))
        return fail(TAHOE_ERR_UNSUPPORTED, "launch_traversal: no kernel of strategy %d reads a typed table", strategy);
    if (cols && (csr || leaf_out || sums_in || f->ob || f->vl ||
                 !(strategy == TAHOE_STRATEGY_QRING || strategy == TAHOE_STRATEGY_ROWTILE || (strategy == TAHOE_STRATEGY_TILEBLOCK && f->sp))))
        return fail(TAHOE_ERR_UNSUPPORTED, "launch_traversal: no kernel of strategy %d reads column-major rows", strategy);
    if ((rows + 63) / 64 > 0x7fffffffu) return fail(TAHOE_ERR_INVALID_ARG, "too many rows for one launch: %zu", rows);
    if (const tahoe_status s = strategy_available(f, strategy)) return s;  // (set_strategy has refused it already)
    const bool timed = f->profiling && f->prof_count < f->ev_start.size();
    if (timed) TAHOE_HIP_TRY(hipEventRecord(f->ev_start[f->prof_count], stream));
    bool mid_recorded = false;
    if (timed && !(strategy == TAHOE_STRATEGY_QRING && !f->sp && f->p.num_trees != 0)) {
        // strategies without a separately timed pre-pass: mid = start, so tahoe_forest_prepass_times reads 0 and
        // tahoe_forest_kernel_times the whole launch (a sparse handle's quantise pass counts as part of its walk)
        TAHOE_HIP_TRY(hipEventRecord(f->ev_mid[f->prof_count], stream));
        mid_recorded = true;
    }
    const int vec4_ok = (f->p.num_cols % 4 == 0) && ((reinterpret_cast<uintptr_t>(data) & 15u) == 0);
    if (f->p.num_trees == 0) {
        // Nothing to walk: sums are zero (an empty j-loop in predict_on_cpu).
        if (sums && sums_in && sums != sums_in)
            TAHOE_HIP_TRY(hipMemcpyAsync(sums, sums_in, rows * sizeof(float), hipMemcpyDeviceToDevice, stream));
        else if (sums && !sums_in)
            TAHOE_HIP_TRY(hipMemsetAsync(sums, 0, rows * (size_t)f->num_classes * sizeof(float), stream));
    } else if (f->ob) {
        const tahoe_status os = oblivious_launch(f, sums, leaf_out, data, rows, stream, strategy, sums_in, csr);
        if (os != TAHOE_OK) return os;
    } else if (f->vl) {
        const tahoe_status vs = vector_launch(f, sums, leaf_out, data, rows, stream, strategy, csr);
        if (vs != TAHOE_OK) return vs;
    } else if (f->sp) {
        const tahoe_status ss = sparse_launch(f, sums, leaf_out, data, rows, stream, strategy, sums_in, csr, cols, table);
        if (ss != TAHOE_OK) return ss;
    } else if (strategy == TAHOE_STRATEGY_QRING) {
        const tahoe_status qs = qring_launch(f, sums, leaf_out, data, rows, stream, timed ? f->ev_mid[f->prof_count] : nullptr, sums_in, cols, table);
        mid_recorded = timed;
        if (qs != TAHOE_OK) return qs;
    } else if (strategy == TAHOE_STRATEGY_TILERING && tilering_rows(f) == 0 && widef_rows(f) > 0) {
        const tahoe_status ws = widef_launch(f, sums, leaf_out, data, rows, stream, sums_in);  // rows too wide for a 64-row tile
        if (ws != TAHOE_OK) return ws;
    } else if (strategy == TAHOE_STRATEGY_TILERING) {
        if (tilering_rows(f) == 128)
            launch_tilering<128, 4>(f, sums, leaf_out, sums_in, data, rows, stream, vec4_ok);
        else
            launch_tilering<64, 8>(f, sums, leaf_out, sums_in, data, rows, stream, vec4_ok);
        TAHOE_HIP_TRY(hipGetLastError());
    } else if (strategy == TAHOE_STRATEGY_TILEBLOCK) {
        if (tileblock_rows(f) == 128)
            launch_tileblock<128>(f, sums, leaf_out, sums_in, data, rows, stream, vec4_ok);
        else
            launch_tileblock<64>(f, sums, leaf_out, sums_in, data, rows, stream, vec4_ok);
        TAHOE_HIP_TRY(hipGetLastError());
    } else if (strategy == TAHOE_STRATEGY_ROWTILE) {
        const size_t grid = (rows + kTileRows - 1) / kTileRows;
        const int lds = rowtile_lds_bytes(f->p.num_cols, f->lds_levels);
        const int nc = f->num_classes;
        with_leaf_mc_nanm(leaf_out != nullptr, nc > 1, f->nan_missing, [&](auto wl, auto mc, auto nanm) {
            constexpr bool NANM = decltype(nanm)::value;
            if (csr)  // (predictions only: no leaf-index form)
                hipLaunchKernelGGL((rowtile_kernel<false, decltype(mc)::value, true, false, false, NANM>), dim3((unsigned)grid), dim3(kBlock), lds, stream,
                                   f->inner, f->leaf_val, f->leaf_orig, data, sums, leaf_out, sums_in, rows, f->p.num_cols,
                                   f->p.num_trees, f->depth, f->lds_levels, f->p.missing, vec4_ok, nc, *csr, nullptr, 0, ColsView{});
            else if (cols)
                hipLaunchKernelGGL((rowtile_kernel<false, decltype(mc)::value, false, false, true, NANM>), dim3((unsigned)grid), dim3(kBlock), lds,
                                   stream, f->inner, f->leaf_val, f->leaf_orig, data, sums, leaf_out, sums_in, rows, f->p.num_cols,
                                   f->p.num_trees, f->depth, f->lds_levels, f->p.missing, 0, nc, CsrView{}, nullptr, 0, *cols);
            else
                hipLaunchKernelGGL((rowtile_kernel<decltype(wl)::value, decltype(mc)::value, false, false, false, NANM>), dim3((unsigned)grid), dim3(kBlock), lds,
                                   stream, f->inner, f->leaf_val, f->leaf_orig, data, sums, leaf_out, sums_in, rows, f->p.num_cols,
                                   f->p.num_trees, f->depth, f->lds_levels, f->p.missing, vec4_ok, nc, CsrView{}, nullptr, 0, ColsView{});
        });
        TAHOE_HIP_TRY(hipGetLastError());
    } else if (strategy == TAHOE_STRATEGY_DIRECT) {
        const size_t grid = (rows + kBlock - 1) / kBlock;
        const int nc = f->num_classes;
        with_leaf_mc_nanm(leaf_out != nullptr, nc > 1, f->nan_missing, [&](auto wl, auto mc, auto nanm) {
            hipLaunchKernelGGL((direct_kernel<decltype(wl)::value, decltype(mc)::value, false, decltype(nanm)::value>), dim3((unsigned)grid), dim3(kBlock), 0,
                               stream, f->inner, f->leaf_val, f->leaf_orig, data, sums, leaf_out, sums_in, rows, f->p.num_cols,
                               f->p.num_trees, f->depth, f->p.missing, nc, nullptr, 0);
        });
        TAHOE_HIP_TRY(hipGetLastError());
    } else {
        return fail(TAHOE_ERR_INVALID_ARG, "unknown strategy %d", strategy);
    }
    if (timed) {
        if (!mid_recorded) TAHOE_HIP_TRY(hipEventRecord(f->ev_mid[f->prof_count], stream));
        TAHOE_HIP_TRY(hipEventRecord(f->ev_stop[f->prof_count], stream));
        ++f->prof_count;
    }
    return TAHOE_OK;
}

static tahoe_status launch_transform(float *preds, size_t rows, int output, int num_trees, float threshold,
                                     float global_bias, hipStream_t stream)
{
    // forest::predict runs transform_k only when it changes something (Struct.h:263).
    if (rows == 0 || (output == TAHOE_OUT_RAW && global_bias == 0.0f)) return TAHOE_OK;
    const size_t grid = (rows + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(transform_kernel, dim3((unsigned)grid), dim3(kBlock), 0, stream, preds, rows, output,
                       num_trees, threshold, global_bias);
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

static tahoe_status launch_transform_mc(const tahoe_forest *f, float *preds, size_t rows, hipStream_t stream)
{
    if (rows == 0 || (f->p.output == TAHOE_OUT_RAW && f->p.global_bias == 0.0f)) return TAHOE_OK;
    const size_t grid = (rows + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(transform_mc_kernel, dim3((unsigned)grid), dim3(kBlock), 0, stream, preds, rows, f->num_classes, f->p.output,
                       f->class_trees, f->p.global_bias);
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

// The reference's adaptive-format width rule (Struct.h:1827-1852): bytes of the packed bits word.
static int reference_bits_bytes(int max_fid)
{
    if (max_fid <= 0) return 1;
    const int len = (int)((std::log2((double)max_fid) + 3.0) / 8.0);
    return len == 0 ? 1 : (len == 1 ? 2 : 4);
}

tahoe_status check_params(const tahoe_forest_params *p, int num_classes, bool have_nodes, const char *nodes)
{
    if (p->num_trees < 0) return fail(TAHOE_ERR_INVALID_ARG, "num_trees must be non-negative");
    if (p->num_cols < 0) return fail(TAHOE_ERR_INVALID_ARG, "num_cols must be non-negative");
    if ((p->output & ~(TAHOE_OUT_AVG | TAHOE_OUT_SIGMOID | TAHOE_OUT_THRESHOLD | (num_classes > 1 ? TAHOE_OUT_SOFTMAX : 0))) != 0)
        return fail(TAHOE_ERR_INVALID_ARG, "output should be a combination of RAW, AVG, SIGMOID and THRESHOLD");
    if (p->num_trees > 0 && !have_nodes) return fail(TAHOE_ERR_INVALID_ARG, "%s is null", nodes);
    return TAHOE_OK;
}

tahoe_status check_classes(const tahoe_forest_params *p, int num_classes)
{
    if (num_classes < 1 || num_classes > 1024) return fail(TAHOE_ERR_INVALID_ARG, "num_classes must be in [1,1024], got %d", num_classes);
    if (p->num_trees < 0 || p->num_trees % num_classes != 0)
        return fail(TAHOE_ERR_INVALID_ARG, "num_trees (%d) must be a non-negative multiple of num_classes (%d)", p->num_trees, num_classes);
    if ((p->output & TAHOE_OUT_SOFTMAX) != 0 && num_classes == 1)
        return fail(TAHOE_ERR_INVALID_ARG, "SOFTMAX needs num_classes > 1");
    if ((p->output & TAHOE_OUT_SOFTMAX) != 0 && (p->output & TAHOE_OUT_SIGMOID) != 0)
        return fail(TAHOE_ERR_INVALID_ARG, "SOFTMAX and SIGMOID exclude each other");
    if ((p->output & TAHOE_OUT_THRESHOLD) != 0 && num_classes > 1)
        return fail(TAHOE_ERR_INVALID_ARG, "THRESHOLD needs num_classes == 1");
    return TAHOE_OK;
}

// The one reader of the handle knobs (struct tahoe_knobs)
static tahoe_knobs read_knobs()
{
    auto num = [](const char *name, int unset) {
        const char *e = getenv(name);
        return e ? atoi(e) : unset;
    };
    auto on = [&](const char *name) { return num(name, 1) != 0; };  // the knobs that "= 0" turns off
    tahoe_knobs k;
    k.lds_levels = num("TAHOE_LDS_LEVELS", k.lds_levels);
    k.tile_rows = num("TAHOE_TILE_ROWS", k.tile_rows);
    k.qring_walkers = num("TAHOE_QRING_WALKERS", k.qring_walkers);
    k.qring_chains = num("TAHOE_QRING_CHAINS", k.qring_chains);
    k.qring_slices = num("TAHOE_QRING_SLICES", k.qring_slices);
    k.qring_groups = num("TAHOE_QRING_GROUPS", k.qring_groups);
    k.qring_wide_chains = num("TAHOE_QRING_WIDE_CHAINS", k.qring_wide_chains);
    k.qring_wide = on("TAHOE_QRING_WIDE");
    k.qring_narrow = on("TAHOE_QRING_NARROW");
    k.qring_regions = on("TAHOE_QRING_REGIONS");
    k.qring_code8 = on("TAHOE_QRING_CODE8");
    k.qring_narrow128 = on("TAHOE_QRING_NARROW128");
    k.qring_top24 = on("TAHOE_QRING_TOP24");
    k.quant_buckets = on("TAHOE_QUANT_BUCKETS");
    k.quant_multi = on("TAHOE_QUANT_MULTI");
    k.sparse_qring = on("TAHOE_SPARSE_QRING");
    k.widef = on("TAHOE_WIDEF");
    k.wstream = num("TAHOE_WSTREAM", k.wstream);
    k.wstream_slab_mb = num("TAHOE_WSTREAM_SLAB_MB", k.wstream_slab_mb);
    k.approx_form = num("TAHOE_APPROX_FORM", k.approx_form);
    k.csr_chunk_mb = num("TAHOE_CSR_CHUNK_MB", k.csr_chunk_mb);
    k.csr_fused = num("TAHOE_CSR_FUSED", k.csr_fused);
    k.columns_fused = num("TAHOE_COLUMNS_FUSED", k.columns_fused);
    k.table_fused = num("TAHOE_TABLE_FUSED", k.table_fused);
    k.oblivious_shap_inplace = num("TAHOE_OBLIVIOUS_SHAP_INPLACE", 0) != 0;
    k.vector_shap_kb = num("TAHOE_VECTOR_SHAP_KB", k.vector_shap_kb);
    k.vector_shap_grid = num("TAHOE_VECTOR_SHAP_GRID", k.vector_shap_grid);
    k.pd_chunk_rows = num("TAHOE_PD_CHUNK_ROWS", k.pd_chunk_rows);
    return k;
}

tahoe_status open_handle(const tahoe_forest_params *p, int num_classes, ForestPtr &f)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(TAHOE_ERR_NO_DEVICE, "no HIP device is visible; libtahoe_amd has no CPU path");
    int dev = 0;
    TAHOE_HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    TAHOE_HIP_TRY(hipGetDeviceProperties(&prop, dev));
    f.reset(new (std::nothrow) tahoe_forest());
    if (!f) return fail(TAHOE_ERR_NO_MEMORY, "tahoe_forest_create");
    f->p = *p;
    f->num_classes = num_classes;
    f->class_trees = p->num_trees / num_classes;
    f->device = dev;
    f->num_cus = prop.multiProcessorCount;
    f->lds_limit = (int)prop.maxSharedMemoryPerMultiProcessor > 0 ? (int)prop.maxSharedMemoryPerMultiProcessor
                                                                   : (int)prop.sharedMemPerBlock;
    f->knobs = read_knobs();
    if (const tahoe_status s = hip_status(hipMalloc(reinterpret_cast<void **>(&f->error_flag), 2 * sizeof(int)), "hipMalloc(error_flag)"))
        return s;
    return hip_status(hipMemset(f->error_flag, 0, 2 * sizeof(int)), "hipMemset(error_flag)");
}

// The float32 kernels of a dense handle that may need more than the default 64 KiB of dynamic LDS: every form its shape can take
static tahoe_status allow_float32_lds(const tahoe_forest *f)
{
    const int lim = f->lds_limit;
    hipError_t e = hipSuccess;
    if (rowtile_fits(f) &&
        ((e = allow_max_lds_leaf([](auto wl) { return &rowtile_kernel<decltype(wl)::value>; }, lim)) != hipSuccess ||
         (f->num_classes > 1 && (e = allow_max_lds_leaf([](auto wl) { return &rowtile_kernel<decltype(wl)::value, true>; }, lim)) != hipSuccess) ||
         (e = allow_max_lds(reinterpret_cast<const void *>(&rowtile_kernel<false, false, true>), lim)) != hipSuccess ||
         (e = allow_max_lds(reinterpret_cast<const void *>(&rowtile_kernel<false, true, true>), lim)) != hipSuccess ||
         (e = allow_max_lds(reinterpret_cast<const void *>(&rowtile_kernel<false, false, false, false, true>), lim)) != hipSuccess ||
         (e = allow_max_lds(reinterpret_cast<const void *>(&rowtile_kernel<false, true, false, false, true>), lim)) != hipSuccess))
        return hip_status(e, "hipFuncSetAttribute(rowtile)");
    if (rowtile_fits(f) && f->nan_missing)  // ... and the same forms under TAHOE_CREATE_NAN_MISSING, the staged ones included
        for (const void *k : {(const void *)&rowtile_kernel<false, false, false, false, false, true>, (const void *)&rowtile_kernel<true, false, false, false, false, true>,
                              (const void *)&rowtile_kernel<false, true, false, false, false, true>, (const void *)&rowtile_kernel<true, true, false, false, false, true>,
                              (const void *)&rowtile_kernel<false, false, true, false, false, true>, (const void *)&rowtile_kernel<false, true, true, false, false, true>,
                              (const void *)&rowtile_kernel<false, false, false, false, true, true>, (const void *)&rowtile_kernel<false, true, false, false, true, true>,
                              (const void *)&rowtile_kernel<false, false, false, true, false, true>, (const void *)&rowtile_kernel<false, true, false, true, false, true>})
            if ((e = allow_max_lds(k, lim)) != hipSuccess) return hip_status(e, "hipFuncSetAttribute(rowtile, NaN missing)");
    if (!f->has_blocks) return TAHOE_OK;
    if ((tileblock_lds_bytes(f, 128) <= lim &&
         (e = allow_max_lds_leaf([](auto wl) { return &tileblock_kernel<128, decltype(wl)::value>; }, lim)) != hipSuccess) ||
        (tileblock_lds_bytes(f, 64) <= lim &&
         (e = allow_max_lds_leaf([](auto wl) { return &tileblock_kernel<64, decltype(wl)::value>; }, lim)) != hipSuccess))
        return hip_status(e, "hipFuncSetAttribute(tileblock)");
    if ((tilering_lds_bytes(f, 64) <= lim &&
         (e = allow_max_lds_leaf([](auto wl) { return &tilering_kernel<64, 8, decltype(wl)::value>; }, lim)) != hipSuccess) ||
        (tilering_lds_bytes(f, 128) <= lim &&
         (e = allow_max_lds_leaf([](auto wl) { return &tilering_kernel<128, 4, decltype(wl)::value>; }, lim)) != hipSuccess))
        return hip_status(e, "hipFuncSetAttribute(tilering)");
    return TAHOE_OK;
}

tahoe_status predict_rows(tahoe_forest *f, float *preds, const float *data, size_t rows, hipStream_t stream, const CsrView *csr,
                          int csr_strategy, const ColsView *cols, const TableView *table)
{
    DeviceGuard on_device(f->device);
    tahoe_status s = launch_traversal(f, preds, nullptr, data, rows, stream, nullptr, csr, csr_strategy, cols, table);
    if (s != TAHOE_OK) return s;
    if (f->num_classes > 1) return launch_transform_mc(f, preds, rows, stream);
    return launch_transform(preds, rows, f->p.output, f->p.num_trees, f->p.threshold, f->p.global_bias, stream);
}

// The strategy of tahoe_forest_predict_staged: a forced one that has a staged form, or AUTO's -- the tile kernel that needs no
// pre-pass (a sparse handle: TILEBLOCK, else ROWTILE, else DIRECT; a dense one: ROWTILE when its tile fits LDS, else DIRECT).
// An oblivious or vector-leaf handle (TAHOE_CREATE_STAGED) walks as tahoe_forest_predict does: DIRECT or ROWTILE, AUTO by its tile.
// 0: no stages are set, or the forced strategy (QRING, TILERING, dense TILEBLOCK) has no staged form.
static int staged_strategy(const tahoe_forest *f)
{
    if (!f->stages_dev) return 0;  // (an oblivious or vector-leaf handle without TAHOE_CREATE_STAGED never has stages)
    if (f->ob || f->vl) return resolve_strategy(f, 0);  // (never a third strategy: strategy_available)
    const int forced = f->strategy;  // (tahoe_forest_set_strategy has checked that the handle can run it)
    if (forced == TAHOE_STRATEGY_DIRECT || forced == TAHOE_STRATEGY_ROWTILE) return forced;
    if (f->sp) {
        if (forced == TAHOE_STRATEGY_TILEBLOCK) return forced;
        if (forced != TAHOE_STRATEGY_AUTO) return 0;
        if (sparse_top_waves(f) > 0) return TAHOE_STRATEGY_TILEBLOCK;
        return sparse_tile_fits(f) ? TAHOE_STRATEGY_ROWTILE : TAHOE_STRATEGY_DIRECT;
    }
    if (forced != TAHOE_STRATEGY_AUTO) return 0;
    return rowtile_fits(f) ? TAHOE_STRATEGY_ROWTILE : TAHOE_STRATEGY_DIRECT;
}

// The walk of tahoe_forest_predict_staged over a dense handle: DIRECT or ROWTILE with the stage stores
static tahoe_status launch_staged_dense(tahoe_forest *f, float *out, const float *data, size_t rows, hipStream_t stream, int strategy)
{
    const int nc = f->num_classes, S = (int)f->num_stages;
    const int vec4_ok = (f->p.num_cols % 4 == 0) && ((reinterpret_cast<uintptr_t>(data) & 15u) == 0);
    auto with_mc = [&](auto &&fn) {  // fn(multi-class, NaN is missing)
        with_leaf_mc(nc > 1, f->nan_missing, fn);
    };
    if (strategy == TAHOE_STRATEGY_ROWTILE) {
        const size_t grid = (rows + kTileRows - 1) / kTileRows;
        const int lds = rowtile_lds_bytes(f->p.num_cols, f->lds_levels);
        with_mc([&](auto mc, auto nanm) {
            hipLaunchKernelGGL((rowtile_kernel<false, decltype(mc)::value, false, true, false, decltype(nanm)::value>), dim3((unsigned)grid), dim3(kBlock), lds, stream,
                               f->inner, f->leaf_val, f->leaf_orig, data, out, nullptr, nullptr, rows, f->p.num_cols, f->p.num_trees,
                               f->depth, f->lds_levels, f->p.missing, vec4_ok, nc, CsrView{}, f->stages_dev, S, ColsView{});
        });
    } else {
        const size_t grid = (rows + kBlock - 1) / kBlock;
        with_mc([&](auto mc, auto nanm) {
            hipLaunchKernelGGL((direct_kernel<false, decltype(mc)::value, true, decltype(nanm)::value>), dim3((unsigned)grid), dim3(kBlock), 0, stream, f->inner,
                               f->leaf_val, f->leaf_orig, data, out, nullptr, nullptr, rows, f->p.num_cols, f->p.num_trees, f->depth,
                               f->p.missing, nc, f->stages_dev, S);
        });
    }
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

int csr_fused_strategy(const tahoe_forest *f, size_t rows, size_t nnz)
{
    if (f->p.num_trees == 0) return -1;
    const bool tile = f->ob ? oblivious_tile_fits(f) : f->vl ? vector_tile_fits(f) : f->sp ? sparse_tile_fits(f) : rowtile_fits(f);
    const bool top = f->sp && sparse_top_waves(f) > 0;
    // a forced strategy is honoured: the tile kernels that have the loader take it, every other strategy gets dense chunks
    if (f->strategy == TAHOE_STRATEGY_ROWTILE) return tile ? TAHOE_STRATEGY_ROWTILE : -1;
    if (f->strategy == TAHOE_STRATEGY_TILEBLOCK) return top ? TAHOE_STRATEGY_TILEBLOCK : -1;
    if (f->strategy != TAHOE_STRATEGY_AUTO || f->knobs.csr_fused == 0) return -1;
    const int fused = top ? TAHOE_STRATEGY_TILEBLOCK : tile ? TAHOE_STRATEGY_ROWTILE : -1;
    if (f->knobs.csr_fused > 0) return fused;
    if (f->ob || f->vl) {
        // An oblivious or vector-leaf handle (TAHOE_CREATE_CSR), as measured (tools/native_csr_time.py,
        // profiles/native_csr/native_csr_time.json).  AUTO runs the tile kernel on dense rows whenever the tile
        // fits, so rule 1 alone would take the fused form at every density; it lost where rows store many entries: the one-wave
        // loader scatters a row's entries 8 at a time behind two dependent loads, once per block of 8 classes, and a 64-row tile
        // keeps ever fewer waves on a CU as it widens, while the densify pass costs the same per column at any density.  Both
        // sides grow with num_cols, and the crossover sat near 100 stagings of an entry per row at 64 and at 512 columns (200 k
        // rows, 100 trees: 64 columns, every entry stored, K = 8 fused / fallback 0.95, K = 10 -- two class blocks -- 1.02; 512
        // columns, K = 8, oblivious 0.80 at 26 entries per row and 1.10 at 128, vector-leaf 0.77 at 26, 0.95 at 128 and 1.46
        // at 512); a threshold of 96 keeps all of those on their faster side but the vector-leaf cell at 128, which it gives up 5 %.
        const double class_blocks = (double)((f->num_classes + 7) / 8);  // (kObClasses = kVecClasses = 8)
        return tile && (double)nnz * class_blocks <= 96.0 * (double)rows ? TAHOE_STRATEGY_ROWTILE : -1;
    }
    // AUTO, as measured (tools/csr_time.py, profiles/csr/csr_time.json).  Where AUTO runs that tile kernel
    // on dense rows anyway, the same kernel fed from CSR saves writing the chunk and reading it back: faster at every density.
    if (resolve_strategy(f, rows) == fused) return fused;
    // A dense handle whose AUTO is another form (QRING, TILERING): ROWTILE from CSR beats densify + AUTO while the forest is
    // light for its width (trees x depth <= 8 x num_cols, the heaviest shape it was measured to win on) and at most a quarter
    // of the entries is stored (500 x depth 8 on 500 features: 1.9 - 2.2 ms against 3.3 - 3.6 ms; with every entry stored 3.4
    // against 2.8 ms).  Heavier forests are where QRING outruns ROWTILE by more than the densify pass costs.
    if (!f->sp && tile && (long long)f->p.num_trees * f->depth <= 8LL * f->p.num_cols &&
        4.0 * (double)nnz <= (double)rows * (double)f->p.num_cols)
        return TAHOE_STRATEGY_ROWTILE;
    return -1;
}

// Which kernel reads a column-major batch in place.  The strategy is the one the same handle runs on
// row-major rows -- a forced one, or AUTO's for this many rows -- whenever that strategy has a column loader: QRING (every form
// walks codes; only the quantise pass reads floats), ROWTILE where the 64-row tile fits, TILEBLOCK on a sparse handle.  There
// is no rule that swaps AUTO's form for another.  Everything else, and every oblivious or vector-leaf handle, gets chunks.
int columns_fused_strategy(const tahoe_forest *f, size_t rows)
{
    if (f->p.num_trees == 0 || f->p.num_cols == 0 || f->ob || f->vl) return -1;
    if (f->strategy == TAHOE_STRATEGY_AUTO && f->knobs.columns_fused == 0) return -1;
    const int s = resolve_strategy(f, rows);  // (a forced strategy resolves to itself)
    if (s == TAHOE_STRATEGY_QRING) return (f->sp ? sparse_q_available(f) : qring_walkers(f) > 0) ? s : -1;
    if (s == TAHOE_STRATEGY_ROWTILE) return (f->sp ? sparse_tile_fits(f) : rowtile_fits(f)) ? s : -1;
    if (s == TAHOE_STRATEGY_TILEBLOCK) return f->sp && sparse_top_waves(f) > 0 ? s : -1;
    return -1;
}

// Which kernel reads a typed table in place: QRING's quantise pass, where QRING is the strategy the same
// handle runs on row-major rows -- forced, or AUTO's for this many rows.  No rule swaps AUTO's form.  Everything else -- the
// float32 tile kernels too, which have no typed loader yet -- and every oblivious or vector-leaf handle gets chunks.
int table_fused_strategy(const tahoe_forest *f, size_t rows)
{
    if (f->p.num_trees == 0 || f->p.num_cols == 0 || f->ob || f->vl) return -1;
    if (f->strategy == TAHOE_STRATEGY_AUTO && f->knobs.table_fused == 0) return -1;
    const int s = resolve_strategy(f, rows);  // (a forced strategy resolves to itself)
    if (s == TAHOE_STRATEGY_QRING) return (f->sp ? sparse_q_available(f) : qring_walkers(f) > 0) ? s : -1;
    return -1;
}

}  // namespace tahoe

using namespace tahoe;

extern "C" {

tahoe_status tahoe_forest_create(tahoe_forest **out, const tahoe_dense_node *nodes, const tahoe_forest_params *p)
{
    unsigned flags = 0;
    if (const char *e = getenv("TAHOE_RELAYOUT"))  // experiments: the re-layout without touching the caller
        if (atoi(e) != 0) flags |= TAHOE_CREATE_PROB_RELAYOUT;
    return tahoe_forest_create_ex(out, nodes, p, flags);
}

// num_classes > 1: tahoe_forest_create_multiclass, whose own checks have run; the trees are laid out class-major.
static tahoe_status create_dense(tahoe_forest **out, const tahoe_dense_node *nodes, const tahoe_forest_params *p, unsigned flags,
                                 int num_classes)
{
    if (!out || !p) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_create: null argument");
    if ((flags & ~(unsigned)(TAHOE_CREATE_PROB_RELAYOUT | TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_APPROX_CONTRIBS | TAHOE_CREATE_NAN_MISSING)) != 0)
        return fail(TAHOE_ERR_INVALID_ARG, "unknown create flags 0x%x", flags);
    if (const tahoe_status s = check_nan_missing_flags(flags, nullptr)) return s;
    *out = nullptr;
    if (p->depth < 0 || p->depth > 30) return fail(TAHOE_ERR_INVALID_ARG, "depth must be in [0,30], got %d", p->depth);
    if (p->algo < TAHOE_ALGO_NAIVE || p->algo > TAHOE_ALGO_BATCH_TREE_REORG)
        return fail(TAHOE_ERR_INVALID_ARG, "algo should be NAIVE, TREE_REORG or BATCH_TREE_REORG");
    if (const tahoe_status s = check_params(p, num_classes, nodes != nullptr, "nodes")) return s;
    if (flags & (TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_APPROX_CONTRIBS)) {  // the cover weights, on the caller's nodes, before a device is touched
        const tahoe_status cs = contribs_validate(nodes, p);
        if (cs != TAHOE_OK) return cs;
    }

    ForestPtr f;
    if (const tahoe_status s = open_handle(p, num_classes, f)) return s;
    const int D = p->depth;             // depth of the trees as given
    const int De = std::max(D, 2);      // depth of the normalised trees
    f->depth = De;
    f->n_inner = ((size_t)1 << De) - 1;
    f->n_leaf = (size_t)1 << De;
    // (TAHOE_LDS_LEVELS never raises the caps)
    f->lds_levels = std::max(0, std::min({De, kMaxLdsLevels, f->knobs.lds_levels}));
    f->top_levels = std::max(0, std::min({De - 2, kTopLevelsMax, f->knobs.lds_levels}));
    f->relayout = (flags & TAHOE_CREATE_PROB_RELAYOUT) != 0;
    f->nan_missing = (flags & TAHOE_CREATE_NAN_MISSING) != 0;
    // the float32 top / block views pack fid and def_left into 10 / 16 bits: no room for the exchange bit; and the kernels that
    // walk them (TILEBLOCK, TILERING) do not implement TAHOE_CREATE_NAN_MISSING, so such a handle does not build them
    f->has_blocks = p->num_cols <= kBlockMaxCols && !f->relayout && !f->nan_missing;

    // ---- normalise: heap records of the perfect depth-De tree ----
    const size_t T = (size_t)p->num_trees;
    const size_t src_nodes = (size_t)tahoe_tree_num_nodes(D);
    // internal tree t is the caller's tree src_tree(t): the identity, or the class-major order of a multi-class handle
    const size_t n_cls = (size_t)num_classes, c_trees = (size_t)f->class_trees;
    auto src_tree = [n_cls, c_trees](size_t t) { return n_cls > 1 ? (t % c_trees) * n_cls + t / c_trees : t; };
    const size_t all_nodes = f->n_inner + f->n_leaf;
    std::vector<InnerNode> h_inner(T * f->n_inner);
    std::vector<float> h_leaf(T * f->n_leaf);
    std::vector<uint32_t> h_orig(T * f->n_leaf);
    std::vector<unsigned char> h_real(T * f->n_inner, 0);  // heap records that exist in the original tree
    // trees are independent: normalise them on several host threads; the first invalid node (in tree order) wins
    struct Bad {
        size_t tree = SIZE_MAX, node = 0;
        int kind = 0, fid = 0;  // 1: reachable bottom-level node is not a leaf, 2: fid >= num_cols
    };
    std::vector<Bad> bad_of;
    std::vector<int> max_fid_of;
    std::mutex collect;
    const int num_cols = p->num_cols;
    const size_t n_inner = f->n_inner, n_leaf = f->n_leaf;
    parallel_for(T, 8, [&, n_inner, n_leaf, num_cols](size_t t_lo, size_t t_hi) {
        std::vector<int64_t> inherit(all_nodes);
        Bad bad;
        int max_fid_local = 0;
        for (size_t t = t_lo; t < t_hi && bad.kind == 0; ++t) {
            const tahoe_dense_node *tree = nodes + src_tree(t) * src_nodes;
            for (size_t i = 0; i < all_nodes; ++i) {
                const int64_t up = i ? inherit[(i - 1) / 2] : -1;
                int fid = 0, def_left = 0, is_leaf = 0;
                float value = 0.0f;
                if (up >= 0) {
                    inherit[i] = up;  // below a leaf: unreachable in the original tree
                } else {
                    // i < src_nodes here: a node without a leaf above it is at most on the original bottom
                    // level, because the check below rejects non-leaves there.
                    tahoe_decode_node(&tree[i], &value, nullptr, &fid, &def_left, &is_leaf);
                    if (is_leaf) {
                        inherit[i] = (int64_t)i;
                    } else {
                        inherit[i] = -1;
                        if (2 * i + 2 >= src_nodes || fid >= num_cols) {
                            bad.tree = t;
                            bad.node = i;
                            bad.kind = 2 * i + 2 >= src_nodes ? 1 : 2;
                            bad.fid = fid;
                            break;
                        }
                        max_fid_local = std::max(max_fid_local, fid);
                    }
                }
                if (i < n_inner) {
                    InnerNode &n = h_inner[t * n_inner + i];
                    if (inherit[i] >= 0) {
                        n.thr = 0.0f;  // padding below a leaf: either child leads to the same value
                        n.meta = 0u;
                    } else {
                        n.thr = value;
                        n.meta = (uint32_t)fid | (def_left ? 0x80000000u : 0u);
                        h_real[t * n_inner + i] = 1;
                    }
                } else {
                    const size_t b = t * n_leaf + (i - n_inner);
                    h_leaf[b] = tree[inherit[i]].val;
                    h_orig[b] = (uint32_t)inherit[i];
                }
            }
        }
        std::lock_guard<std::mutex> lock(collect);
        if (bad.kind) bad_of.push_back(bad);
        max_fid_of.push_back(max_fid_local);
    });
    if (!bad_of.empty()) {
        const Bad bad = *std::min_element(bad_of.begin(), bad_of.end(), [](const Bad &x, const Bad &y) { return x.tree < y.tree; });
        if (bad.kind == 1)
            return fail(TAHOE_ERR_INVALID_FOREST,
                        "tree %zu: reachable bottom-level node %zu is not a leaf (the reference would walk out of the tree)",
                        bad.tree, bad.node);
        return fail(TAHOE_ERR_INVALID_FOREST, "tree %zu node %zu: fid %d >= num_cols %d", bad.tree, bad.node, bad.fid, num_cols);
    }
    // ---- probability-guided re-layout (dense_adaptive_forest::init step (ii), Struct.h:1775-1825 with
    // swap_child :1712-1750): bottom-up, at every internal node whose left child weighs less than its right child the
    // two subtrees change places and the node gets the exchange bit, so the likelier child is always the left one.
    // leaf_orig moves with the leaves: leaf indices stay in the original heap numbering.
    if (f->relayout) {
        std::vector<size_t> swaps_of;
        parallel_for(T, 8, [&, n_inner, n_leaf](size_t t_lo, size_t t_hi) {
            std::vector<float> w(all_nodes);
            size_t swaps = 0;
            for (size_t t = t_lo; t < t_hi; ++t) {
                const tahoe_dense_node *tree = nodes + src_tree(t) * src_nodes;
                for (size_t i = 0; i < all_nodes; ++i) w[i] = i < src_nodes ? tree[i].weight : 0.0f;
                InnerNode *in = &h_inner[t * n_inner];
                unsigned char *re = &h_real[t * n_inner];
                float *lv = &h_leaf[t * n_leaf];
                uint32_t *lo = &h_orig[t * n_leaf];
                for (int l = De - 1; l >= 0; --l) {
                    for (size_t i = ((size_t)1 << l) - 1; i < ((size_t)2 << l) - 1; ++i) {
                        if (!re[i]) continue;                    // padding below a leaf: nothing to order
                        const size_t a = 2 * i + 1, b = 2 * i + 2;
                        if (!(w[a] < w[b])) continue;            // Struct.h:1791: swap when the left child is the lighter one
                        for (int d = 0;; ++d) {                  // the two subtrees, level by level
                            const size_t sa = ((a + 1) << d) - 1, sb = ((b + 1) << d) - 1, len = (size_t)1 << d;
                            if (sa >= n_inner) {                 // leaf level of the normalised tree
                                std::swap_ranges(lv + (sa - n_inner), lv + (sa - n_inner) + len, lv + (sb - n_inner));
                                std::swap_ranges(lo + (sa - n_inner), lo + (sa - n_inner) + len, lo + (sb - n_inner));
                                break;
                            }
                            std::swap_ranges(in + sa, in + sa + len, in + sb);
                            std::swap_ranges(re + sa, re + sa + len, re + sb);
                            std::swap_ranges(w.begin() + sa, w.begin() + sa + len, w.begin() + sb);
                        }
                        in[i].meta |= kMetaExchange;
                        ++swaps;
                    }
                }
            }
            std::lock_guard<std::mutex> lock(collect);
            swaps_of.push_back(swaps);
        });
        for (size_t n : swaps_of) f->relayout_swaps += n;
    }
    int max_fid = 0;
    for (int m : max_fid_of) max_fid = std::max(max_fid, m);
    f->bits_bytes = reference_bits_bytes(max_fid);

    // ---- TILEBLOCK views: SoA tops and 32-byte bottom blocks ----
    std::vector<unsigned char> h_top;
    std::vector<uint4> h_blocks;
    if (f->has_blocks) {
        const int n_top = top_nodes(f->top_levels);
        const int stride = top_stride_bytes(f->top_levels);
        const int meta_off = top_thr_bytes(f->top_levels);
        h_top.assign(T * (size_t)stride, 0);
        const size_t n_blocks = (size_t)1 << (De - 2);
        const size_t first = n_blocks - 1;
        h_blocks.resize(T * n_blocks * 2);
        parallel_for(T, 8, [&, n_inner, n_leaf](size_t t_lo, size_t t_hi) {
        for (size_t t = t_lo; t < t_hi; ++t) {
            const InnerNode *in = &h_inner[t * n_inner];
            float *thr = reinterpret_cast<float *>(&h_top[t * stride]);
            uint16_t *meta = reinterpret_cast<uint16_t *>(&h_top[t * stride + meta_off]);
            for (int i = 0; i < n_top; ++i) {  // heap node i -> position i + 1
                thr[i + 1] = in[i].thr;
                meta[i + 1] = (uint16_t)((in[i].meta & 0x7fffu) | ((in[i].meta >> 31) << 15));
            }
            for (size_t b = 0; b < n_blocks; ++b) {
                const size_t r = first + b, l = 2 * r + 1, rr = 2 * r + 2;  // subtree root and its children
                auto pack = [](const InnerNode &n) { return (n.meta & 0x1ffu) | ((n.meta >> 31) << 9); };
                uint4 a, v;
                memcpy(&a.x, &in[r].thr, 4);
                memcpy(&a.y, &in[l].thr, 4);
                memcpy(&a.z, &in[rr].thr, 4);
                a.w = pack(in[r]) | (pack(in[l]) << 10) | (pack(in[rr]) << 20);
                const float *lv = &h_leaf[t * n_leaf + 4 * b];
                memcpy(&v.x, &lv[0], 4);
                memcpy(&v.y, &lv[1], 4);
                memcpy(&v.z, &lv[2], 4);
                memcpy(&v.w, &lv[3], 4);
                h_blocks[(t * n_blocks + b) * 2 + 0] = a;
                h_blocks[(t * n_blocks + b) * 2 + 1] = v;
            }
        }
        });
    }

    tahoe_status s;
    if ((s = hip_status(upload(&f->inner, h_inner, &f->device_bytes), "upload(inner)")) ||
        (s = hip_status(upload(&f->leaf_val, h_leaf, &f->device_bytes), "upload(leaf_val)")) ||
        (s = hip_status(upload(&f->leaf_orig, h_orig, &f->device_bytes), "upload(leaf_orig)")))
        return s;
    if (f->has_blocks && ((s = hip_status(upload(&f->top, h_top, &f->device_bytes), "upload(top)")) ||
                          (s = hip_status(upload(&f->blocks, h_blocks, &f->device_bytes), "upload(blocks)"))))
        return s;
    if ((s = allow_float32_lds(f.get())) || (s = qring_build(f.get(), h_inner, h_real, h_leaf))) return s;
    // no 64-row float32 tile kernel for this shape: the wide-row form
    // (not under TAHOE_CREATE_NAN_MISSING: neither wide-row kernel implements it)
    if (!f->nan_missing && tilering_rows(f.get()) == 0 && tileblock_rows(f.get()) == 0 && (s = widef_build(f.get(), h_inner, h_real, h_leaf)))
        return s;
    // contributions from the caller's nodes, the Saabas records of the final (class-major, re-laid-out) layout
    return finish_create(f, flags, out, [&] { return contribs_build(f.get(), nodes); },
                         [&] { return approx_build(f.get(), nodes, h_inner, h_real); });
}

tahoe_status tahoe_forest_create_ex(tahoe_forest **out, const tahoe_dense_node *nodes, const tahoe_forest_params *p, unsigned flags)
{
    return create_dense(out, nodes, p, flags, 1);
}

tahoe_status tahoe_forest_create_multiclass(tahoe_forest **out, const tahoe_dense_node *nodes, const tahoe_forest_params *p,
                                            int num_classes, unsigned flags)
{
    // every check here runs before a device is touched
    if (!out || !p) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_create_multiclass: null argument");
    *out = nullptr;
    if (const tahoe_status s = check_classes(p, num_classes)) return s;
    return create_dense(out, nodes, p, flags, num_classes);
}

int tahoe_forest_num_classes(const tahoe_forest *f) { return f ? f->num_classes : 0; }

void tahoe_forest_destroy(tahoe_forest *f)
{
    if (!f) return;
    if (f->inner) (void)hipFree(f->inner);
    if (f->leaf_val) (void)hipFree(f->leaf_val);
    if (f->leaf_orig) (void)hipFree(f->leaf_orig);
    if (f->top) (void)hipFree(f->top);
    if (f->blocks) (void)hipFree(f->blocks);
    if (f->error_flag) (void)hipFree(f->error_flag);
    if (f->stages_dev) (void)hipFree(f->stages_dev);
    pipeline_destroy(f);
    csr_destroy(f);
    qring_destroy(f);
    sparse_destroy(f);
    oblivious_destroy(f);
    vector_destroy(f);
    widef_destroy(f);
    interventional_destroy(f);
    contribs_destroy(f);
    approx_destroy(f);
    pd_destroy(f);
    for (hipEvent_t e : f->ev_start) (void)hipEventDestroy(e);
    for (hipEvent_t e : f->ev_mid) (void)hipEventDestroy(e);
    for (hipEvent_t e : f->ev_stop) (void)hipEventDestroy(e);
    delete f;
}

tahoe_status tahoe_forest_predict_raw(tahoe_forest *f, float *sums_dev, const float *data_dev, size_t rows,
                                      void *stream)
{
    if (!f || (rows && (!sums_dev || !data_dev)))
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_raw: null argument");
    return launch_traversal(f, sums_dev, nullptr, data_dev, rows, (hipStream_t)stream);
}

tahoe_status tahoe_forest_predict_accumulate(tahoe_forest *f, float *sums_dev, const float *data_dev, size_t rows,
                                             void *stream)
{
    if (!f || (rows && (!sums_dev || !data_dev)))
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_accumulate: null argument");
    if (const tahoe_status s = refuse_vector(f, "tahoe_forest_predict_accumulate")) return s;
    if (f->num_classes > 1) return fail(TAHOE_ERR_UNSUPPORTED, "tahoe_forest_predict_accumulate: not served on a multi-class handle");
    return launch_traversal(f, sums_dev, nullptr, data_dev, rows, (hipStream_t)stream, sums_dev);
}

tahoe_status tahoe_forest_predict(tahoe_forest *f, float *preds_dev, const float *data_dev, size_t rows,
                                  void *stream)
{
    if (!f || (rows && (!preds_dev || !data_dev)))
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict: null argument");
    return predict_rows(f, preds_dev, data_dev, rows, (hipStream_t)stream);
}

tahoe_status tahoe_forest_set_stages(tahoe_forest *f, const int32_t *rounds, int num_stages)
{
    // every check here runs before a device is touched
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_stages: null forest");
    if (const tahoe_status s = refuse_unstaged(f, "tahoe_forest_set_stages")) return s;
    if (num_stages < 0) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_stages: num_stages must be non-negative, got %d", num_stages);
    if (num_stages > 0 && !rounds) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_stages: rounds is null with num_stages %d", num_stages);
    for (int s = 0; s < num_stages; ++s) {
        if (rounds[s] < 1 || rounds[s] > f->class_trees)
            return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_stages: rounds[%d] = %d is outside [1, %d] (the trees of a class)", s,
                        rounds[s], f->class_trees);
        if (s > 0 && rounds[s] <= rounds[s - 1])
            return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_stages: rounds[%d] = %d is not above rounds[%d] = %d (strictly ascending)",
                        s, rounds[s], s - 1, rounds[s - 1]);
    }
    DeviceGuard on_device(f->device);
    int32_t *dev = nullptr;
    if (num_stages > 0) {
        // the staged tile kernels of this handle's kind may need more than the default 64 KiB of dynamic LDS
        hipError_t e = hipSuccess;
        if (f->ob) {
            if (const tahoe_status s = oblivious_allow_staged_lds(f)) return s;
        } else if (f->vl) {
            if (const tahoe_status s = vector_allow_staged_lds(f)) return s;
        } else if (f->sp) {
            if (const tahoe_status s = sparse_allow_staged_lds(f)) return s;
        } else if (rowtile_fits(f) &&
                   (e = allow_max_lds(f->num_classes > 1 ? reinterpret_cast<const void *>(&rowtile_kernel<false, true, false, true>)
                                                         : reinterpret_cast<const void *>(&rowtile_kernel<false, false, false, true>),
                                      f->lds_limit)) != hipSuccess) {
            return hip_status(e, "hipFuncSetAttribute(rowtile, staged)");
        }
        size_t counted = 0;
        e = upload(&dev, rounds, (size_t)num_stages, &counted);
        if (e != hipSuccess) {
            if (dev) (void)hipFree(dev);
            return e == hipErrorOutOfMemory ? fail(TAHOE_ERR_NO_MEMORY, "tahoe_forest_set_stages: hipMalloc of %d stages failed", num_stages)
                                            : hip_status(e, "upload(stages)");
        }
    }
    TAHOE_HIP_TRY(hipDeviceSynchronize());  // a staged predict in flight may still read the stages it was launched with
    if (f->stages_dev) {
        (void)hipFree(f->stages_dev);
        f->device_bytes -= f->num_stages * sizeof(int32_t);
    }
    f->stages_dev = dev;
    f->num_stages = (size_t)num_stages;
    f->device_bytes += f->num_stages * sizeof(int32_t);
    return TAHOE_OK;
}

int tahoe_forest_get_staged_strategy(const tahoe_forest *f, size_t rows) { return f ? staged_strategy(f) : -1; }

tahoe_status tahoe_forest_predict_staged(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows, void *stream)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_staged: null forest");
    if (const tahoe_status s = refuse_unstaged(f, "tahoe_forest_predict_staged")) return s;
    if (!f->stages_dev)
        return fail(TAHOE_ERR_UNSUPPORTED, "tahoe_forest_predict_staged: no stages are set (tahoe_forest_set_stages)");
    const int strategy = staged_strategy(f);
    if (strategy == 0)
        return fail(TAHOE_ERR_UNSUPPORTED, "tahoe_forest_predict_staged: the forced strategy %d has no staged form; a %s handle serves "
                                           "AUTO, DIRECT%s", f->strategy, f->sp ? "sparse" : "dense",
                    f->sp ? ", ROWTILE and TILEBLOCK" : " and ROWTILE");
    if (rows == 0) return TAHOE_OK;
    if (!out_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_staged: null argument");
    const size_t per_row = f->num_stages * (size_t)f->num_classes;  // <= num_trees
    if (rows > SIZE_MAX / sizeof(float) / per_row)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_staged: rows x stages x classes floats overflow size_t (rows %zu)", rows);
    if ((rows + 63) / 64 > 0x7fffffffu) return fail(TAHOE_ERR_INVALID_ARG, "too many rows for one launch: %zu", rows);
    DeviceGuard on_device(f->device);
    hipStream_t st = (hipStream_t)stream;
    const tahoe_status ws = f->ob   ? oblivious_launch_staged(f, out_dev, data_dev, rows, st, strategy)
                            : f->vl ? vector_launch_staged(f, out_dev, data_dev, rows, st, strategy)
                            : f->sp ? sparse_launch_staged(f, out_dev, data_dev, rows, st, strategy)
                                    : launch_staged_dense(f, out_dev, data_dev, rows, st, strategy);
    if (ws != TAHOE_OK) return ws;
    // (as predict_rows: the transform runs only when it changes something)
    if (f->p.output == TAHOE_OUT_RAW && f->p.global_bias == 0.0f) return TAHOE_OK;
    const size_t n = rows * f->num_stages;
    if ((n + kBlock - 1) / kBlock > 0x7fffffffu)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_staged: too many (row, stage) pairs for one launch: %zu", n);
    hipLaunchKernelGGL(transform_staged_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, out_dev, n,
                       (int)f->num_stages, f->num_classes, f->p.output, f->stages_dev, f->p.threshold, f->p.global_bias);
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

tahoe_status tahoe_forest_predict_leaf_idx(tahoe_forest *f, uint32_t *leaf_dev, float *sums_dev,
                                           const float *data_dev, size_t rows, void *stream)
{
    if (!f || (rows && (!leaf_dev || !data_dev)))
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_leaf_idx: null argument");
    return launch_traversal(f, sums_dev, leaf_dev, data_dev, rows, (hipStream_t)stream);
}

tahoe_status tahoe_transform_preds(float *preds_dev, size_t rows, int output, int num_trees_total, float threshold,
                                   float global_bias, void *stream)
{
    if (rows && !preds_dev) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_transform_preds: null argument");
    return launch_transform(preds_dev, rows, output, num_trees_total, threshold, global_bias, (hipStream_t)stream);
}

tahoe_status tahoe_forest_set_strategy(tahoe_forest *f, int strategy)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "null forest");
    if (strategy < TAHOE_STRATEGY_AUTO || strategy > TAHOE_STRATEGY_QRING)
        return fail(TAHOE_ERR_INVALID_ARG, "unknown strategy %d", strategy);
    if (const tahoe_status s = strategy_available(f, strategy)) return s;
    f->strategy = strategy;
    return TAHOE_OK;
}

tahoe_status tahoe_forest_reserve(tahoe_forest *f, size_t rows)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "null forest");
    if (f->ob || f->vl) return TAHOE_OK;  // an oblivious or vector-leaf handle has no workspace: predict allocates nothing
    const tahoe_status qs = qring_reserve(f, rows);
    if (qs != TAHOE_OK) return qs;
    return widef_reserve(f, rows);  // (the wide-row float32 form's leaf-value workspace, when it streams rows)
}

tahoe_status tahoe_forest_check(tahoe_forest *f, void *stream)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "null forest");
    TAHOE_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (f->error_flag) {
        int flags[2] = {0, 0};
        TAHOE_HIP_TRY(hipMemcpy(flags, f->error_flag, sizeof(flags), hipMemcpyDeviceToHost));
        if (flags[0] != 0) return fail(TAHOE_ERR_HIP, "a bounded LDS ring wait timed out (TILERING/QRING); results are invalid");
        if (flags[1] != 0) {  // reported once: a later clean call checks OK
            TAHOE_HIP_TRY(hipMemset(f->error_flag + 1, 0, sizeof(int)));
            return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_csr: an entry named a column outside [0, %d); such entries were "
                                               "skipped (their rows read the missing value there)", f->p.num_cols);
        }
    }
    return TAHOE_OK;
}

int tahoe_forest_get_strategy(const tahoe_forest *f, size_t rows) { return f ? resolve_strategy(f, rows) : -1; }

int tahoe_forest_get_kernel_form(const tahoe_forest *f, size_t rows)
{
    if (!f) return -1;
    const int strategy = resolve_strategy(f, rows);
    if (f->ob) return strategy == TAHOE_STRATEGY_ROWTILE ? TAHOE_OBLIVIOUS_FORM_TILE : TAHOE_OBLIVIOUS_FORM_DIRECT;
    if (f->vl) return strategy == TAHOE_STRATEGY_ROWTILE ? TAHOE_VECTOR_FORM_TILE : TAHOE_VECTOR_FORM_DIRECT;
    if (f->sp) {
        switch (strategy) {
        case TAHOE_STRATEGY_QRING: return TAHOE_FORM_SPARSE_QRING;
        case TAHOE_STRATEGY_TILEBLOCK: return TAHOE_FORM_SPARSE_TOP;
        case TAHOE_STRATEGY_ROWTILE: return TAHOE_FORM_SPARSE_ROWTILE;
        default: return TAHOE_FORM_SPARSE_DIRECT;
        }
    }
    switch (strategy) {
    case TAHOE_STRATEGY_QRING: return qring_form(f, rows);
    case TAHOE_STRATEGY_TILERING:
        if (tilering_rows(f) > 0) return TAHOE_FORM_TILERING_TILE;
        if (widef_rows(f) > 0) return widef_stream_slots(f) > 0 ? TAHOE_FORM_TILERING_WIDE_STREAM : TAHOE_FORM_TILERING_WIDE_TILE;
        return TAHOE_FORM_NONE;
    case TAHOE_STRATEGY_TILEBLOCK: return tileblock_rows(f) > 0 ? TAHOE_FORM_TILEBLOCK : TAHOE_FORM_NONE;
    case TAHOE_STRATEGY_ROWTILE: return rowtile_fits(f) ? TAHOE_FORM_ROWTILE : TAHOE_FORM_NONE;
    case TAHOE_STRATEGY_DIRECT: return TAHOE_FORM_DIRECT;
    default: return TAHOE_FORM_NONE;
    }
}

const char *tahoe_kernel_form_name(int form)
{
    static const char *const names[] = {"none", "direct", "rowtile", "tileblock", "tilering_tile", "tilering_wide_tile",
                                        "tilering_wide_stream", "qring_region3", "qring_region2", "qring_region_mixed",
                                        "qring_split", "qring_columns", "qring_wide", "qring_gx", "sparse_direct",
                                        "sparse_rowtile", "sparse_top", "sparse_qring", "qring_region8", "qring_region6",
                                        "csr_rowtile", "csr_sparse_rowtile", "csr_sparse_top", "?" /* 23: unassigned */, "oblivious_direct",
                                        "oblivious_tile", "?" /* 26: unassigned */, "vector_direct", "vector_tile", "?" /* 29: unassigned */,
                                        "oblivious_csr_tile", "vector_csr_tile", "?" /* 32: unassigned */, "columns_rowtile",
                                        "columns_sparse_rowtile", "columns_sparse_top"};
    return form >= 0 && form < (int)(sizeof(names) / sizeof(names[0])) ? names[form] : "?";
}

tahoe_status tahoe_forest_get_info(const tahoe_forest *f, tahoe_forest_info *info)
{
    if (!f || !info) return fail(TAHOE_ERR_INVALID_ARG, "null argument");
    memset(info, 0, sizeof(*info));
    info->is_sparse = f->sp != nullptr;
    info->num_trees = f->p.num_trees;
    info->num_cols = f->p.num_cols;
    info->bits_bytes = f->bits_bytes;
    info->device_bytes = f->device_bytes;
    info->device_id = f->device;
    info->num_cus = f->num_cus;
    if (f->sp) return TAHOE_OK;
    info->depth = f->p.depth;
    if (f->ob || f->vl) return TAHOE_OK;  // (depth: the largest of the trees)
    info->lds_levels = f->lds_levels;
    info->lds_bytes_per_block = rowtile_fits(f) ? rowtile_lds_bytes(f->p.num_cols, f->lds_levels) : 0;
    info->top_levels = f->top_levels;
    info->tile_rows = tileblock_rows(f);
    info->tileblock_lds_bytes = info->tile_rows ? (int)tileblock_lds_bytes(f, info->tile_rows) : 0;
    info->qring_walkers = qring_walkers(f);
    info->qring_lds_bytes = (int)qring_lds_bytes(f);
    info->qring_groups = qring_groups(f);
    info->ring_rows = tilering_rows(f) ? tilering_rows(f) : widef_rows(f);
    // (the wide-row float32 form has its own LDS plan: tile + walker slots + ring, or tops image + row slots when streaming)
    info->tilering_lds_bytes = tilering_rows(f) ? (int)tilering_lds_bytes(f, info->ring_rows) : (int)widef_lds_bytes(f);
    info->stream_slots = widef_stream_slots(f);
    info->stream_levels = widef_stream_levels(f);
    info->stream_key_ties = widef_stream_tie_estimate(f);
    info->qring_tile_rows = info->qring_walkers == 0 ? 0 : qwide_rows(f) ? qwide_rows(f) : (qring_code8(f) || qring_six16(f)) ? 384 : qring_regions(f) ? 192 : qring_lds_tile(f) ? 128 : 0;
    info->relayout = f->relayout ? 1 : 0;
    info->relayout_swaps = f->relayout_swaps;
    return TAHOE_OK;
}

tahoe_status tahoe_forest_set_profiling(tahoe_forest *f, int max_launches)
{
    if (!f || max_launches < 0 || max_launches > 4096) return fail(TAHOE_ERR_INVALID_ARG, "bad argument");
    while ((int)f->ev_start.size() < max_launches) {
        hipEvent_t a, b;
        TAHOE_HIP_TRY(hipEventCreate(&a));
        hipError_t e = hipEventCreate(&b);
        if (e != hipSuccess) {
            (void)hipEventDestroy(a);
            return fail(TAHOE_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e));
        }
        hipEvent_t m;
        e = hipEventCreate(&m);
        if (e != hipSuccess) {
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
            return fail(TAHOE_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e));
        }
        f->ev_start.push_back(a);
        f->ev_mid.push_back(m);
        f->ev_stop.push_back(b);
    }
    f->profiling = max_launches > 0;
    f->prof_count = 0;
    return TAHOE_OK;
}

tahoe_status tahoe_forest_kernel_times(tahoe_forest *f, float *ms_out, int capacity, int *count)
{
    if (!f || !count || (capacity > 0 && !ms_out)) return fail(TAHOE_ERR_INVALID_ARG, "null argument");
    const int n = (int)std::min<size_t>(f->prof_count, (size_t)std::max(capacity, 0));
    for (int i = 0; i < n; ++i) {
        TAHOE_HIP_TRY(hipEventSynchronize(f->ev_stop[i]));
        TAHOE_HIP_TRY(hipEventElapsedTime(&ms_out[i], f->ev_mid[i], f->ev_stop[i]));
    }
    *count = n;
    return TAHOE_OK;
}

tahoe_status tahoe_forest_prepass_times(tahoe_forest *f, float *ms_out, int capacity, int *count)
{
    if (!f || !count || (capacity > 0 && !ms_out)) return fail(TAHOE_ERR_INVALID_ARG, "null argument");
    const int n = (int)std::min<size_t>(f->prof_count, (size_t)std::max(capacity, 0));
    for (int i = 0; i < n; ++i) {
        TAHOE_HIP_TRY(hipEventSynchronize(f->ev_mid[i]));
        TAHOE_HIP_TRY(hipEventElapsedTime(&ms_out[i], f->ev_start[i], f->ev_mid[i]));
    }
    *count = n;
    return TAHOE_OK;
}

}  // extern "C"
