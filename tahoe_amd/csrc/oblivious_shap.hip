// TreeSHAP and Saabas contributions on an oblivious handle (tahoe_oblivious_forest_create_ex with TAHOE_CREATE_CONTRIBS /
// TAHOE_CREATE_APPROX_CONTRIBS).  Handles with category sets run the CAT == true
// instantiations of the kernels below, which oblivious_shap_cat.hip compiles from this file's device code.
//
// Every leaf of an oblivious tree tests the same m <= D distinct features in the same order, the cover ratios of a leaf's path
// depend on (tree, leaf) alone, and a row follows the path's element of feature e exactly when its leaf index idx and the leaf j
// agree on that feature's levels: ((idx ^ j) & mask_e) == 0.  Both kernels are lane = row: one wave owns 64 rows, reads every
// table at wave-uniform addresses (scalar loads), and exchanges nothing between lanes.
//
// Tables, built once at create from the leaf covers (float64 on the host):
//   splits[sum D_t]       {thr, id | def_left << 31}; id = the feature's compact id over the features the forest uses (LDS form)
//                         or its column (in-place form).  A category set (tahoe_oblivious_forest_create_cat) keeps its kind bits
//                         and its word or pool index as the walk's record has them; the pool itself is the walk's, not a copy
//   used[U]               column of compact id c, ascending
//   elems[sum m_t]        {id, level mask} of tree t's distinct features in order of first appearance from level 0
//   zz[sum 2^D_t m_t]     {z, 1 - z} of (tree, leaf, element): z = the product of the cover ratios on the leaf's path over the
//                         element's levels, float64 rounded once (below kContribMinZ: 0), 1 - z from float64 beside it
//   zmask[sum 2^D_t]      the level masks of the leaf's elements with z == 0: a row that leaves the path there weighs the leaf 0
//   delta[sum 2 (2^D_t - 1)][K]  Saabas: (float)(E(child) - E(parent)) of the implicit heap's children, level by level
//   bias[K]               the bias column; div = (float)T with TAHOE_OUT_AVG, else 1
//
// Accumulators: a lane's (class, feature) sums live in its own row of an LDS slab of odd stride (conflict-free both when the 64
// lanes add to one feature and when they write whole rows out), or, where the row tile and the slab do not fit the LDS, in the
// lane's own row of phi_dev.  Classes run in blocks of kObShapClasses over gridDim.y.
//
// Sum order, in every form and for any batch: phi[row][k][f] is the float32 sum from +0.0f, trees ascending, within a tree the
// leaves ascending that the row weighs (TreeSHAP; a leaf the row weighs 0 adds nothing) or the levels ascending (Saabas); then
// one division by div.  No atomics.
//
// SHAP interaction values (TAHOE_CREATE_INTERACTIONS): oblivious_inter_kernel, lane = row as above, the
// accumulators in place in the lane's own (F + 1) x (F + 1) matrices of out_dev, the features read from global memory.  It reads
// elems, zz and zmask as they are, through copies of splits and elems that hold columns whatever the form of the other kernels.
//   begin   the wave zeroes its rows' matrices (coalesced), then a barrier; afterwards a lane touches its own matrices only.
//   tree    of m distinct features (m == 0: nothing):
//     phi   ob_shap_tree<m> as it stands, its accumulators row F of the lane's matrix: predict_contribs' sums.
//     pairs (m >= 2) for c = 0 .. m - 2, the conditioned element: the reduced path holds the other R = m - 1 elements in their
//           order, position p = element e = p + (p >= c).  The sums of the pairs (c, e), e > c -- positions p >= c -- come
//           from M[lo][hi] (lo < hi the two columns) into registers, take one add per leaf the row weighs, leaves ascending,
//           and go back.  Per such leaf j, with mism = idx ^ j, o_e = (mism & mask_e) == 0 and {z_e, 1 - z_e} = zz[j][e]:
//             cf = (o_c ? 1 - z_c : -z_c) * 0.5f
//             EXTEND over the R positions: ob_shap_tree's loop with R for M
//             S0' = sum_{i < R} pw[i] * (float)((R + 1) / (R - i)), i ascending from +0.0f
//             per p >= c: tot = ob_shap_tree's unwound sum with R for M and z_e;  w = o_e ? tot * (1 - z_e) : -S0'
//               per class: sum = sum + (w * cf) * leaf[j][k]
//           Every coefficient is a float64 quotient rounded once, every product and sum one float32 operation.
//   end     per lane and class, over the used columns u[0] < u[1] < ...: M[a][b] = M[b][a] = M[a][b] / div for a < b; then per
//           used column a: S = +0.0f + M[a][b] for b != a ascending, M[a][a] = M[F][a] / div - S; then row F becomes +0.0f and
//           M[F][F] = bias[k].  Everything else keeps the +0.0f of the begin.
//
// Interventional TreeSHAP (TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL): oblivious_iv_kernel, lane = row, the
// accumulators and the begin / end of oblivious_shap_kernel.  A background row r enters tree t only through its leaf index R, so
// tahoe_forest_set_background keeps per tree the occupied leaves, ascending, with their integer counts (occ, occ_off) -- not the rows.
//   tree    of m distinct features (m == 0: nothing), X the row's leaf index; per occupied leaf {R, count}, in order:
//             diff = X ^ R;  dU = the elements e with diff & mask_e != 0 (the players), u = popcount(dU);  u == 0: no term
//             cf = (float)count
//             per submask sub of dU, in descending numeric order from dU itself down to 0 (sub = (sub - 1) & dU), s = popcount(sub):
//               j = R ^ (diff & OR_{e in sub} mask_e)            the live leaf: x's bits on the levels of sub, r's elsewhere
//               per e in dU, e ascending:  w = e in sub ? W+[u][s] : -W-[u][s]
//                 per class: sum = sum + (w * cf) * leaf[j][k]
//           W+[u][s] = (s - 1)! (u - s)! / u!, W-[u][s] = s! (u - s - 1)! / u!: float64 quotients rounded once, 17 x 17 each, in LDS.
//           The lanes of a wave differ in dU; the submask loop runs until the wave's last lane is through.
//   end     every used column / (float)B, then ob_shap_end: / div and the bias column of the background.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <type_traits>
#include <vector>

#include "contribs_internal.h"
#include "oblivious_internal.h"

namespace tahoe {

constexpr int kObShapClasses = 4;  // classes of one grid.y block: 16 x 4 accumulators in VGPRs at m = 16, (1 + 4) U x 256 B of LDS

// What the kernels read, by value in the kernel arguments
struct ObShapView {
    const InnerNode *splits;
    const int32_t *split_off;
    const int64_t *leaf_off;
    const float *leaves;
    const int32_t *used;
    const uint2 *elems;
    const int32_t *elem_off;
    const float2 *zz;
    const int64_t *zz_off;
    const uint32_t *zmask;
    const float *delta;
    const float *bias;
    float div, missing;
    int F, K, T, U, S;  // columns, leaf dimension, trees, used features, floats per slab row (odd)
};
// ... as a kernel argument: on a handle with category sets the walk's pool (shared, not copied; null: no pooled set) and its length
// in words ride behind it, and a handle without sets passes what it always passed
struct ObShapCatView : ObShapView {
    const uint32_t *cat_pool;
    uint32_t cat_words;
};
template <bool CAT>
using ObCatView = std::conditional_t<CAT, ObShapCatView, ObShapView>;
template <bool CAT>
inline ObCatView<CAT> ob_cat_view(const ObShapView &v, const uint32_t *cat_pool, uint32_t cat_words)
{
    ObCatView<CAT> c;
    static_cast<ObShapView &>(c) = v;
    if constexpr (CAT) {
        c.cat_pool = cat_pool;
        c.cat_words = cat_words;
    }
    return c;
}

constexpr int kObIvW = 17;                        // u and s run over 0 .. 16
constexpr int kObIvTable = 2 * kObIvW * kObIvW;   // floats of W+ | W-

// What oblivious_iv_kernel reads beside the view: the background of tahoe_forest_set_background and the weight tables
struct ObIvView {
    const uint2 *occ;         // {leaf, count} of every occupied (tree, leaf), tree-major, leaves ascending
    const int32_t *occ_off;   // [T + 1]
    const float *wtab;        // [kObIvTable]
    float fB;                 // (float)background rows
};



// One wave's 64 rows and their accumulators for the classes [k0, k0 + kb) of this grid.y block
template <int KB, bool INPLACE>
struct ObShapRows {
    int lane, nr, k0, kb;
    size_t row0, F1, out_row;
    bool row_ok;
    const float *x;  // INPLACE: the lane's row
    float *tile;     // else the 64 rows' used features, [U][64]
    float *slab;     // ... and the accumulators, [64][S]
    float *acc;      // the lane's accumulator of (class k0 + k, id) is acc[k * kstride + id]
    size_t kstride;
    __device__ __forceinline__ float feature(uint32_t id) const { return INPLACE ? x[id] : tile[id * 64u + (uint32_t)lane]; }
    __device__ __forceinline__ float load(int k, uint32_t id) const
    {
        return (!INPLACE || row_ok) ? acc[(size_t)k * kstride + id] : 0.0f;
    }
    __device__ __forceinline__ void store(int k, uint32_t id, float v) const
    {
        if (!INPLACE || row_ok) acc[(size_t)k * kstride + id] = v;
    }
};

// Zeroes the block's part of phi (every column: the ones no tree uses stay 0), stages the row tile and zeroes the slab
template <int KB, bool INPLACE>
__device__ __forceinline__ ObShapRows<KB, INPLACE> ob_shap_begin(const ObShapView &v, float *__restrict__ phi,
                                                                 const float *__restrict__ data, size_t rows, float *smem)
{
    ObShapRows<KB, INPLACE> r;
    r.lane = (int)threadIdx.x;
    r.row0 = (size_t)blockIdx.x * 64;
    const size_t row = r.row0 + (size_t)r.lane;
    r.row_ok = row < rows;
    r.nr = (int)std::min<size_t>(64, rows - r.row0);
    r.k0 = (int)blockIdx.y * KB;
    r.kb = std::min(KB, v.K - r.k0);
    r.F1 = (size_t)v.F + 1;
    r.out_row = (size_t)v.K * r.F1;
    for (int q = 0; q < r.nr; ++q)
        for (int k = 0; k < r.kb; ++k) {
            float *o = phi + (r.row0 + (size_t)q) * r.out_row + (size_t)(r.k0 + k) * r.F1;
            for (int i = r.lane; i < v.F; i += 64) o[i] = 0.0f;
        }
    const size_t my = r.row_ok ? row : r.row0;  // (a lane past the batch works on the tile's first row and stores nothing)
    const float *src = data + my * (size_t)v.F;
    r.x = src;
    r.tile = smem;
    r.slab = smem + (size_t)v.U * 64;
    if (INPLACE) {
        r.acc = phi + my * r.out_row + (size_t)r.k0 * r.F1;
        r.kstride = r.F1;
    } else {
        for (int c = 0; c < v.U; ++c) r.tile[c * 64 + r.lane] = src[v.used[c]];
        r.acc = r.slab + (size_t)r.lane * (size_t)v.S;
        r.kstride = (size_t)v.U;
        for (int i = 0; i < r.kb * v.U; ++i) r.acc[i] = 0.0f;
    }
    __syncthreads();  // the zeroes land before any lane adds to its row or writes a used column
    return r;
}

// The used columns of every row out (the AVG division) and the bias column
template <int KB, bool INPLACE>
__device__ __forceinline__ void ob_shap_end(const ObShapView &v, const ObShapRows<KB, INPLACE> &r, float *__restrict__ phi)
{
    __syncthreads();
    for (int q = 0; q < r.nr; ++q)
        for (int k = 0; k < r.kb; ++k) {
            float *o = phi + (r.row0 + (size_t)q) * r.out_row + (size_t)(r.k0 + k) * r.F1;
            const float *s = r.slab + (size_t)q * (size_t)v.S + (size_t)k * (size_t)v.U;
            for (int c = r.lane; c < v.U; c += 64) {
                const int fid = v.used[c];
                const float sum = INPLACE ? o[fid] : s[c];
                o[fid] = sum / v.div;
            }
            if (r.lane == 0) o[v.F] = v.bias[r.k0 + k];
        }
}

// The row's leaf index of tree t (level 0 = bit 0), as oblivious_walk computes it; each(l, id, idx) after level l's bit is in.
// This is the only place where an explanation kernel sees the row, so a category set (a record with kObCat, a wave-uniform
// branch in ob_split_bit) changes nothing else: no table holds a threshold.  CAT == false is the code of a handle without sets:
// every kernel is instantiated for both, because the branch taken at run time on every handle cost a numeric handle up to a
// quarter of its Saabas time.
template <bool CAT, class Rows, class Each>
__device__ __forceinline__ uint32_t ob_shap_leaf_index(const ObCatView<CAT> &v, const Rows &r, int t, Each &&each)
{
    const uint32_t *cat_pool = nullptr;
    uint32_t cat_words = 0;
    if constexpr (CAT) {
        cat_pool = v.cat_pool;
        cat_words = v.cat_words;
    }
    const int s0 = v.split_off[t];
    const int d = v.split_off[t + 1] - s0;
    uint32_t idx = 0;
    for (int l = 0; l < d; ++l) {
        const InnerNode n = v.splits[s0 + l];
        const uint32_t id = CAT ? ob_split_fid(n.meta) : n.meta & kMetaFidMask;
        idx |= ob_split_bit<CAT>(n, r.feature(id), v.missing, cat_pool, cat_words) << l;
        each(l, id, idx);
    }
    return idx;
}

// One tree of M distinct features: the running sums of its features come into VGPRs, take the terms of the leaves in order, and
// go back.  pw[] is indexed by unrolled loops only, so it stays in registers.  Per leaf, with z_e and o_e in {0, 1} of element e:
//   EXTEND over the M elements (Lundberg et al. 2018, Algorithm 2), then per element the unwound sum:
//     o_e = 1: the recurrence over pw with z_e;  the term is sum (1 - z_e) leaf
//     o_e = 0: sum = S0 / z_e with S0 = sum_i pw[i] (M + 1) / (M - i) the same for every element, so the term sum (0 - z_e) leaf
//              is -S0 leaf and the division is never made
//   A leaf with z_e == 0 and o_e == 0 for some e has path weight 0 and is skipped (by the wave when no lane weighs it).
template <int M, int KB, bool INPLACE>
__device__ __forceinline__ void ob_shap_tree(const ObShapRows<KB, INPLACE> &r, const uint2 *__restrict__ el,
                                             const float2 *__restrict__ zz, const uint32_t *__restrict__ zmask,
                                             const float *__restrict__ lv, int nleaf, uint32_t idx, int K)
{
    uint32_t id[M], mask[M];
    float a[M][KB];
#pragma unroll
    for (int e = 0; e < M; ++e) {
        id[e] = el[e].x;
        mask[e] = el[e].y;
#pragma unroll
        for (int k = 0; k < KB; ++k) a[e][k] = (KB == 1 || k < r.kb) ? r.load(k, id[e]) : 0.0f;
    }
    for (int j = 0; j < nleaf; ++j) {
        const uint32_t mism = idx ^ (uint32_t)j;
        const bool live = (mism & zmask[j]) == 0u;
        if (__ballot(live) == 0ull) continue;
        const float2 *zj = zz + (size_t)j * M;
        float pw[M + 1], z[M], omz[M];
        bool o[M];
        pw[0] = 1.0f;
#pragma unroll
        for (int e = 0; e < M; ++e) {
            const int l = e + 1;
            const float2 zo = zj[e];
            z[e] = zo.x;
            omz[e] = zo.y;
            o[e] = (mism & mask[e]) == 0u;
            pw[l] = 0.0f;
#pragma unroll
            for (int i = l - 1; i >= 0; --i) {
                const float t = pw[i] * (float)((double)(i + 1) / (double)(l + 1));
                pw[i + 1] = pw[i + 1] + (o[e] ? t : 0.0f);
                pw[i] = pw[i] * (z[e] * (float)((double)(l - i) / (double)(l + 1)));
            }
        }
        float s0 = 0.0f;
#pragma unroll
        for (int i = 0; i < M; ++i) s0 = s0 + pw[i] * (float)((double)(M + 1) / (double)(M - i));
        const float *lj = lv + (size_t)j * (size_t)K;
#pragma unroll
        for (int e = 0; e < M; ++e) {
            float nxt = pw[M], tot = 0.0f;
#pragma unroll
            for (int i = M - 1; i >= 0; --i) {
                const float tmp = nxt * (float)((double)(M + 1) / (double)(i + 1));
                tot = tot + tmp;
                if (i > 0) nxt = pw[i] - tmp * (z[e] * (float)((double)(M - i) / (double)(M + 1)));
            }
            const float w = o[e] ? tot * omz[e] : -s0;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const float leaf = (KB == 1 || k < r.kb) ? lj[k] : 0.0f;
                const float sum = a[e][k] + w * leaf;
                a[e][k] = live ? sum : a[e][k];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < M; ++e)
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (KB == 1 || k < r.kb) r.store(k, id[e], a[e][k]);
}

// TreeSHAP: grid (row tiles, class blocks), one wave per workgroup.  Dynamic LDS (not INPLACE): [U][64] tile | [64][S] slab.
template <int KB, bool INPLACE, bool CAT = false>
__global__ void __launch_bounds__(64) oblivious_shap_kernel(const ObCatView<CAT> v, float *__restrict__ phi,
                                                            const float *__restrict__ data, size_t rows)
{
    extern __shared__ __attribute__((aligned(16))) float ob_shap_smem[];
    const ObShapRows<KB, INPLACE> r = ob_shap_begin<KB, INPLACE>(v, phi, data, rows, ob_shap_smem);
    for (int t = 0; t < v.T; ++t) {
        const int e0 = v.elem_off[t];
        const int m = v.elem_off[t + 1] - e0;  // wave-uniform, as everything read below
        if (m == 0) continue;                  // a single leaf: all of it is bias
        const uint32_t idx = ob_shap_leaf_index<CAT>(v, r, t, [](int, uint32_t, uint32_t) {});
        const int nleaf = 1 << (v.split_off[t + 1] - v.split_off[t]);
        const uint2 *el = v.elems + e0;
        const float2 *zz = v.zz + v.zz_off[t];
        const uint32_t *zm = v.zmask + v.leaf_off[t];
        const float *lv = v.leaves + (size_t)v.leaf_off[t] * (size_t)v.K + r.k0;
        switch (m) {
#define TAHOE_OB_SHAP_CASE(M) \
    case M: ob_shap_tree<M, KB, INPLACE>(r, el, zz, zm, lv, nleaf, idx, v.K); break;
            TAHOE_OB_SHAP_CASE(1) TAHOE_OB_SHAP_CASE(2) TAHOE_OB_SHAP_CASE(3) TAHOE_OB_SHAP_CASE(4)
            TAHOE_OB_SHAP_CASE(5) TAHOE_OB_SHAP_CASE(6) TAHOE_OB_SHAP_CASE(7) TAHOE_OB_SHAP_CASE(8)
            TAHOE_OB_SHAP_CASE(9) TAHOE_OB_SHAP_CASE(10) TAHOE_OB_SHAP_CASE(11) TAHOE_OB_SHAP_CASE(12)
            TAHOE_OB_SHAP_CASE(13) TAHOE_OB_SHAP_CASE(14) TAHOE_OB_SHAP_CASE(15) TAHOE_OB_SHAP_CASE(16)
#undef TAHOE_OB_SHAP_CASE
        default: break;
        }
    }
    ob_shap_end<KB, INPLACE>(v, r, phi);
}

// Saabas: the walk of oblivious_walk with one add per level -- the taken child's delta to the level's feature
template <int KB, bool INPLACE, bool CAT = false>
__global__ void __launch_bounds__(64) oblivious_approx_kernel(const ObCatView<CAT> v, float *__restrict__ phi,
                                                              const float *__restrict__ data, size_t rows)
{
    extern __shared__ __attribute__((aligned(16))) float ob_shap_smem[];
    const ObShapRows<KB, INPLACE> r = ob_shap_begin<KB, INPLACE>(v, phi, data, rows, ob_shap_smem);
    for (int t = 0; t < v.T; ++t) {
        // children of level l start at 2^(l + 1) - 2 of the tree's deltas; the child's index is the leaf index so far
        const float *dt = v.delta + (size_t)(2 * (v.leaf_off[t] - t)) * (size_t)v.K + r.k0;
        ob_shap_leaf_index<CAT>(v, r, t, [&](int l, uint32_t id, uint32_t idx) {
            const float *d = dt + (size_t)((2u << l) - 2u + idx) * (size_t)v.K;
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (KB == 1 || k < r.kb) r.store(k, id, r.load(k, id) + d[k]);
        });
    }
    ob_shap_end<KB, INPLACE>(v, r, phi);
}

// The pairs of one tree of M >= 2 distinct features (the file's header: "pairs").  mat: the lane's matrix of class r.k0, the next
// class mat_k floats on.  The conditioned element c is a wave-uniform loop; pw, z, o and a are indexed by unrolled loops only.
template <int M, int KB>
__device__ __forceinline__ void ob_inter_tree(const ObShapRows<KB, true> &r, float *__restrict__ mat, size_t mat_k,
                                              const uint2 *__restrict__ el, const float2 *__restrict__ zz,
                                              const uint32_t *__restrict__ zmask, const float *__restrict__ lv, int nleaf,
                                              uint32_t idx, int K)
{
    constexpr int R = M - 1;
    for (int c = 0; c < R; ++c) {
        const uint32_t idc = el[c].x, maskc = el[c].y;
        // M[lo][hi] of the pair (c, element at position p)
        auto at = [&](int p) {
            const uint32_t ide = el[p + (p >= c ? 1 : 0)].x;
            return (size_t)std::min(idc, ide) * r.F1 + (size_t)std::max(idc, ide);
        };
        uint32_t mask[R];
        float a[R][KB];
#pragma unroll
        for (int p = 0; p < R; ++p) {
            mask[p] = el[p + (p >= c ? 1 : 0)].y;
#pragma unroll
            for (int k = 0; k < KB; ++k)
                a[p][k] = (p >= c && (KB == 1 || k < r.kb) && r.row_ok) ? mat[(size_t)k * mat_k + at(p)] : 0.0f;
        }
        for (int j = 0; j < nleaf; ++j) {
            const uint32_t mism = idx ^ (uint32_t)j;
            const bool live = (mism & zmask[j]) == 0u;
            if (__ballot(live) == 0ull) continue;
            const float2 *zj = zz + (size_t)j * M;
            const float2 zc = zj[c];
            const float cf = ((mism & maskc) == 0u ? zc.y : -zc.x) * 0.5f;
            float pw[R + 1], z[R], omz[R];
            bool o[R];
            pw[0] = 1.0f;
#pragma unroll
            for (int p = 0; p < R; ++p) {
                const int l = p + 1;
                const float2 zo = zj[p + (p >= c ? 1 : 0)];
                z[p] = zo.x;
                omz[p] = zo.y;
                o[p] = (mism & mask[p]) == 0u;
                pw[l] = 0.0f;
#pragma unroll
                for (int i = l - 1; i >= 0; --i) {
                    const float t = pw[i] * (float)((double)(i + 1) / (double)(l + 1));
                    pw[i + 1] = pw[i + 1] + (o[p] ? t : 0.0f);
                    pw[i] = pw[i] * (z[p] * (float)((double)(l - i) / (double)(l + 1)));
                }
            }
            float s0 = 0.0f;
#pragma unroll
            for (int i = 0; i < R; ++i) s0 = s0 + pw[i] * (float)((double)(R + 1) / (double)(R - i));
            const float *lj = lv + (size_t)j * (size_t)K;
#pragma unroll
            for (int p = 0; p < R; ++p) {
                if (p < c) continue;
                float nxt = pw[R], tot = 0.0f;
#pragma unroll
                for (int i = R - 1; i >= 0; --i) {
                    const float tmp = nxt * (float)((double)(R + 1) / (double)(i + 1));
                    tot = tot + tmp;
                    if (i > 0) nxt = pw[i] - tmp * (z[p] * (float)((double)(R - i) / (double)(R + 1)));
                }
                const float w = o[p] ? tot * omz[p] : -s0;
                const float wc = w * cf;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    const float leaf = (KB == 1 || k < r.kb) ? lj[k] : 0.0f;
                    const float sum = a[p][k] + wc * leaf;
                    a[p][k] = live ? sum : a[p][k];
                }
            }
        }
#pragma unroll
        for (int p = 0; p < R; ++p)
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (p >= c && (KB == 1 || k < r.kb) && r.row_ok) mat[(size_t)k * mat_k + at(p)] = a[p][k];
    }
}

// SHAP interaction values: grid (row tiles, class blocks), one wave per workgroup, no LDS.  v holds columns in splits and elems.
template <int KB, bool CAT = false>
__global__ void __launch_bounds__(64) oblivious_inter_kernel(const ObCatView<CAT> vin, float *__restrict__ out,
                                                             const float *__restrict__ data, size_t rows)
{
    // The view's pointers pass through an empty asm and are ordinary scalar values from here on.  As kernel-argument loads, which
    // the register allocator may repeat instead of spilling, a 16-dword group of them left a spill slot behind that no
    // instruction uses: 68 bytes of stack per lane in the resource table.  So: ScratchSize 0.
    ObCatView<CAT> v = vin;
    asm volatile("" : "+s"(v.splits), "+s"(v.split_off), "+s"(v.leaf_off), "+s"(v.leaves), "+s"(v.used), "+s"(v.elems), "+s"(v.elem_off),
                 "+s"(v.zz), "+s"(v.zz_off), "+s"(v.zmask), "+s"(v.bias));
    if constexpr (CAT) asm volatile("" : "+s"(v.cat_pool));
    ObShapRows<KB, true> r;
    r.lane = (int)threadIdx.x;
    r.row0 = (size_t)blockIdx.x * 64;
    const size_t row = r.row0 + (size_t)r.lane;
    r.row_ok = row < rows;
    r.nr = (int)std::min<size_t>(64, rows - r.row0);
    r.k0 = (int)blockIdx.y * KB;
    r.kb = std::min(KB, v.K - r.k0);
    r.F1 = (size_t)v.F + 1;
    const size_t mat_k = r.F1 * r.F1;
    r.out_row = (size_t)v.K * mat_k;
    for (int q = 0; q < r.nr; ++q) {  // the block's matrices of a row are contiguous
        float *o = out + (r.row0 + (size_t)q) * r.out_row + (size_t)r.k0 * mat_k;
        for (size_t i = (size_t)r.lane; i < (size_t)r.kb * mat_k; i += 64) o[i] = 0.0f;
    }
    const size_t my = r.row_ok ? row : r.row0;  // (a lane past the batch reads the tile's first row and neither loads nor stores)
    r.x = data + my * (size_t)v.F;
    r.tile = r.slab = nullptr;
    float *mat = out + my * r.out_row + (size_t)r.k0 * mat_k;
    r.acc = mat + (size_t)v.F * r.F1;  // phi accumulates in row F, which ends as zeroes
    r.kstride = mat_k;
    __syncthreads();  // the zeroes land before any lane adds to its matrices
    for (int t = 0; t < v.T; ++t) {
        const int e0 = v.elem_off[t];
        const int m = v.elem_off[t + 1] - e0;  // wave-uniform, as everything read below
        if (m == 0) continue;
        const uint32_t idx = ob_shap_leaf_index<CAT>(v, r, t, [](int, uint32_t, uint32_t) {});
        const int nleaf = 1 << (v.split_off[t + 1] - v.split_off[t]);
        const uint2 *el = v.elems + e0;
        const float2 *zz = v.zz + v.zz_off[t];
        const uint32_t *zm = v.zmask + v.leaf_off[t];
        const float *lv = v.leaves + (size_t)v.leaf_off[t] * (size_t)v.K + r.k0;
        switch (m) {
        case 1: ob_shap_tree<1, KB, true>(r, el, zz, zm, lv, nleaf, idx, v.K); break;  // no pair
#define TAHOE_OB_INTER_CASE(M) \
    case M: \
        ob_shap_tree<M, KB, true>(r, el, zz, zm, lv, nleaf, idx, v.K); \
        ob_inter_tree<M, KB>(r, mat, mat_k, el, zz, zm, lv, nleaf, idx, v.K); \
        break;
            TAHOE_OB_INTER_CASE(2) TAHOE_OB_INTER_CASE(3) TAHOE_OB_INTER_CASE(4) TAHOE_OB_INTER_CASE(5)
            TAHOE_OB_INTER_CASE(6) TAHOE_OB_INTER_CASE(7) TAHOE_OB_INTER_CASE(8) TAHOE_OB_INTER_CASE(9)
            TAHOE_OB_INTER_CASE(10) TAHOE_OB_INTER_CASE(11) TAHOE_OB_INTER_CASE(12) TAHOE_OB_INTER_CASE(13)
            TAHOE_OB_INTER_CASE(14) TAHOE_OB_INTER_CASE(15) TAHOE_OB_INTER_CASE(16)
#undef TAHOE_OB_INTER_CASE
        default: break;
        }
    }
    if (!r.row_ok) return;
    for (int k = 0; k < r.kb; ++k) {
        float *mk = mat + (size_t)k * mat_k;
        for (int a = 0; a < v.U; ++a)
            for (int b = a + 1; b < v.U; ++b) {
                const size_t fa = (size_t)v.used[a], fb = (size_t)v.used[b];
                const float q = mk[fa * r.F1 + fb] / v.div;
                mk[fa * r.F1 + fb] = q;
                mk[fb * r.F1 + fa] = q;
            }
        float *phi = mk + (size_t)v.F * r.F1;
        for (int a = 0; a < v.U; ++a) {
            const size_t fa = (size_t)v.used[a];
            float s = 0.0f;
            for (int b = 0; b < v.U; ++b)
                if (b != a) s = s + mk[fa * r.F1 + (size_t)v.used[b]];
            mk[fa * r.F1 + fa] = phi[fa] / v.div - s;
        }
        for (int a = 0; a < v.U; ++a) phi[v.used[a]] = 0.0f;
        phi[v.F] = v.bias[r.k0 + k];
    }
}

// Interventional TreeSHAP, one tree of M distinct features (the file's header: "tree").  a, id and mask as in ob_shap_tree; W is
// the LDS copy of the weight tables.  The occupancy entries sit at wave-uniform addresses; the leaf gather is per lane.
template <int M, int KB, bool INPLACE>
__device__ __forceinline__ void ob_iv_tree(const ObShapRows<KB, INPLACE> &r, const uint2 *__restrict__ el,
                                           const uint2 *__restrict__ occ, int nocc, const float *__restrict__ lv, uint32_t X, int K,
                                           const float *W)
{
    uint32_t id[M], mask[M];
    float a[M][KB];
#pragma unroll
    for (int e = 0; e < M; ++e) {
        id[e] = el[e].x;
        mask[e] = el[e].y;
#pragma unroll
        for (int k = 0; k < KB; ++k) a[e][k] = (KB == 1 || k < r.kb) ? r.load(k, id[e]) : 0.0f;
    }
    for (int q = 0; q < nocc; ++q) {
        const uint2 oc = occ[q];
        const uint32_t R = oc.x;
        const float cf = (float)oc.y;
        const uint32_t diff = X ^ R;
        uint32_t dU = 0u;
#pragma unroll
        for (int e = 0; e < M; ++e) dU |= (diff & mask[e]) != 0u ? 1u << e : 0u;
        const int u = __popc(dU);
        uint32_t sub = dU;
        bool act = dU != 0u;
        while (__ballot(act) != 0ull) {
            const int s = __popc(sub);
            uint32_t lm = 0u;
#pragma unroll
            for (int e = 0; e < M; ++e) lm |= (sub >> e & 1u) != 0u ? mask[e] : 0u;
            const uint32_t j = R ^ (diff & lm);  // < 2^D: R, diff and lm are
            const float wp = W[u * kObIvW + s] * cf;
            const float wm = -(W[kObIvW * kObIvW + u * kObIvW + s] * cf);
            const float *lj = lv + (size_t)j * (size_t)K;
            float leaf[KB];
#pragma unroll
            for (int k = 0; k < KB; ++k) leaf[k] = (KB == 1 || k < r.kb) ? lj[k] : 0.0f;
#pragma unroll
            for (int e = 0; e < M; ++e) {
                const float w = (sub >> e & 1u) != 0u ? wp : wm;
                const bool on = act && (dU >> e & 1u) != 0u;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    const float sum = a[e][k] + w * leaf[k];
                    a[e][k] = on ? sum : a[e][k];
                }
            }
            act = act && sub != 0u;
            sub = (sub - 1u) & dU;
        }
    }
#pragma unroll
    for (int e = 0; e < M; ++e)
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (KB == 1 || k < r.kb) r.store(k, id[e], a[e][k]);
}

// Interventional TreeSHAP: grid (row tiles, class blocks), one wave per workgroup.  Dynamic LDS: (not INPLACE) [U][64] tile |
// [64][S] slab, then [kObIvTable] weights.  v.bias is the bias column of the background.
template <int KB, bool INPLACE, bool CAT = false>
__global__ void __launch_bounds__(64) oblivious_iv_kernel(const ObCatView<CAT> v, const ObIvView b, float *__restrict__ phi,
                                                          const float *__restrict__ data, size_t rows)
{
    extern __shared__ __attribute__((aligned(16))) float ob_shap_smem[];
    float *W = ob_shap_smem + (INPLACE ? 0 : (v.U + v.S) * 64);
    for (int i = (int)threadIdx.x; i < kObIvTable; i += 64) W[i] = b.wtab[i];
    const ObShapRows<KB, INPLACE> r = ob_shap_begin<KB, INPLACE>(v, phi, data, rows, ob_shap_smem);  // (its barrier)
    for (int t = 0; t < v.T; ++t) {
        const int e0 = v.elem_off[t];
        const int m = v.elem_off[t + 1] - e0;  // wave-uniform, as everything read below but the leaves
        if (m == 0) continue;                  // a single leaf: all of it is bias
        const uint32_t idx = ob_shap_leaf_index<CAT>(v, r, t, [](int, uint32_t, uint32_t) {});
        const uint2 *el = v.elems + e0;
        const int o0 = b.occ_off[t];
        const int nocc = b.occ_off[t + 1] - o0;
        const uint2 *oc = b.occ + o0;
        const float *lv = v.leaves + (size_t)v.leaf_off[t] * (size_t)v.K + r.k0;
        switch (m) {
#define TAHOE_OB_IV_CASE(M) \
    case M: ob_iv_tree<M, KB, INPLACE>(r, el, oc, nocc, lv, idx, v.K, W); break;
            TAHOE_OB_IV_CASE(1) TAHOE_OB_IV_CASE(2) TAHOE_OB_IV_CASE(3) TAHOE_OB_IV_CASE(4)
            TAHOE_OB_IV_CASE(5) TAHOE_OB_IV_CASE(6) TAHOE_OB_IV_CASE(7) TAHOE_OB_IV_CASE(8)
            TAHOE_OB_IV_CASE(9) TAHOE_OB_IV_CASE(10) TAHOE_OB_IV_CASE(11) TAHOE_OB_IV_CASE(12)
            TAHOE_OB_IV_CASE(13) TAHOE_OB_IV_CASE(14) TAHOE_OB_IV_CASE(15) TAHOE_OB_IV_CASE(16)
#undef TAHOE_OB_IV_CASE
        default: break;
        }
    }
    // the mean over the background: the lane's own sums of the used columns, before ob_shap_end's division by div
    for (int c = 0; c < v.U; ++c) {
        const uint32_t id = INPLACE ? (uint32_t)v.used[c] : (uint32_t)c;
        for (int k = 0; k < r.kb; ++k) r.store(k, id, r.load(k, id) / b.fB);
    }
    ob_shap_end<KB, INPLACE>(v, r, phi);
}

// ---- launches.  Each translation unit instantiates its own CAT; K == 1 takes the single-class kernels. ----
template <class Fn>
inline void ob_with_classes_and_form(int K, bool inplace, Fn &&fn)
{
    auto with_form = [&](auto kb) {
        if (inplace) fn(kb, std::true_type{});
        else fn(kb, std::false_type{});
    };
    if (K == 1) with_form(std::integral_constant<int, 1>{});
    else with_form(std::integral_constant<int, kObShapClasses>{});
}

// TreeSHAP (flag == TAHOE_CREATE_CONTRIBS) or Saabas
template <bool CAT>
void ob_launch_shap(unsigned flag, int K, bool inplace, dim3 grid, size_t lds_bytes, hipStream_t stream, const ObShapView &view,
                    const uint32_t *cat_pool, uint32_t cat_words, float *phi_dev, const float *data_dev, size_t rows)
{
    const ObCatView<CAT> v = ob_cat_view<CAT>(view, cat_pool, cat_words);
    ob_with_classes_and_form(K, inplace, [&](auto kb, auto ip) {
        constexpr int KB = decltype(kb)::value;
        constexpr bool IP = decltype(ip)::value;
        if (flag == TAHOE_CREATE_CONTRIBS)
            hipLaunchKernelGGL((oblivious_shap_kernel<KB, IP, CAT>), grid, dim3(64), lds_bytes, stream, v, phi_dev, data_dev, rows);
        else
            hipLaunchKernelGGL((oblivious_approx_kernel<KB, IP, CAT>), grid, dim3(64), lds_bytes, stream, v, phi_dev, data_dev, rows);
    });
}

template <bool CAT>
void ob_launch_iv(int K, bool inplace, dim3 grid, size_t lds_bytes, hipStream_t stream, const ObShapView &view,
                  const uint32_t *cat_pool, uint32_t cat_words, const ObIvView &b, float *phi_dev, const float *data_dev, size_t rows)
{
    const ObCatView<CAT> v = ob_cat_view<CAT>(view, cat_pool, cat_words);
    ob_with_classes_and_form(K, inplace, [&](auto kb, auto ip) {
        hipLaunchKernelGGL((oblivious_iv_kernel<decltype(kb)::value, decltype(ip)::value, CAT>), grid, dim3(64), lds_bytes, stream, v, b,
                           phi_dev, data_dev, rows);
    });
}

// The LDS forms may need more than the default 64 KiB: those of TreeSHAP and Saabas, or (iv) of the interventional kernel
template <bool CAT>
hipError_t ob_allow_lds(bool iv, int limit)
{
    hipError_t e = hipSuccess;
    if (iv) {
        if ((e = allow_max_lds(reinterpret_cast<const void *>(&oblivious_iv_kernel<1, false, CAT>), limit)) != hipSuccess) return e;
        return allow_max_lds(reinterpret_cast<const void *>(&oblivious_iv_kernel<kObShapClasses, false, CAT>), limit);
    }
    if ((e = allow_max_lds(reinterpret_cast<const void *>(&oblivious_shap_kernel<1, false, CAT>), limit)) != hipSuccess ||
        (e = allow_max_lds(reinterpret_cast<const void *>(&oblivious_shap_kernel<kObShapClasses, false, CAT>), limit)) != hipSuccess ||
        (e = allow_max_lds(reinterpret_cast<const void *>(&oblivious_approx_kernel<1, false, CAT>), limit)) != hipSuccess)
        return e;
    return allow_max_lds(reinterpret_cast<const void *>(&oblivious_approx_kernel<kObShapClasses, false, CAT>), limit);
}

// CAT == true lives in oblivious_shap_cat.hip, which compiles this file's device code with TAHOE_OBLIVIOUS_SHAP_CAT_UNIT defined, so
// that the two halves of the kernels build side by side
extern template void ob_launch_shap<true>(unsigned, int, bool, dim3, size_t, hipStream_t, const ObShapView &, const uint32_t *, uint32_t,
                                          float *, const float *, size_t);
void ob_launch_inter_cat(int K, dim3 grid, hipStream_t stream, const ObShapView &view, const uint32_t *cat_pool, uint32_t cat_words,
                         float *out_dev, const float *data_dev, size_t rows);
extern template void ob_launch_iv<true>(int, bool, dim3, size_t, hipStream_t, const ObShapView &, const uint32_t *, uint32_t,
                                        const ObIvView &, float *, const float *, size_t);
extern template hipError_t ob_allow_lds<true>(bool, int);

#ifdef TAHOE_OBLIVIOUS_SHAP_CAT_UNIT
template void ob_launch_shap<true>(unsigned, int, bool, dim3, size_t, hipStream_t, const ObShapView &, const uint32_t *, uint32_t,
                                   float *, const float *, size_t);
template void ob_launch_iv<true>(int, bool, dim3, size_t, hipStream_t, const ObShapView &, const uint32_t *, uint32_t, const ObIvView &,
                                 float *, const float *, size_t);
template hipError_t ob_allow_lds<true>(bool, int);

void ob_launch_inter_cat(int K, dim3 grid, hipStream_t stream, const ObShapView &view, const uint32_t *cat_pool, uint32_t cat_words,
                         float *out_dev, const float *data_dev, size_t rows)
{
    const ObCatView<true> v = ob_cat_view<true>(view, cat_pool, cat_words);
    if (K == 1) hipLaunchKernelGGL((oblivious_inter_kernel<1, true>), grid, dim3(64), 0, stream, v, out_dev, data_dev, rows);
    else hipLaunchKernelGGL((oblivious_inter_kernel<kObShapClasses, true>), grid, dim3(64), 0, stream, v, out_dev, data_dev, rows);
}
#endif

}  // namespace tahoe

#ifndef TAHOE_OBLIVIOUS_SHAP_CAT_UNIT  // from here on: the tables and the entry points

struct tahoe_oshap {
    tahoe::InnerNode *splits = nullptr;
    int32_t *used = nullptr;
    uint2 *elems = nullptr;
    int32_t *elem_off = nullptr;
    float2 *zz = nullptr;
    int64_t *zz_off = nullptr;
    uint32_t *zmask = nullptr;
    float *delta = nullptr;
    float *bias = nullptr;
    tahoe::InnerNode *splits_col = nullptr;  // TAHOE_CREATE_INTERACTIONS: splits and elems with id = the column in either form
    uint2 *elems_col = nullptr;
    bool contribs = false, approx = false, inter = false;
    bool inplace = false;  // accumulate in phi_dev (else in LDS)
    size_t lds_bytes = 0;
    tahoe::ObShapView view{};
    tahoe::ObShapView inter_view{};  // view with splits_col and elems_col
    // TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL: the weight tables (create); the background (tahoe_forest_set_background): occupied
    // leaves, per-tree offsets, bias column
    bool iv = false;
    size_t iv_lds_bytes = 0;  // oblivious_iv_kernel: lds_bytes, then the weight tables
    float *wtab = nullptr;
    uint2 *occ = nullptr;
    int32_t *occ_off = nullptr;
    float *iv_bias = nullptr;
    size_t bg_rows = 0;   // 0: no background
    size_t bg_bytes = 0;  // device bytes of the three background buffers (counted in tahoe_forest::device_bytes)
};

namespace tahoe {

tahoe_status oblivious_shap_validate(const int32_t *depths, int num_trees, const float *leaf_covers)
{
    size_t at = 0;
    for (int t = 0; t < num_trees; ++t) {
        const size_t n = (size_t)1 << depths[t];
        for (size_t j = 0; j < n; ++j) {
            const float c = leaf_covers[at + j];
            if (!(c >= 0.0f) || std::isinf(c))
                return fail(TAHOE_ERR_INVALID_FOREST, "tahoe_oblivious_forest_create_ex: tree %d leaf %zu: cover %g is negative or "
                                                      "not finite", t, j, (double)c);
        }
        at += n;
    }
    return TAHOE_OK;
}

namespace {

// The cover ratios of one tree's implicit heap.  Level l has 2^l nodes, numbered by the l low bits of the leaf index (the
// decisions of levels 0 .. l - 1); the children of node p of level l are p (left) and p | 1 << l (right) of level l + 1.
struct ObHeap {
    int D = 0;
    std::vector<std::vector<double>> cover;  // [l][node]: float64 sum of the leaf covers below
    std::vector<std::vector<double>> ratio;  // [l][node], l >= 1: the share of its parent's mix; 1/2 under a node of cover 0
    void build(int depth, const float *leaf_covers)
    {
        D = depth;
        cover.assign((size_t)D + 1, {});
        ratio.assign((size_t)D + 1, {});
        cover[(size_t)D].assign(leaf_covers, leaf_covers + ((size_t)1 << D));
        for (int l = D - 1; l >= 0; --l) {
            const size_t n = (size_t)1 << l;
            cover[(size_t)l].resize(n);
            ratio[(size_t)l + 1].resize(2 * n);
            for (size_t p = 0; p < n; ++p) {
                const double wl = cover[(size_t)l + 1][p], wr = cover[(size_t)l + 1][p | n];
                cover[(size_t)l][p] = wl + wr;
                ratio[(size_t)l + 1][p] = wl + wr > 0.0 ? wl / (wl + wr) : 0.5;
                ratio[(size_t)l + 1][p | n] = wl + wr > 0.0 ? wr / (wl + wr) : 0.5;
            }
        }
    }
};

// The distinct features of a tree's D levels in order of first appearance from level 0, with their level masks; returns their number
int tree_elements(const InnerNode *ts, int D, uint32_t *fid, uint32_t *mask)
{
    int m = 0;
    for (int l = 0; l < D; ++l) {
        const uint32_t fl = ob_split_fid(ts[l].meta);
        int e = 0;
        while (e < m && fid[e] != fl) ++e;
        if (e == m) {
            fid[m] = fl;
            mask[m++] = 0u;
        }
        mask[e] |= 1u << l;
    }
    return m;
}

uint32_t bit_reverse(uint32_t p, int d)
{
    uint32_t r = 0;
    for (int b = 0; b < d; ++b) r |= ((p >> b) & 1u) << (d - 1 - b);
    return r;
}

}  // namespace

tahoe_status oblivious_shap_build(tahoe_forest *f, const ObliviousSource &src, unsigned flags)
{
    tahoe_ostate *o = f->ob;
    tahoe_oshap *sh = new (std::nothrow) tahoe_oshap();
    if (!sh) return fail(TAHOE_ERR_NO_MEMORY, "oblivious_shap_build");
    o->shap = sh;
    sh->contribs = (flags & TAHOE_CREATE_CONTRIBS) != 0;
    sh->approx = (flags & TAHOE_CREATE_APPROX_CONTRIBS) != 0;
    sh->inter = (flags & TAHOE_CREATE_INTERACTIONS) != 0;
    sh->iv = (flags & TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL) != 0;
    const bool paths = sh->contribs || sh->inter;  // elems, zz and zmask serve both
    const bool cover_tables = sh->contribs || sh->inter || sh->approx;  // (src.leaf_covers may be null without them)
    const int T = f->p.num_trees, K = f->num_classes, F = f->p.num_cols;
    const std::vector<InnerNode> &splits = *src.h_splits;
    const std::vector<int32_t> &split_off = *src.h_split_off;
    const std::vector<int64_t> &leaf_off = *src.h_leaf_off;

    // ---- the features the forest uses, and the form ----
    std::vector<int32_t> used;
    used.reserve(splits.size());
    for (const InnerNode &n : splits) used.push_back((int32_t)ob_split_fid(n.meta));
    std::sort(used.begin(), used.end());
    used.erase(std::unique(used.begin(), used.end()), used.end());
    const int U = (int)used.size();
    const int S = (std::min(K, kObShapClasses) * U) | 1;
    sh->lds_bytes = ((size_t)U + (size_t)S) * 64 * sizeof(float);
    // One form per handle (the ids of splits and elems follow it): with the interventional flag its weight tables must fit as well
    const size_t iv_table_bytes = sh->iv ? kObIvTable * sizeof(float) : 0;
    sh->inplace = sh->lds_bytes + iv_table_bytes > (size_t)f->lds_limit || f->knobs.oblivious_shap_inplace;  // TAHOE_OBLIVIOUS_SHAP_INPLACE
    if (sh->inplace) sh->lds_bytes = 0;
    auto id_of = [&](uint32_t fid) {
        return sh->inplace ? fid : (uint32_t)(std::lower_bound(used.begin(), used.end(), (int32_t)fid) - used.begin());
    };
    std::vector<InnerNode> h_splits(splits.size());
    for (size_t s = 0; s < splits.size(); ++s) {  // the id takes the fid's place; def_left, the kind bits and the set word / pool index stay
        const uint32_t fid = ob_split_fid(splits[s].meta);
        h_splits[s] = InnerNode{splits[s].thr, id_of(fid) | (splits[s].meta & ~fid)};
    }

    // ---- per tree: elements, zero fractions, deltas, E_t ----
    std::vector<uint2> h_elems;
    std::vector<int32_t> h_elem_off((size_t)T + 1, 0);
    std::vector<float2> h_zz;
    std::vector<int64_t> h_zz_off((size_t)T, 0);
    std::vector<uint32_t> h_zmask(paths ? src.num_leaves : 0, 0u);
    std::vector<uint2> h_elems_col;
    std::vector<float> h_delta(sh->approx ? 2 * (src.num_leaves - (size_t)T) * (size_t)K : 0, 0.0f);
    std::vector<double> bias_sum((size_t)K, 0.0);
    ObHeap heap;
    std::vector<std::vector<double>> E;  // node means of one class, [l][node]
    std::vector<double> prod, next;
    for (int t = 0; t < T; ++t) {
        const int D = src.depths[t];
        const size_t nleaf = (size_t)1 << D, lo = (size_t)leaf_off[(size_t)t];
        const InnerNode *ts = splits.data() + split_off[(size_t)t];
        if (!cover_tables) {  // TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL alone: the elements, and nothing that reads a cover
            uint32_t fid[kObMaxDepth], mask[kObMaxDepth];
            const int m = tree_elements(ts, D, fid, mask);
            for (int e = 0; e < m; ++e) h_elems.push_back(make_uint2(id_of(fid[e]), mask[e]));
            h_elem_off[(size_t)t + 1] = (int32_t)h_elems.size();
            continue;
        }
        heap.build(D, src.leaf_covers + lo);
        // E_t[k]: the leaves in heap order left to right (the leaf at heap position h is leaf bit_reverse(h)), each times the
        // product of its path's ratios multiplied root first -- tree_expect's sum on the heap expansion, operation for operation
        prod.assign(1, 1.0);
        for (int l = 0; l < D; ++l) {
            next.resize((size_t)2 << l);
            for (size_t q = 0; q < next.size(); ++q) next[q] = prod[q & (((size_t)1 << l) - 1)] * heap.ratio[(size_t)l + 1][q];
            prod.swap(next);
        }
        for (int k = 0; k < K; ++k) {
            double e = 0.0;
            for (size_t h = 0; h < nleaf; ++h) {
                const size_t j = bit_reverse((uint32_t)h, D);
                e += (double)src.leaf_values[(lo + j) * (size_t)K + (size_t)k] * prod[j];
            }
            bias_sum[(size_t)k] += e;
        }
        if (sh->approx) {
            float *dt = h_delta.data() + 2 * (lo - (size_t)t) * (size_t)K;
            E.resize((size_t)D + 1);
            for (int k = 0; k < K; ++k) {
                E[(size_t)D].resize(nleaf);
                for (size_t j = 0; j < nleaf; ++j) E[(size_t)D][j] = (double)src.leaf_values[(lo + j) * (size_t)K + (size_t)k];
                for (int l = D - 1; l >= 0; --l) {
                    const size_t n = (size_t)1 << l;
                    E[(size_t)l].resize(n);
                    for (size_t p = 0; p < n; ++p) {
                        const double wl = heap.cover[(size_t)l + 1][p], wr = heap.cover[(size_t)l + 1][p | n];
                        const double el = E[(size_t)l + 1][p], er = E[(size_t)l + 1][p | n];
                        const double e = wl + wr > 0.0 ? (wl * el + wr * er) / (wl + wr) : (el + er) / 2.0;
                        E[(size_t)l][p] = e;
                        dt[(2 * n - 2 + p) * (size_t)K + (size_t)k] = (float)(el - e);
                        dt[(2 * n - 2 + (p | n)) * (size_t)K + (size_t)k] = (float)(er - e);
                    }
                }
            }
        }
        if (paths || sh->iv) {
            uint32_t fid[kObMaxDepth], mask[kObMaxDepth];
            const int m = tree_elements(ts, D, fid, mask);
            for (int e = 0; e < m; ++e) h_elems.push_back(make_uint2(id_of(fid[e]), mask[e]));
            if (!paths) {
                h_elem_off[(size_t)t + 1] = (int32_t)h_elems.size();
                continue;
            }
            if (sh->inter)
                for (int e = 0; e < m; ++e) h_elems_col.push_back(make_uint2(fid[e], mask[e]));
            h_zz_off[(size_t)t] = (int64_t)h_zz.size();
            for (size_t j = 0; j < nleaf; ++j) {
                uint32_t zm = 0u;
                for (int e = 0; e < m; ++e) {
                    double z = 1.0;
                    for (int l = 0; l < D; ++l)
                        if (mask[e] >> l & 1u) z *= heap.ratio[(size_t)l + 1][j & (((size_t)2 << l) - 1)];
                    const float zf = z < kContribMinZ ? 0.0f : (float)z;  // the cut of contribs.hip's path tables
                    if (zf == 0.0f) zm |= mask[e];
                    h_zz.push_back(make_float2(zf, (float)(1.0 - z)));
                }
                h_zmask[lo + j] = zm;
            }
        }
        h_elem_off[(size_t)t + 1] = (int32_t)h_elems.size();
    }
    const bool avg = (f->p.output & TAHOE_OUT_AVG) != 0 && T > 0;
    std::vector<float> h_bias((size_t)K);
    for (int k = 0; k < K; ++k)
        h_bias[(size_t)k] = (float)((avg ? bias_sum[(size_t)k] / (double)T : bias_sum[(size_t)k]) + (double)f->p.global_bias);

    tahoe_status s = TAHOE_OK;
    if ((s = hip_status(upload(&sh->splits, h_splits, &f->device_bytes), "upload(shap splits)")) ||
        (s = hip_status(upload(&sh->used, used, &f->device_bytes), "upload(used)")) ||
        (s = hip_status(upload(&sh->elems, h_elems, &f->device_bytes), "upload(elems)")) ||
        (s = hip_status(upload(&sh->elem_off, h_elem_off, &f->device_bytes), "upload(elem_off)")) ||
        (s = hip_status(upload(&sh->zz, h_zz, &f->device_bytes), "upload(zz)")) ||
        (s = hip_status(upload(&sh->zz_off, h_zz_off, &f->device_bytes), "upload(zz_off)")) ||
        (s = hip_status(upload(&sh->zmask, h_zmask, &f->device_bytes), "upload(zmask)")) ||
        (s = hip_status(upload(&sh->delta, h_delta, &f->device_bytes), "upload(delta)")) ||
        (s = hip_status(upload(&sh->bias, h_bias, &f->device_bytes), "upload(bias)")))
        return s;
    if (sh->inter &&  // (src's splits hold columns)
        ((s = hip_status(upload(&sh->splits_col, splits, &f->device_bytes), "upload(interaction splits)")) ||
         (s = hip_status(upload(&sh->elems_col, h_elems_col, &f->device_bytes), "upload(interaction elems)"))))
        return s;
    sh->view = ObShapView{sh->splits, o->split_off, o->leaf_off, o->leaves, sh->used, sh->elems, sh->elem_off, sh->zz, sh->zz_off,
                          sh->zmask, sh->delta, sh->bias, avg ? (float)T : 1.0f, f->p.missing, F, K, T, U, S};
    sh->inter_view = sh->view;
    sh->inter_view.splits = sh->splits_col;
    sh->inter_view.elems = sh->elems_col;
    if (sh->iv) {
        // W+[u][s] = (s - 1)! (u - s)! / u! = 1 / (s C(u, s)) for 1 <= s <= u, W-[u][s] = s! (u - s - 1)! / u! = 1 / ((u - s) C(u, s))
        // for 0 <= s < u; C(u, s) is exact in float64 (<= C(16, 8)); 0 elsewhere
        std::vector<float> h_w((size_t)kObIvTable, 0.0f);
        for (int u = 1; u < kObIvW; ++u) {
            double binom = 1.0;  // C(u, s)
            for (int s = 0; s <= u; ++s) {
                if (s > 0) binom = binom * (double)(u - s + 1) / (double)s;
                if (s >= 1) h_w[(size_t)(u * kObIvW + s)] = (float)(1.0 / ((double)s * binom));
                if (s < u) h_w[(size_t)(kObIvW * kObIvW + u * kObIvW + s)] = (float)(1.0 / ((double)(u - s) * binom));
            }
        }
        if ((s = hip_status(upload(&sh->wtab, h_w, &f->device_bytes), "upload(interventional weights)"))) return s;
        sh->iv_lds_bytes = sh->lds_bytes + kObIvTable * sizeof(float);  // the tile and slab of the handle's form, then the tables
        if (!sh->inplace) {
            const hipError_t e = o->cats ? ob_allow_lds<true>(true, f->lds_limit) : ob_allow_lds<false>(true, f->lds_limit);
            if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(oblivious_iv)");
        }
    }
    if (!sh->inplace) {  // the LDS forms may need more than the default 64 KiB
        const hipError_t e = o->cats ? ob_allow_lds<true>(false, f->lds_limit) : ob_allow_lds<false>(false, f->lds_limit);
        if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(oblivious_shap)");
    }
    return TAHOE_OK;
}

void oblivious_shap_destroy(tahoe_forest *f)
{
    tahoe_oshap *sh = f->ob ? f->ob->shap : nullptr;
    if (!sh) return;
    for (void *p : {(void *)sh->splits, (void *)sh->used, (void *)sh->elems, (void *)sh->elem_off, (void *)sh->zz, (void *)sh->zz_off,
                    (void *)sh->zmask, (void *)sh->delta, (void *)sh->bias, (void *)sh->splits_col, (void *)sh->elems_col,
                    (void *)sh->wtab, (void *)sh->occ, (void *)sh->occ_off, (void *)sh->iv_bias})
        if (p) (void)hipFree(p);
    delete sh;
    f->ob->shap = nullptr;
}

bool oblivious_serves(const tahoe_forest *f, unsigned flag)
{
    const tahoe_oshap *sh = f->ob ? f->ob->shap : nullptr;
    if (!sh) return false;
    if (flag == TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL) return sh->iv;
    return flag == TAHOE_CREATE_CONTRIBS ? sh->contribs : flag == TAHOE_CREATE_INTERACTIONS ? sh->inter : sh->approx;
}

tahoe_status oblivious_predict_shap(tahoe_forest *f, unsigned flag, float *phi_dev, const float *data_dev, size_t rows,
                                    hipStream_t stream, const char *fn)
{
    if (rows == 0) return TAHOE_OK;
    if (!phi_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "%s: null argument", fn);
    if (const tahoe_status st = check_shap_out(f, rows, 1, fn)) return st;
    const tahoe_oshap *sh = f->ob->shap;
    DeviceGuard on_device(f->device);
    const int K = f->num_classes;
    const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((K + kObShapClasses - 1) / kObShapClasses));
    // a handle without sets launches the instantiations without the kind test
    const tahoe_ostate *o = f->ob;
    if (o->cats)
        ob_launch_shap<true>(flag, K, sh->inplace, grid, sh->lds_bytes, stream, sh->view, o->cat_pool, o->cat_words, phi_dev, data_dev,
                             rows);
    else
        ob_launch_shap<false>(flag, K, sh->inplace, grid, sh->lds_bytes, stream, sh->view, nullptr, 0u, phi_dev, data_dev, rows);
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

tahoe_status oblivious_predict_interactions(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                            const char *fn)
{
    if (rows == 0) return TAHOE_OK;
    if (!out_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "%s: null argument", fn);
    if (const tahoe_status st = check_shap_out(f, rows, 2, fn)) return st;
    const tahoe_oshap *sh = f->ob->shap;
    DeviceGuard on_device(f->device);
    const int K = f->num_classes;
    const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((K + kObShapClasses - 1) / kObShapClasses));
    const tahoe_ostate *o = f->ob;
    if (o->cats) ob_launch_inter_cat(K, grid, stream, sh->inter_view, o->cat_pool, o->cat_words, out_dev, data_dev, rows);
    else if (K == 1) hipLaunchKernelGGL((oblivious_inter_kernel<1>), grid, dim3(64), 0, stream, sh->inter_view, out_dev, data_dev, rows);
    else hipLaunchKernelGGL((oblivious_inter_kernel<kObShapClasses>), grid, dim3(64), 0, stream, sh->inter_view, out_dev, data_dev, rows);
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

namespace {

void ob_background_free(tahoe_forest *f, tahoe_oshap *sh)
{
    for (void *p : {(void *)sh->occ, (void *)sh->occ_off, (void *)sh->iv_bias})
        if (p) (void)hipFree(p);
    sh->occ = nullptr;
    sh->occ_off = nullptr;
    sh->iv_bias = nullptr;
    f->device_bytes -= sh->bg_bytes;
    sh->bg_rows = sh->bg_bytes = 0;
}

}  // namespace

// tahoe_forest_set_background on a handle with TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL, after the refusals of a NULL handle, a missing
// flag and a NULL background.  The old background stays until the new one is complete.
tahoe_status oblivious_set_background(tahoe_forest *f, const float *bg_dev, size_t bg_rows, hipStream_t stream)
{
    tahoe_oshap *sh = f->ob->shap;
    const size_t F = (size_t)f->p.num_cols, K = (size_t)f->num_classes, T = (size_t)f->p.num_trees;
    if (F > 0 && bg_rows > SIZE_MAX / sizeof(float) / F)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_background: rows x num_cols floats overflow size_t (rows %zu)", bg_rows);
    if (bg_rows > (size_t)INT32_MAX)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_background: %zu background rows (at most 2^31 - 1)", bg_rows);
    DeviceGuard on_device(f->device);
    if (bg_rows == 0) {
        ob_background_free(f, sh);
        return TAHOE_OK;
    }
    if (bg_rows > SIZE_MAX / sizeof(uint32_t) / std::max<size_t>(T, K))
        return fail(TAHOE_ERR_NO_MEMORY, "tahoe_forest_set_background: %zu rows x %zu trees of leaf indices overflow size_t", bg_rows, T);
    uint32_t *leaf = nullptr;
    float *sums = nullptr;
    uint2 *occ = nullptr;
    int32_t *occ_off = nullptr;
    float *bias = nullptr;
    auto bail = [&](tahoe_status st) {
        for (void *p : {(void *)leaf, (void *)sums, (void *)occ, (void *)occ_off, (void *)bias})
            if (p) (void)hipFree(p);
        (void)hipGetLastError();  // a failed allocation is not the caller's next error
        return st;
    };
    if (hipMalloc(reinterpret_cast<void **>(&leaf), std::max<size_t>(bg_rows * T, 1) * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&sums), bg_rows * K * sizeof(float)) != hipSuccess)
        return bail(fail(TAHOE_ERR_NO_MEMORY, "tahoe_forest_set_background: the leaf indices of %zu background rows x %zu trees do not "
                                              "fit on the device; the previous background is kept", bg_rows, T));
    // R(r, t): tahoe_forest_predict_leaf_idx's words; raw_k(r): tahoe_forest_predict_raw's bits.  DIRECT serves every shape and
    // allocates nothing; the caller's strategy setting is restored.
    const int saved = f->strategy;
    f->strategy = TAHOE_STRATEGY_DIRECT;
    tahoe_status st = tahoe_forest_predict_leaf_idx(f, leaf, nullptr, bg_dev, bg_rows, stream);
    if (st == TAHOE_OK) st = tahoe_forest_predict_raw(f, sums, bg_dev, bg_rows, stream);
    f->strategy = saved;
    if (st != TAHOE_OK) return bail(st);
    std::vector<uint32_t> h_leaf(bg_rows * T);
    std::vector<float> raw(bg_rows * K);
    hipError_t e = hipMemcpyAsync(h_leaf.data(), leaf, h_leaf.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(raw.data(), sums, raw.size() * sizeof(float), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return bail(fail(TAHOE_ERR_HIP, "tahoe_forest_set_background: %s", hipGetErrorString(e)));

    // per tree the occupied leaves, ascending, with their counts
    std::vector<uint2> h_occ;
    std::vector<int32_t> h_off(T + 1, 0);
    std::vector<uint32_t> col(bg_rows);
    for (size_t t = 0; t < T; ++t) {
        for (size_t r = 0; r < bg_rows; ++r) col[r] = h_leaf[r * T + t];
        std::sort(col.begin(), col.end());
        for (size_t r = 0; r < bg_rows;) {
            size_t n = r;
            while (n < bg_rows && col[n] == col[r]) ++n;
            h_occ.push_back(make_uint2(col[r], (uint32_t)(n - r)));
            r = n;
        }
        if (h_occ.size() > (size_t)INT32_MAX)
            return bail(fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_background: more than 2^31 - 1 occupied (tree, leaf) pairs"));
        h_off[t + 1] = (int32_t)h_occ.size();
    }
    const bool avg = (f->p.output & TAHOE_OUT_AVG) != 0 && T > 0;
    std::vector<float> h_bias(K);
    for (size_t k = 0; k < K; ++k) {
        double sum = 0.0;
        for (size_t r = 0; r < bg_rows; ++r) sum += (double)raw[r * K + k];
        double m = sum / (double)bg_rows;
        if (avg) m /= (double)T;
        h_bias[k] = (float)(m + (double)f->p.global_bias);
    }
    size_t bytes = 0;
    if ((e = upload(&occ, h_occ, &bytes)) != hipSuccess || (e = upload(&occ_off, h_off, &bytes)) != hipSuccess ||
        (e = upload(&bias, h_bias, &bytes)) != hipSuccess)
        return bail(fail(e == hipErrorOutOfMemory ? TAHOE_ERR_NO_MEMORY : TAHOE_ERR_HIP,
                         "tahoe_forest_set_background: %s; the previous background is kept", hipGetErrorString(e)));
    (void)hipFree(leaf);
    (void)hipFree(sums);
    ob_background_free(f, sh);
    sh->occ = occ;
    sh->occ_off = occ_off;
    sh->iv_bias = bias;
    sh->bg_rows = bg_rows;
    sh->bg_bytes = bytes;
    f->device_bytes += bytes;
    return TAHOE_OK;
}

// tahoe_forest_predict_contribs_interventional on such a handle, after the refusals of a NULL handle and a missing flag
tahoe_status oblivious_predict_interventional(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                              const char *fn)
{
    const tahoe_oshap *sh = f->ob->shap;
    if (sh->bg_rows == 0) return fail(TAHOE_ERR_UNSUPPORTED, "%s: no background set (tahoe_forest_set_background)", fn);
    if (rows == 0) return TAHOE_OK;
    if (!phi_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "%s: null argument", fn);
    if (const tahoe_status st = check_shap_out(f, rows, 1, fn)) return st;
    if ((rows + 63) / 64 > 0x7fffffffu) return fail(TAHOE_ERR_INVALID_ARG, "%s: too many rows for one launch: %zu", fn, rows);
    DeviceGuard on_device(f->device);
    const int K = f->num_classes;
    ObShapView v = sh->view;
    v.bias = sh->iv_bias;
    const ObIvView b{sh->occ, sh->occ_off, sh->wtab, (float)sh->bg_rows};
    const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((K + kObShapClasses - 1) / kObShapClasses));
    const tahoe_ostate *o = f->ob;
    if (o->cats) ob_launch_iv<true>(K, sh->inplace, grid, sh->iv_lds_bytes, stream, v, o->cat_pool, o->cat_words, b, phi_dev, data_dev, rows);
    else ob_launch_iv<false>(K, sh->inplace, grid, sh->iv_lds_bytes, stream, v, nullptr, 0u, b, phi_dev, data_dev, rows);
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

}  // namespace tahoe

#endif  // TAHOE_OBLIVIOUS_SHAP_CAT_UNIT
