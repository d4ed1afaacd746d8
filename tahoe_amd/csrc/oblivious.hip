// Oblivious (symmetric) forests -- CatBoost models -- on a native handle (tahoe_oblivious_forest_create).
//
// Every node of a level of an oblivious tree shares one split, so a tree of depth D is D (feature, border) records and a table of
// 2^D leaves, each a vector of K = leaf_dim values.  Device layout, built once at create:
//   splits[sum D_t]      InnerNode {thr, fid | def_left << 31}, tree-major, record l of a tree = the split of level l
//   split_off[T + 1]     first record of tree t; D_t = split_off[t + 1] - split_off[t]
//   leaf_off[T]          first leaf of tree t, in leaves (64-bit: T x 2^16 leaves x K values passes 2^31)
//   leaves[sum 2^D_t][K] as the caller gave them (CatBoost's layout)
//   cat_pool[]           tahoe_oblivious_forest_create_cat only: header and words of every set wider than one word; a narrower set
//                        rides in its split record (forest_internal.h: kObCat)
// The walk has nothing to gather per lane: a level's split record sits at a wave-uniform address (scalar loads), its feature is one
// 64-float row of the LDS tile, the leaf index is D compare bits (level 0 = bit 0), and one table read finishes the tree.
//
// Sum order: margin[row][k] = float32 sum from +0.0f over trees 0..T-1 in order of leaves[t][idx_t][k] -- what every other kernel
// of the library computes on the heap expansion of the forest, bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "oblivious_internal.h"

namespace tahoe {

constexpr int kObTrees = 4;    // consecutive trees whose leaf indices and leaf reads are in flight before they are added in order
constexpr int kObClasses = 8;  // accumulators a lane keeps: gridDim.y runs over blocks of 8 classes, each repeats the walk

// The walk of one row over all trees, for classes [blockIdx.y * KB, + KB).  feature(fid) reads the row's value of a feature.
// KB == 1 is the single-output handle (K == 1; sums_in continues a running sum), KB == kObClasses a block of a vector leaf.
// Leaf indices are written once, by class block 0.
// CAT: the handle has category sets (tahoe_oblivious_forest_create_cat); a level's record then says its kind (ob_split_bit).  An
// inline set is tested in registers; a pooled one gathers its member word per lane, and the kObTrees trees in flight overlap it.
// STAGED (tahoe_forest_predict_staged on a handle of TAHOE_CREATE_STAGED): `sums` is out[rows][S][K] and
// stages[0 .. S) the strictly ascending tree counts.  The running sums are stored wherever the tree just added ends a stage, by a
// cursor si that every class block runs for itself; the sums go on untouched, and the final store is not done (a stage equal
// to num_trees is that store).  first_end is stages[0], which a kernel reads before it stages its tile: read here, the load's
// latency stands between the tile and the first tree of every wave.
template <int KB, bool WRITE_LEAF, bool CAT, bool STAGED = false, class Feature>
__device__ __forceinline__ void oblivious_walk(const InnerNode *__restrict__ splits, const int32_t *__restrict__ split_off,
                                               const int64_t *__restrict__ leaf_off, const float *__restrict__ leaves, float *sums,
                                               uint32_t *__restrict__ leaf_out, const float *sums_in, size_t row, bool row_ok,
                                               int num_trees, int K, float missing, const uint32_t *__restrict__ cat_pool,
                                               uint32_t cat_words, const int32_t *__restrict__ stages, int S, int first_end,
                                               Feature &&feature)
{
    static_assert(!STAGED || !WRITE_LEAF, "no staged leaf indices");
    const int k0 = (int)blockIdx.y * KB;
    float acc[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) acc[j] = 0.0f;
    if (KB == 1 && sums_in && row_ok) acc[0] = sums_in[row];  // continues a running sum (tree shards chained in order)
    const bool write_leaf = WRITE_LEAF && row_ok && blockIdx.y == 0;

    // v[0 .. KB) <- the row's leaf values of tree t for this class block
    auto walk_tree = [&](int t, float *v) {
        const int s0 = split_off[t];
        const int d = split_off[t + 1] - s0;  // wave-uniform, as every split record below
        uint32_t idx = 0;
#pragma unroll 4
        for (int l = 0; l < d; ++l) {
            const InnerNode n = splits[s0 + l];
            const uint32_t fid = CAT ? ob_split_fid(n.meta) : n.meta & kMetaFidMask;
            idx |= ob_split_bit<CAT>(n, feature(fid), missing, cat_pool, cat_words) << l;
        }
        if (write_leaf) leaf_out[row * (size_t)num_trees + t] = idx;
        const float *lv = leaves + ((size_t)leaf_off[t] + idx) * (size_t)K + k0;
#pragma unroll
        for (int j = 0; j < KB; ++j) v[j] = (KB == 1 || k0 + j < K) ? lv[j] : 0.0f;
    };

    // STAGED: the cursor and the tree count that ends its stage (wave-uniform; one load when the cursor moves); -1 after the last
    int si = 0, send = first_end;
    auto stage_end = [&](int trees_done) {  // after the adds of tree trees_done - 1
        if (trees_done != send) return;
        if (row_ok) {
#pragma unroll
            for (int j = 0; j < KB; ++j)
                if (KB == 1 || k0 + j < K) sums[(row * (size_t)S + (size_t)si) * (size_t)K + k0 + j] = acc[j];
        }
        ++si;
        send = si < S ? stages[si] : -1;
    };

    int t = 0;
    if constexpr (STAGED) {
        // A loop of its own (the plain one below keeps its statements, and so its instruction stream).  ends: a stage may end in
        // this window, at any of the four trees
        auto window = [&](int t0, auto ends) {
            float v[kObTrees][KB];
#pragma unroll
            for (int u = 0; u < kObTrees; ++u) walk_tree(t0 + u, v[u]);
#pragma unroll
            for (int u = 0; u < kObTrees; ++u) {  // tree order
#pragma unroll
                for (int j = 0; j < KB; ++j) acc[j] += v[u][j];
                if constexpr (decltype(ends)::value) stage_end(t0 + u + 1);
            }
        };
        // The windows that lie before the cursor's stage end run the plain loop, bounded by that end instead of num_trees, so the
        // compare is paid per stage and not per tree (on a K == 1 tree of depth 6 a compare per tree was 2.4 % of the walk); the
        // window a stage ends in takes the compares.  Every end <= t is behind the cursor: send > t or send == -1.
        for (;;) {
            const int before = send < 0 ? num_trees : min(num_trees, send - 1);
            for (; t + kObTrees <= before; t += kObTrees) window(t, std::false_type{});
            if (t + kObTrees > num_trees) break;
            window(t, std::true_type{});
            t += kObTrees;
        }
    }
    for (; !STAGED && t + kObTrees <= num_trees; t += kObTrees) {
        float v[kObTrees][KB];
#pragma unroll
        for (int u = 0; u < kObTrees; ++u) walk_tree(t + u, v[u]);
#pragma unroll
        for (int u = 0; u < kObTrees; ++u)  // tree order
#pragma unroll
            for (int j = 0; j < KB; ++j) acc[j] += v[u][j];
    }
    for (; t < num_trees; ++t) {
        float v[KB];
        walk_tree(t, v);
#pragma unroll
        for (int j = 0; j < KB; ++j) acc[j] += v[j];
        if constexpr (STAGED) stage_end(t + 1);
    }
    if (!STAGED && sums && row_ok) {
#pragma unroll
        for (int j = 0; j < KB; ++j)
            if (KB == 1 || k0 + j < K) sums[row * (size_t)K + k0 + j] = acc[j];
    }
}

// ROWTILE on an oblivious handle: one wave = one workgroup owns 64 rows (lane = row), staged feature-major in LDS with the loop of
// rowtile_kernel; a level's feature is the row tile[fid][0..64): 64 consecutive floats, no bank conflict, no per-lane address
// arithmetic.  A lane reads back only what it stored itself, so there is no barrier after staging, and nothing crosses waves.
// Dynamic LDS: [cols][64] float.
// CSR (tahoe_forest_predict_csr on a handle of TAHOE_CREATE_CSR): the tile is staged from csr by
// csr_stage_tile_wave (forest_internal.h) and `data` is not read.  There kCsrLanes lanes scatter one row, so a lane does read what
// other lanes stored: a barrier stands between the staging and the walk.  Every class block stages the tile again.
template <int KB, bool WRITE_LEAF, bool CAT, bool STAGED = false, bool CSR = false>
__global__ void __launch_bounds__(kTileRows) oblivious_tile_kernel(const InnerNode *__restrict__ splits,
                                                                   const int32_t *__restrict__ split_off,
                                                                   const int64_t *__restrict__ leaf_off,
                                                                   const float *__restrict__ leaves, const float *__restrict__ data,
                                                                   float *sums, uint32_t *__restrict__ leaf_out, const float *sums_in,
                                                                   size_t rows, int cols, int num_trees, int K, float missing,
                                                                   int vec4_ok, const uint32_t *__restrict__ cat_pool,
                                                                   uint32_t cat_words, const int32_t *__restrict__ stages, int S,
                                                                   CsrView csr)
{
    static_assert(!CSR || (!WRITE_LEAF && !STAGED), "CSR rows: predictions only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *tile = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * kTileRows;
    const size_t row = row0 + lane;
    const bool row_ok = row < rows;
    const int first_end = STAGED ? stages[0] : 0;

    // ---- stage the row tile, transposed to feature-major ----
    if constexpr (CSR) {
        csr_stage_tile_wave(tile, cols, row0, rows, csr, missing, lane);
        __syncthreads();  // the walk reads what other lanes scattered
    } else {
        const float *src = data + (row_ok ? row : row0) * (size_t)cols;
        if (vec4_ok) {
            const float4 *src4 = reinterpret_cast<const float4 *>(src);
            for (int f4 = 0; f4 < cols / 4; ++f4) {
                float4 v = row_ok ? src4[f4] : make_float4(0.f, 0.f, 0.f, 0.f);
                tile[(4 * f4 + 0) * kTileRows + lane] = v.x;
                tile[(4 * f4 + 1) * kTileRows + lane] = v.y;
                tile[(4 * f4 + 2) * kTileRows + lane] = v.z;
                tile[(4 * f4 + 3) * kTileRows + lane] = v.w;
            }
        } else {
            for (int f = 0; f < cols; ++f) tile[f * kTileRows + lane] = row_ok ? src[f] : 0.0f;
        }
    }

    oblivious_walk<KB, WRITE_LEAF, CAT, STAGED>(splits, split_off, leaf_off, leaves, sums, leaf_out, sums_in, row, row_ok, num_trees,
                                                K, missing, cat_pool, cat_words, stages, S, first_end,
                                                [&](uint32_t fid) { return tile[fid * kTileRows + lane]; });
}

// DIRECT: the same walk with the features read from global memory, for any num_cols.
template <int KB, bool WRITE_LEAF, bool CAT, bool STAGED = false>
__global__ void __launch_bounds__(kBlock) oblivious_direct_kernel(const InnerNode *__restrict__ splits,
                                                                  const int32_t *__restrict__ split_off,
                                                                  const int64_t *__restrict__ leaf_off,
                                                                  const float *__restrict__ leaves, const float *__restrict__ data,
                                                                  float *sums, uint32_t *__restrict__ leaf_out, const float *sums_in,
                                                                  size_t rows, int cols, int num_trees, int K, float missing,
                                                                  const uint32_t *__restrict__ cat_pool, uint32_t cat_words,
                                                                  const int32_t *__restrict__ stages, int S)
{
    const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool row_ok = row < rows;
    const float *x = data + (row_ok ? row : 0) * (size_t)cols;  // (a lane past the batch walks row 0 and stores nothing)
    oblivious_walk<KB, WRITE_LEAF, CAT, STAGED>(splits, split_off, leaf_off, leaves, sums, leaf_out, sums_in, row, row_ok, num_trees,
                                                K, missing, cat_pool, cat_words, stages, S, STAGED ? stages[0] : 0,
                                                [&](uint32_t fid) { return x[fid]; });
}

static long long oblivious_tile_bytes(const tahoe_forest *f) { return (long long)f->p.num_cols * kTileRows * (long long)sizeof(float); }

bool oblivious_tile_fits(const tahoe_forest *f) { return f->p.num_cols >= 1 && oblivious_tile_bytes(f) <= f->lds_limit; }

// The launch of both forms.  STAGED: sums is out[rows][num_stages][K], leaf_out and sums_in are null.  csr (never with STAGED):
// the tile kernel's CSR instantiation; strategy is ROWTILE (csr_fused_strategy), leaf_out null
template <bool STAGED>
static tahoe_status oblivious_launch_as(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data, size_t rows,
                                        hipStream_t stream, int strategy, const float *sums_in, const CsrView *csr = nullptr)
{
    if (csr && (STAGED || leaf_out || strategy != TAHOE_STRATEGY_ROWTILE))
        return fail(TAHOE_ERR_UNSUPPORTED, "oblivious_launch: CSR rows are served by the tile kernel, predictions only");
    const tahoe_ostate *o = f->ob;
    const int32_t *stages = STAGED ? f->stages_dev : nullptr;
    const int S = STAGED ? (int)f->num_stages : 0;
    const int K = f->num_classes, T = f->p.num_trees, cols = f->p.num_cols;
    const unsigned blocks_y = (unsigned)((K + kObClasses - 1) / kObClasses);  // 1 when K == 1
    const int vec4_ok = (cols % 4 == 0) && ((reinterpret_cast<uintptr_t>(data) & 15u) == 0);
    auto launch = [&](auto kb, auto wl, auto cat) {
        constexpr int KB = decltype(kb)::value;
        constexpr bool WL = decltype(wl)::value && !STAGED;
        constexpr bool CAT = decltype(cat)::value;
        if (csr) {
            if constexpr (!STAGED && !WL)
                hipLaunchKernelGGL((oblivious_tile_kernel<KB, false, CAT, false, true>),
                                   dim3((unsigned)((rows + kTileRows - 1) / kTileRows), blocks_y), dim3(kTileRows),
                                   (size_t)oblivious_tile_bytes(f), stream, o->splits, o->split_off, o->leaf_off, o->leaves, data, sums,
                                   leaf_out, sums_in, rows, cols, T, K, f->p.missing, vec4_ok, o->cat_pool, o->cat_words, stages, S,
                                   *csr);
        } else if (strategy == TAHOE_STRATEGY_ROWTILE)
            hipLaunchKernelGGL((oblivious_tile_kernel<KB, WL, CAT, STAGED>),
                               dim3((unsigned)((rows + kTileRows - 1) / kTileRows), blocks_y), dim3(kTileRows),
                               (size_t)oblivious_tile_bytes(f), stream, o->splits, o->split_off, o->leaf_off, o->leaves, data, sums,
                               leaf_out, sums_in, rows, cols, T, K, f->p.missing, vec4_ok, o->cat_pool, o->cat_words, stages, S,
                               CsrView{});
        else
            hipLaunchKernelGGL((oblivious_direct_kernel<KB, WL, CAT, STAGED>), dim3((unsigned)((rows + kBlock - 1) / kBlock), blocks_y),
                               dim3(kBlock), 0, stream, o->splits, o->split_off, o->leaf_off, o->leaves, data, sums, leaf_out, sums_in,
                               rows, cols, T, K, f->p.missing, o->cat_pool, o->cat_words, stages, S);
    };
    with_leaf(leaf_out != nullptr, [&](auto wl) {  // a handle without sets launches the instantiation without the kind test
        auto with_classes = [&](auto cat) {
            if (K == 1) launch(std::integral_constant<int, 1>{}, wl, cat);
            else launch(std::integral_constant<int, kObClasses>{}, wl, cat);
        };
        if (o->cats) with_classes(std::true_type{});
        else with_classes(std::false_type{});
    });
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

tahoe_status oblivious_launch(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data, size_t rows, hipStream_t stream,
                              int strategy, const float *sums_in, const CsrView *csr)
{
    return oblivious_launch_as<false>(f, sums, leaf_out, data, rows, stream, strategy, sums_in, csr);
}

tahoe_status oblivious_launch_staged(tahoe_forest *f, float *out, const float *data, size_t rows, hipStream_t stream, int strategy)
{
    return oblivious_launch_as<true>(f, out, nullptr, data, rows, stream, strategy, nullptr);
}

void oblivious_destroy(tahoe_forest *f)
{
    tahoe_ostate *o = f->ob;
    if (!o) return;
    oblivious_shap_destroy(f);
    if (o->splits) (void)hipFree(o->splits);
    if (o->split_off) (void)hipFree(o->split_off);
    if (o->leaf_off) (void)hipFree(o->leaf_off);
    if (o->leaves) (void)hipFree(o->leaves);
    if (o->cat_pool) (void)hipFree(o->cat_pool);
    delete o;
    f->ob = nullptr;
}

// The tile kernels may need more than the default 64 KiB of dynamic LDS
static tahoe_status oblivious_allow_lds(const tahoe_forest *f)
{
    hipError_t e = hipSuccess;
    if (!oblivious_tile_fits(f)) return TAHOE_OK;
    if (f->ob->cats
            ? ((e = allow_max_lds_leaf([](auto wl) { return &oblivious_tile_kernel<1, decltype(wl)::value, true>; }, f->lds_limit)) != hipSuccess ||
               (e = allow_max_lds_leaf([](auto wl) { return &oblivious_tile_kernel<kObClasses, decltype(wl)::value, true>; }, f->lds_limit)) != hipSuccess)
            : ((e = allow_max_lds_leaf([](auto wl) { return &oblivious_tile_kernel<1, decltype(wl)::value, false>; }, f->lds_limit)) != hipSuccess ||
               (e = allow_max_lds_leaf([](auto wl) { return &oblivious_tile_kernel<kObClasses, decltype(wl)::value, false>; }, f->lds_limit)) != hipSuccess))
        return hip_status(e, "hipFuncSetAttribute(oblivious_tile)");
    if (f->csr) {  // the CSR-loader instantiations (tahoe_forest_predict_csr) of this handle's kind
        const bool one = f->num_classes == 1;
        const void *fn = f->ob->cats ? (one ? reinterpret_cast<const void *>(&oblivious_tile_kernel<1, false, true, false, true>)
                                            : reinterpret_cast<const void *>(&oblivious_tile_kernel<kObClasses, false, true, false, true>))
                                     : (one ? reinterpret_cast<const void *>(&oblivious_tile_kernel<1, false, false, false, true>)
                                            : reinterpret_cast<const void *>(&oblivious_tile_kernel<kObClasses, false, false, false, true>));
        return hip_status(allow_max_lds(fn, f->lds_limit), "hipFuncSetAttribute(oblivious_tile, csr)");
    }
    return TAHOE_OK;
}

// ... and so may the staged ones of this handle (tahoe_forest_set_stages calls it)
tahoe_status oblivious_allow_staged_lds(const tahoe_forest *f)
{
    if (!oblivious_tile_fits(f)) return TAHOE_OK;
    const bool one = f->num_classes == 1;
    const void *fn = f->ob->cats ? (one ? reinterpret_cast<const void *>(&oblivious_tile_kernel<1, false, true, true>)
                                        : reinterpret_cast<const void *>(&oblivious_tile_kernel<kObClasses, false, true, true>))
                                 : (one ? reinterpret_cast<const void *>(&oblivious_tile_kernel<1, false, false, true>)
                                        : reinterpret_cast<const void *>(&oblivious_tile_kernel<kObClasses, false, false, true>));
    return hip_status(allow_max_lds(fn, f->lds_limit), "hipFuncSetAttribute(oblivious_tile, staged)");
}

}  // namespace tahoe

using namespace tahoe;

extern "C" tahoe_status tahoe_oblivious_forest_create_cat(tahoe_forest **out, const int32_t *depths,
                                                          const tahoe_oblivious_split *splits, const float *leaf_values,
                                                          const float *leaf_covers, const tahoe_forest_params *p, int leaf_dim,
                                                          unsigned flags, const tahoe_categorical_splits *cats)
{
    // every check here runs before a device is touched
    if (!out || !depths || !leaf_values || !p) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_oblivious_forest_create: null argument");
    *out = nullptr;
    if (p->num_trees < 0) return fail(TAHOE_ERR_INVALID_ARG, "num_trees must be non-negative");
    const int T = p->num_trees;
    long long total_depth = 0;
    for (int t = 0; t < T; ++t) total_depth += depths[t];
    if (total_depth > 0 && !splits) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_oblivious_forest_create: splits is null");
    if (total_depth > INT32_MAX) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_oblivious_forest_create: more than 2^31 - 1 splits");
    if (leaf_dim < 1 || leaf_dim > 1024)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_oblivious_forest_create: leaf_dim must be in [1,1024], got %d", leaf_dim);
    if (const tahoe_status s = check_params(p, leaf_dim, true, "splits")) return s;
    tahoe_forest_params any_trees = *p;
    any_trees.num_trees = 0;  // every tree feeds every class: no multiple-of-classes rule, only the output bits
    if (const tahoe_status s = check_classes(&any_trees, leaf_dim)) return s;
    for (int t = 0; t < T; ++t)
        if (depths[t] < 0 || depths[t] > kObMaxDepth)
            return fail(TAHOE_ERR_INVALID_ARG, "tahoe_oblivious_forest_create: tree %d: depth %d is outside [0,%d]", t, depths[t],
                        kObMaxDepth);
    std::vector<InnerNode> h_splits((size_t)total_depth);
    std::vector<int32_t> h_split_off((size_t)T + 1, 0);
    std::vector<int64_t> h_leaf_off((size_t)T, 0);
    int max_depth = 0;
    size_t num_leaves = 0;
    for (int t = 0, s = 0; t < T; ++t) {
        for (int l = 0; l < depths[t]; ++l, ++s) {
            const uint32_t bits = (uint32_t)splits[s].bits;
            const uint32_t fid = bits & kMetaFidMask;
            if (fid >= (uint32_t)p->num_cols)
                return fail(TAHOE_ERR_INVALID_FOREST, "tahoe_oblivious_forest_create: tree %d level %d: fid %u >= num_cols %d", t, l, fid,
                            p->num_cols);
            h_splits[(size_t)s] = InnerNode{splits[s].thr, fid | ((bits >> 30) & 1u) << 31};
        }
        h_split_off[(size_t)t + 1] = s;
        h_leaf_off[(size_t)t] = (int64_t)num_leaves;
        num_leaves += (size_t)1 << depths[t];
        max_depth = std::max(max_depth, depths[t]);
    }

    // ... and the checks of the explanation flags, after those every create makes
    // (TAHOE_CREATE_STAGED opens tahoe_forest_set_stages / _predict_staged, reads no cover and builds no table; TAHOE_CREATE_CSR
    // opens tahoe_forest_predict_csr / _reserve_csr / _get_csr_plan in the same way)
    const bool staged = (flags & TAHOE_CREATE_STAGED) != 0, csr_rows = (flags & TAHOE_CREATE_CSR) != 0;
    flags &= ~(unsigned)(TAHOE_CREATE_STAGED | TAHOE_CREATE_CSR);
    if (const tahoe_status s = check_nan_missing_flags(flags, "an oblivious")) return s;
    if (flags & ~(unsigned)(TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_APPROX_CONTRIBS | TAHOE_CREATE_INTERACTIONS |
                            TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL))
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_oblivious_forest_create_ex: flags 0x%x: only TAHOE_CREATE_CONTRIBS, "
                                           "TAHOE_CREATE_APPROX_CONTRIBS, TAHOE_CREATE_INTERACTIONS and "
                                           "TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL are served", flags);
    const unsigned cover_flags = flags & ~(unsigned)TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL;  // (the interventional game reads no cover)
    if (cover_flags && !leaf_covers)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_oblivious_forest_create_ex: leaf_covers is null, and the flags need the covers");
    if (cover_flags)
        if (const tahoe_status s = oblivious_shap_validate(depths, T, leaf_covers)) return s;

    // ... and those of the category sets (tahoe_oblivious_forest_create_cat), which name (tree, level) records
    std::vector<uint32_t> h_pool;
    if (cats) {
        if (const tahoe_status s = check_cat_args(cats, (int)total_depth)) return s;
        if (cats->num_splits == 0) cats = nullptr;  // the handle of tahoe_oblivious_forest_create_ex
    }
    if (cats) {
        if (p->num_cols > (1 << 28))
            return fail(TAHOE_ERR_UNSUPPORTED, "tahoe_oblivious_forest_create_cat: categorical splits need num_cols <= 2^28 (the "
                                               "split record keeps bits 28 to 30 for the kind of split); num_cols = %d", p->num_cols);
        // a set of at most one word rides in its record, where thr was; a wider one goes to the pool: header, then its words
        for (int k = 0; k < cats->num_splits; ++k) {
            InnerNode &n = h_splits[(size_t)cats->node[k]];
            const uint32_t nw = (uint32_t)(cats->offset[k + 1] - cats->offset[k]);
            const bool ml = cats->members_left && cats->members_left[k];
            uint32_t word = nw ? cats->words[cats->offset[k]] : 0u;
            n.meta |= kObCat;
            if (nw <= 1) {
                n.meta |= ml ? kObCatLeft : 0u;
            } else {
                n.meta |= kObCatPooled;
                word = (uint32_t)h_pool.size();
                h_pool.push_back((ml ? 0x80000000u : 0u) | nw);
                h_pool.insert(h_pool.end(), cats->words + cats->offset[k], cats->words + cats->offset[k + 1]);
            }
            memcpy(&n.thr, &word, sizeof word);
        }
    }

    ForestPtr f;
    if (const tahoe_status s = open_handle(p, leaf_dim, f)) return s;
    f->class_trees = T;  // AVG divides by (float)num_trees whatever K is
    f->p.depth = f->depth = max_depth;
    f->staged = staged;
    f->csr = csr_rows;
    f->ob = new (std::nothrow) tahoe_ostate();
    if (!f->ob) return fail(TAHOE_ERR_NO_MEMORY, "tahoe_oblivious_forest_create");
    tahoe_ostate *o = f->ob;
    o->cats = cats != nullptr;
    tahoe_status s = TAHOE_OK;
    if (!h_pool.empty()) {
        o->cat_words = (uint32_t)h_pool.size();
        if ((s = hip_status(upload(&o->cat_pool, h_pool, &f->device_bytes), "upload(categorical splits)"))) return s;
    }
    if ((s = hip_status(upload(&o->splits, h_splits, &f->device_bytes), "upload(splits)")) ||
        (s = hip_status(upload(&o->split_off, h_split_off, &f->device_bytes), "upload(split_off)")) ||
        (s = hip_status(upload(&o->leaf_off, h_leaf_off, &f->device_bytes), "upload(leaf_off)")) ||
        (s = hip_status(upload(&o->leaves, leaf_values, num_leaves * (size_t)leaf_dim, &f->device_bytes), "upload(leaves)")) ||
        (s = oblivious_allow_lds(f.get())))
        return s;
    if (flags) {
        const ObliviousSource src{depths, &h_splits, &h_split_off, &h_leaf_off, leaf_values, leaf_covers, num_leaves};
        if ((s = oblivious_shap_build(f.get(), src, flags))) return s;
    }
    *out = f.release();
    return TAHOE_OK;
}

extern "C" tahoe_status tahoe_oblivious_forest_create_ex(tahoe_forest **out, const int32_t *depths,
                                                         const tahoe_oblivious_split *splits, const float *leaf_values,
                                                         const float *leaf_covers, const tahoe_forest_params *p, int leaf_dim,
                                                         unsigned flags)
{
    return tahoe_oblivious_forest_create_cat(out, depths, splits, leaf_values, leaf_covers, p, leaf_dim, flags, nullptr);
}

extern "C" tahoe_status tahoe_oblivious_forest_create(tahoe_forest **out, const int32_t *depths, const tahoe_oblivious_split *splits,
                                                      const float *leaf_values, const tahoe_forest_params *p, int leaf_dim)
{
    return tahoe_oblivious_forest_create_ex(out, depths, splits, leaf_values, nullptr, p, leaf_dim, 0u);
}
