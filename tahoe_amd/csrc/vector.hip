// Vector-leaf forests -- irregular trees whose leaves hold K values -- on a native handle (tahoe_vector_forest_create; DESIGN.md
// section 25): scikit-learn's forest classifiers and multi-output regressors, XGBoost's multi_output_tree.
//
// Device layout, built once at create:
//   nodes[num_nodes]   VNode, 16 bytes: {val, bits, left_idx, 0} in the caller's order -- the 12-byte tahoe_sparse_node padded so
//                      that a step of the walk is one aligned 16-byte gather that never straddles a cache line.  At a leaf
//                      left_idx is the index of the leaf's vector.
//   roots[T]           first node of tree t
//   leaves[L][K]       the leaf vectors as the caller gave them
// The node order is the caller's, so the position the walk ends on is the leaf index the caller expects.
//
// Sum order: margin[row][k] = float32 sum from +0.0f over trees 0..T-1 in order of the row's leaf vector element k -- what the
// sparse kernels compute on the K-fold expansion of the forest (tree t * K + k = tree t with element k at its leaves), bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <type_traits>
#include <vector>

#include "forest_internal.h"
#include "vector_internal.h"

namespace tahoe {

constexpr int kVecTrees = 4;    // consecutive trees a lane walks at once; their leaf reads are in flight before they are added in order
constexpr int kVecClasses = 8;  // accumulators a lane keeps: gridDim.y runs over blocks of 8 classes, each repeats the walk

// The walk of one row over all trees, for classes [blockIdx.y * KB, + KB).  feature(fid) reads the row's value of a feature.
// KB == 1 is the single-output handle (K == 1), KB == kVecClasses a block of a vector leaf.  Leaf indices are written once, by
// class block 0.
// STAGED (tahoe_forest_predict_staged on a handle of TAHOE_CREATE_STAGED): `sums` is out[rows][S][K] and
// stages[0 .. S) the strictly ascending tree counts.  The running sums are stored wherever the tree just added ends a stage, by a
// cursor si that every class block runs for itself; the sums go on untouched, and the final store is not done (a stage equal
// to num_trees is that store).  first_end is stages[0], which a kernel reads before it stages its tile.  The compare sits after
// every tree's adds: next to the gathers of an irregular tree it does not show, so this walk has no second loop as
// oblivious_walk's has.
template <int KB, bool WRITE_LEAF, bool STAGED = false, class Feature>
__device__ __forceinline__ void vector_walk(const VNode *__restrict__ nodes, const int32_t *__restrict__ roots,
                                            const float *__restrict__ leaves, float *sums, uint32_t *__restrict__ leaf_out, size_t row,
                                            bool row_ok, int num_trees, int K, float missing, const int32_t *__restrict__ stages, int S,
                                            int first_end, Feature &&feature)
{
    static_assert(!STAGED || !WRITE_LEAF, "no staged leaf indices");
    const int k0 = (int)blockIdx.y * KB;
    float acc[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) acc[j] = 0.0f;
    const bool write_leaf = WRITE_LEAF && row_ok && blockIdx.y == 0;

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

    // Trees t .. t + W - 1 at once.  A step of tree u is a per-lane gather of one node, so the W gathers of a round are issued
    // together, unconditionally -- a lane that has reached its leaf in tree u re-reads the root, one cache line for all such
    // lanes -- and the round's W feature reads follow together.  The rounds end when every lane has a leaf in all W trees: a
    // lane that is done with one tree keeps stepping the others.  create() guarantees left_idx > curr and in range: the walk
    // terminates.
    auto window = [&](int t, auto w) {
        constexpr int W = decltype(w)::value;
        const VNode *root[W];
        uint32_t curr[W], vec[W];
        bool done[W];
#pragma unroll
        for (int u = 0; u < W; ++u) {
            root[u] = nodes + roots[t + u];
            curr[u] = 0u;
            vec[u] = 0u;
            done[u] = false;
        }
        for (;;) {
            VNode n[W];
#pragma unroll
            for (int u = 0; u < W; ++u) n[u] = root[u][done[u] ? 0u : curr[u]];
            bool live[W];
            float x[W];
#pragma unroll
            for (int u = 0; u < W; ++u) {
                const bool leaf = (n[u].bits & kVIsLeaf) != 0u;
                live[u] = !done[u] && !leaf;
                vec[u] = (!done[u] && leaf) ? n[u].left_idx : vec[u];
                done[u] = done[u] || leaf;
                x[u] = feature(live[u] ? (n[u].bits & kVFidMask) : 0u);  // (fid 0 exists: a tree with an internal node has num_cols >= 1)
            }
            bool all = true;
#pragma unroll
            for (int u = 0; u < W; ++u) {
                const uint32_t next = n[u].left_idx + go_right(x[u], n[u].val, (n[u].bits & kVDefLeft) != 0u, missing);
                curr[u] = live[u] ? next : curr[u];
                all = all && done[u];
            }
            if (all) break;
        }
        float v[W][KB];
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const float *lv = leaves + (size_t)vec[u] * (size_t)K + k0;
#pragma unroll
            for (int j = 0; j < KB; ++j) v[u][j] = (KB == 1 || k0 + j < K) ? lv[j] : 0.0f;
            if (write_leaf) leaf_out[row * (size_t)num_trees + (size_t)(t + u)] = curr[u];
        }
#pragma unroll
        for (int u = 0; u < W; ++u) {  // tree order
#pragma unroll
            for (int j = 0; j < KB; ++j) acc[j] += v[u][j];
            if constexpr (STAGED) stage_end(t + u + 1);  // (a stage can end at any tree of the window)
        }
    };

    int t = 0;
    for (; t + kVecTrees <= num_trees; t += kVecTrees) window(t, std::integral_constant<int, kVecTrees>{});
    for (; t < num_trees; ++t) window(t, std::integral_constant<int, 1>{});
    if (!STAGED && sums && row_ok) {
#pragma unroll
        for (int j = 0; j < KB; ++j)
            if (KB == 1 || k0 + j < K) sums[row * (size_t)K + k0 + j] = acc[j];
    }
}

// ROWTILE on a vector-leaf handle: one wave = one workgroup owns 64 rows (lane = row), staged feature-major in LDS with the loop
// of oblivious_tile_kernel.  A node's feature is tile[fid * 64 + lane] with a per-lane fid: the bank is the lane's whatever fid
// is, so the read is conflict-free.  A lane reads back only what it stored itself, so there is no barrier after staging, and
// nothing crosses waves.  Dynamic LDS: [cols][64] float.
// CSR (tahoe_forest_predict_csr on a handle of TAHOE_CREATE_CSR): as oblivious_tile_kernel's -- the tile is
// staged by csr_stage_tile_wave, whose lanes store other lanes' rows, so a barrier stands between the staging and the walk.
template <int KB, bool WRITE_LEAF, bool STAGED = false, bool CSR = false>
__global__ void __launch_bounds__(kTileRows) vector_tile_kernel(const VNode *__restrict__ nodes, const int32_t *__restrict__ roots,
                                                                const float *__restrict__ leaves, const float *__restrict__ data,
                                                                float *sums, uint32_t *__restrict__ leaf_out, size_t rows, int cols,
                                                                int num_trees, int K, float missing, int vec4_ok,
                                                                const int32_t *__restrict__ stages, int S, CsrView csr)
{
    static_assert(!CSR || (!WRITE_LEAF && !STAGED), "CSR rows: predictions only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *tile = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * kTileRows;
    const size_t row = row0 + lane;
    const bool row_ok = row < rows;
    const int first_end = STAGED ? stages[0] : 0;

    // ---- stage the row tile, transposed to feature-major (a lane past the batch stages and walks a row of zeros; from CSR: an
    // empty row, every feature missing) ----
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

    vector_walk<KB, WRITE_LEAF, STAGED>(nodes, roots, leaves, sums, leaf_out, row, row_ok, num_trees, K, missing, stages, S,
                                        first_end, [&](uint32_t fid) { return tile[fid * kTileRows + lane]; });
}

// DIRECT: the same walk with the features read from global memory, for any num_cols.
template <int KB, bool WRITE_LEAF, bool STAGED = false>
__global__ void __launch_bounds__(kBlock) vector_direct_kernel(const VNode *__restrict__ nodes, const int32_t *__restrict__ roots,
                                                               const float *__restrict__ leaves, const float *__restrict__ data,
                                                               float *sums, uint32_t *__restrict__ leaf_out, size_t rows, int cols,
                                                               int num_trees, int K, float missing,
                                                               const int32_t *__restrict__ stages, int S)
{
    const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool row_ok = row < rows;
    const float *x = data + (row_ok ? row : 0) * (size_t)cols;  // (a lane past the batch walks row 0 and stores nothing)
    vector_walk<KB, WRITE_LEAF, STAGED>(nodes, roots, leaves, sums, leaf_out, row, row_ok, num_trees, K, missing, stages, S,
                                        STAGED ? stages[0] : 0, [&](uint32_t fid) { return x[fid]; });
}

static long long vector_tile_bytes(const tahoe_forest *f) { return (long long)f->p.num_cols * kTileRows * (long long)sizeof(float); }

bool vector_tile_fits(const tahoe_forest *f) { return f->p.num_cols >= 1 && vector_tile_bytes(f) <= f->lds_limit; }

// The launch of both forms.  STAGED: sums is out[rows][num_stages][K] and leaf_out is null.  csr (never with STAGED): the tile
// kernel's CSR instantiation; strategy is ROWTILE (csr_fused_strategy), leaf_out null
template <bool STAGED>
static tahoe_status vector_launch_as(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data, size_t rows,
                                     hipStream_t stream, int strategy, const CsrView *csr = nullptr)
{
    if (csr && (STAGED || leaf_out || strategy != TAHOE_STRATEGY_ROWTILE))
        return fail(TAHOE_ERR_UNSUPPORTED, "vector_launch: CSR rows are served by the tile kernel, predictions only");
    const tahoe_vstate *v = f->vl;
    const int32_t *stages = STAGED ? f->stages_dev : nullptr;
    const int S = STAGED ? (int)f->num_stages : 0;
    const int K = f->num_classes, T = f->p.num_trees, cols = f->p.num_cols;
    const unsigned blocks_y = (unsigned)((K + kVecClasses - 1) / kVecClasses);  // 1 when K == 1
    if (cols == 0) data = v->leaves;  // every tree is a single leaf: the walk's idle feature read needs one readable float
    const int vec4_ok = (cols % 4 == 0) && ((reinterpret_cast<uintptr_t>(data) & 15u) == 0);
    auto launch = [&](auto kb, auto wl) {
        constexpr int KB = decltype(kb)::value;
        constexpr bool WL = decltype(wl)::value && !STAGED;
        if (csr) {
            if constexpr (!STAGED && !WL)
                hipLaunchKernelGGL((vector_tile_kernel<KB, false, false, true>),
                                   dim3((unsigned)((rows + kTileRows - 1) / kTileRows), blocks_y), dim3(kTileRows),
                                   (size_t)vector_tile_bytes(f), stream, v->nodes, v->roots, v->leaves, data, sums, leaf_out, rows,
                                   cols, T, K, f->p.missing, vec4_ok, stages, S, *csr);
        } else if (strategy == TAHOE_STRATEGY_ROWTILE)
            hipLaunchKernelGGL((vector_tile_kernel<KB, WL, STAGED>), dim3((unsigned)((rows + kTileRows - 1) / kTileRows), blocks_y),
                               dim3(kTileRows), (size_t)vector_tile_bytes(f), stream, v->nodes, v->roots, v->leaves, data, sums,
                               leaf_out, rows, cols, T, K, f->p.missing, vec4_ok, stages, S, CsrView{});
        else
            hipLaunchKernelGGL((vector_direct_kernel<KB, WL, STAGED>), dim3((unsigned)((rows + kBlock - 1) / kBlock), blocks_y),
                               dim3(kBlock), 0, stream, v->nodes, v->roots, v->leaves, data, sums, leaf_out, rows, cols, T, K,
                               f->p.missing, stages, S);
    };
    with_leaf(leaf_out != nullptr, [&](auto wl) {
        if (K == 1) launch(std::integral_constant<int, 1>{}, wl);
        else launch(std::integral_constant<int, kVecClasses>{}, wl);
    });
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

tahoe_status vector_launch(tahoe_forest *f, float *sums, uint32_t *leaf_out, const float *data, size_t rows, hipStream_t stream,
                           int strategy, const CsrView *csr)
{
    return vector_launch_as<false>(f, sums, leaf_out, data, rows, stream, strategy, csr);
}

tahoe_status vector_launch_staged(tahoe_forest *f, float *out, const float *data, size_t rows, hipStream_t stream, int strategy)
{
    return vector_launch_as<true>(f, out, nullptr, data, rows, stream, strategy);
}

void vector_destroy(tahoe_forest *f)
{
    tahoe_vstate *v = f->vl;
    if (!v) return;
    interventional_destroy(f);  // the background of a handle created with TAHOE_CREATE_INTERVENTIONAL
    vector_shap_destroy(f);
    vector_approx_destroy(f);
    if (v->nodes) (void)hipFree(v->nodes);
    if (v->roots) (void)hipFree(v->roots);
    if (v->leaves) (void)hipFree(v->leaves);
    delete v;
    f->vl = nullptr;
}

// The tile kernels may need more than the default 64 KiB of dynamic LDS
static tahoe_status vector_allow_lds(const tahoe_forest *f)
{
    hipError_t e = hipSuccess;
    if (vector_tile_fits(f) &&
        ((e = allow_max_lds_leaf([](auto wl) { return &vector_tile_kernel<1, decltype(wl)::value>; }, f->lds_limit)) != hipSuccess ||
         (e = allow_max_lds_leaf([](auto wl) { return &vector_tile_kernel<kVecClasses, decltype(wl)::value>; }, f->lds_limit)) != hipSuccess))
        return hip_status(e, "hipFuncSetAttribute(vector_tile)");
    if (f->csr && vector_tile_fits(f)) {  // the CSR-loader instantiation (tahoe_forest_predict_csr) of this handle's K
        const void *fn = f->num_classes == 1 ? reinterpret_cast<const void *>(&vector_tile_kernel<1, false, false, true>)
                                             : reinterpret_cast<const void *>(&vector_tile_kernel<kVecClasses, false, false, true>);
        return hip_status(allow_max_lds(fn, f->lds_limit), "hipFuncSetAttribute(vector_tile, csr)");
    }
    return TAHOE_OK;
}

// ... and so may the staged ones of this handle (tahoe_forest_set_stages calls it)
tahoe_status vector_allow_staged_lds(const tahoe_forest *f)
{
    if (!vector_tile_fits(f)) return TAHOE_OK;
    const void *fn = f->num_classes == 1 ? reinterpret_cast<const void *>(&vector_tile_kernel<1, false, true>)
                                         : reinterpret_cast<const void *>(&vector_tile_kernel<kVecClasses, false, true>);
    return hip_status(allow_max_lds(fn, f->lds_limit), "hipFuncSetAttribute(vector_tile, staged)");
}

}  // namespace tahoe

using namespace tahoe;

extern "C" tahoe_status tahoe_vector_forest_create_ex(tahoe_forest **out, const int32_t *trees, const tahoe_sparse_node *nodes,
                                                      const float *leaf_values, int64_t num_leaf_vectors, const float *covers,
                                                      const tahoe_forest_params *p, int leaf_dim, unsigned flags)
{
    // every check here runs before a device is touched
    if (!out || !p) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_vector_forest_create: null argument");
    *out = nullptr;
    if (p->num_trees < 0) return fail(TAHOE_ERR_INVALID_ARG, "num_trees must be non-negative");
    if (p->num_nodes < 0) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_vector_forest_create: num_nodes must be non-negative");
    if (num_leaf_vectors < 0)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_vector_forest_create: num_leaf_vectors must be non-negative, got %lld",
                    (long long)num_leaf_vectors);
    if (leaf_dim < 1 || leaf_dim > 1024)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_vector_forest_create: leaf_dim must be in [1,1024], got %d", leaf_dim);
    if (const tahoe_status s = check_params(p, leaf_dim, trees && nodes, "trees / nodes")) return s;
    if (num_leaf_vectors > 0 && !leaf_values) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_vector_forest_create: leaf_values is null");
    tahoe_forest_params any_trees = *p;
    any_trees.num_trees = 0;  // every tree feeds every class: no multiple-of-classes rule, only the output bits
    if (const tahoe_status s = check_classes(&any_trees, leaf_dim)) return s;
    if ((unsigned long long)num_leaf_vectors > SIZE_MAX / sizeof(float) / (unsigned)leaf_dim)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_vector_forest_create: num_leaf_vectors x leaf_dim floats overflow size_t");

    // Structure check, as tahoe_sparse_forest_create's: roots ascending, every child pair inside its tree and after its parent
    // (which also rules out cycles, so device walks terminate), fid < num_cols; and every leaf names a vector of the table.
    const int T = p->num_trees;
    std::vector<VNode> h_nodes((size_t)p->num_nodes, VNode{0.0f, kVIsLeaf, 0u, 0u});  // (nodes outside every tree are never read)
    std::vector<int> level;
    int max_depth = 0;
    for (int t = 0; t < T; ++t) {
        const long long lo = trees[t], hi = (t + 1 < T) ? trees[t + 1] : p->num_nodes;
        if (lo < 0 || hi <= lo || hi > p->num_nodes)
            return fail(TAHOE_ERR_INVALID_FOREST, "tree %d: root offsets must be ascending and inside [0, num_nodes)", t);
        level.assign((size_t)(hi - lo), 0);  // (children come after their parent: one forward pass gives every node's level)
        for (long long i = 0; i < hi - lo; ++i) {
            const tahoe_sparse_node &n = nodes[lo + i];
            const uint32_t bits = (uint32_t)n.bits;
            if (bits & kVIsLeaf) {
                if (n.left_idx < 0 || (long long)n.left_idx >= (long long)num_leaf_vectors)
                    return fail(TAHOE_ERR_INVALID_FOREST, "tree %d node %lld: leaf vector %d is outside [0, %lld)", t, i, n.left_idx,
                                (long long)num_leaf_vectors);
                h_nodes[(size_t)(lo + i)] = VNode{0.0f, kVIsLeaf, (uint32_t)n.left_idx, 0u};
                max_depth = std::max(max_depth, level[(size_t)i]);
                continue;
            }
            if (n.left_idx <= i || (long long)n.left_idx + 1 >= hi - lo)
                return fail(TAHOE_ERR_INVALID_FOREST, "tree %d node %lld: children %d, %d are not after the node and inside the tree", t,
                            i, n.left_idx, n.left_idx + 1);
            if ((bits & kVFidMask) >= (uint32_t)p->num_cols)
                return fail(TAHOE_ERR_INVALID_FOREST, "tree %d node %lld: fid %u >= num_cols %d", t, i, bits & kVFidMask, p->num_cols);
            h_nodes[(size_t)(lo + i)] = VNode{n.val, bits, (uint32_t)n.left_idx, 0u};
            level[(size_t)n.left_idx] = level[(size_t)n.left_idx + 1] = level[(size_t)i] + 1;
        }
    }
    // the checks of tahoe_sparse_forest_create_ex for the flags: covers (TAHOE_CREATE_CONTRIBS; TAHOE_CREATE_INTERVENTIONAL alone
    // reads none), and at most 31 distinct features on a leaf's path
    // (TAHOE_CREATE_STAGED opens tahoe_forest_set_stages / _predict_staged, reads no cover and builds no table; TAHOE_CREATE_CSR
    // opens tahoe_forest_predict_csr / _reserve_csr / _get_csr_plan in the same way)
    const bool staged = (flags & TAHOE_CREATE_STAGED) != 0, csr_rows = (flags & TAHOE_CREATE_CSR) != 0;
    flags &= ~(unsigned)(TAHOE_CREATE_STAGED | TAHOE_CREATE_CSR);
    constexpr unsigned kShapFlags = TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_INTERVENTIONAL | TAHOE_CREATE_VECTOR_INTERACTIONS;
    if (const tahoe_status s = check_nan_missing_flags(flags, "a vector-leaf")) return s;
    if ((flags & ~(kShapFlags | TAHOE_CREATE_VECTOR_APPROX)) != 0)
        return fail(TAHOE_ERR_INVALID_ARG,
                    "unknown create flags 0x%x (a vector-leaf handle takes TAHOE_CREATE_CONTRIBS, TAHOE_CREATE_INTERVENTIONAL, "
                    "TAHOE_CREATE_VECTOR_INTERACTIONS and TAHOE_CREATE_VECTOR_APPROX only)",
                    flags & ~(kShapFlags | TAHOE_CREATE_VECTOR_APPROX));
    // interaction values take phi from the TreeSHAP pass and the covers' zero fractions: no meaning without TAHOE_CREATE_CONTRIBS
    if ((flags & TAHOE_CREATE_VECTOR_INTERACTIONS) != 0 && (flags & TAHOE_CREATE_CONTRIBS) == 0)
        return fail(TAHOE_ERR_INVALID_ARG, "TAHOE_CREATE_VECTOR_INTERACTIONS needs TAHOE_CREATE_CONTRIBS (and covers) in the same call");
    const bool with_covers = (flags & TAHOE_CREATE_CONTRIBS) != 0;
    if (with_covers && !covers) return fail(TAHOE_ERR_INVALID_ARG, "TAHOE_CREATE_CONTRIBS needs covers (one per node)");
    // Saabas deltas (TAHOE_CREATE_VECTOR_APPROX) read the covers and no path: alone, the covers are checked and no length is
    const bool approx = (flags & TAHOE_CREATE_VECTOR_APPROX) != 0;
    if (approx && !covers) return fail(TAHOE_ERR_INVALID_ARG, "TAHOE_CREATE_VECTOR_APPROX needs covers (one per node)");
    if (flags & kShapFlags) {
        if (const tahoe_status cs = contribs_validate_sparse(trees, nodes, covers, p, true, with_covers || approx)) return cs;
    } else if (approx) {
        if (const tahoe_status cs = contribs_validate_sparse(trees, nodes, covers, p, false)) return cs;
    }

    ForestPtr f;
    if (const tahoe_status s = open_handle(p, leaf_dim, f)) return s;
    f->class_trees = T;  // AVG divides by (float)num_trees whatever K is
    f->p.depth = f->depth = max_depth;
    f->bits_bytes = 4;
    f->staged = staged;
    f->csr = csr_rows;
    f->vl = new (std::nothrow) tahoe_vstate();
    if (!f->vl) return fail(TAHOE_ERR_NO_MEMORY, "tahoe_vector_forest_create");
    tahoe_vstate *v = f->vl;
    tahoe_status s = TAHOE_OK;
    if ((s = hip_status(upload(&v->nodes, h_nodes, &f->device_bytes), "upload(nodes)")) ||
        (s = hip_status(upload(&v->roots, trees, (size_t)T, &f->device_bytes), "upload(roots)")) ||
        (s = hip_status(upload(&v->leaves, leaf_values, (size_t)num_leaf_vectors * (size_t)leaf_dim, &f->device_bytes), "upload(leaves)")) ||
        (s = vector_allow_lds(f.get())))
        return s;
    if ((flags & kShapFlags) && (s = vector_shap_build(f.get(), trees, nodes, leaf_values, with_covers ? covers : nullptr, flags)))
        return s;
    if (approx && (s = vector_approx_build(f.get(), trees, nodes, leaf_values, covers))) return s;
    *out = f.release();
    return TAHOE_OK;
}

extern "C" tahoe_status tahoe_vector_forest_create(tahoe_forest **out, const int32_t *trees, const tahoe_sparse_node *nodes,
                                                   const float *leaf_values, int64_t num_leaf_vectors, const tahoe_forest_params *p,
                                                   int leaf_dim)
{
    return tahoe_vector_forest_create_ex(out, trees, nodes, leaf_values, num_leaf_vectors, nullptr, p, leaf_dim, 0u);
}
