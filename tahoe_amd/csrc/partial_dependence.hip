// Partial dependence on sparse forests (TAHOE_CREATE_PARTIAL_DEPENDENCE, tahoe_forest_predict_partial_dependence): what
// scikit-learn's partial_dependence(method="recursion") computes.  A grid point gives values to the target features only.  At a
// split on a target it takes predict's branch; at any other split it goes down BOTH children, each weighted by its share of the
// node's cover, and the tree's value is the weighted sum of the leaves it reaches ("Partial dependence").
//
// The bits are specified (include/tahoe_amd.h): per internal node fl = cl / (cl + cr) and fr = cr / (cl + cr) in float32, built
// here on the host; the walk multiplies the weight by fl or fr once per non-target split, adds w * val per leaf in depth-first
// order, left before right, and never visits a child whose fraction is 0.0f.  Every product and every sum is one float32
// operation: __fmul_rn / __fadd_rn, which no contraction can fuse (the library is also built with -ffp-contract=off).
//
// Kernels:
//   pd_walk_kernel  one wave = 64 consecutive grid points x one tree; the kPdWaves waves of a workgroup take consecutive trees and
//                   share the 64 points' target values in LDS.  The right siblings a lane has still to visit wait on a stack of
//                   (node, weight) pairs in LDS, [slot][lane] (16 KiB per wave: a lane's slot s is one ds_read_b64 / ds_write_b64
//                   at a lane-linear address, no bank conflict); create() bounds its depth.  Tree values go to ws[tree][point].
//   pd_sum_kernel   one thread per (grid point, class): adds the class's tree values in tree order, 16 loads in flight.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "forest_internal.h"

struct tahoe_pdstate {
    float2 *frac = nullptr;  // per stored node (the order of the handle's device nodes): {fl, fr}; {0, 0} at a leaf
    float *ws = nullptr;     // [num_trees][chunk] tree values of one chunk of grid points
    size_t chunk = 0;        // grid points per chunk: a multiple of 64
};

namespace tahoe {

constexpr int kPdWaves = 4;         // waves (consecutive trees) per workgroup
constexpr int kPdStack = 32;        // pending right siblings per lane = the deepest leaf create() accepts, in edges
constexpr int kPdMaxTargets = 32;
constexpr int kPdSumThreads = 256;
constexpr size_t kPdWorkspaceBytes = (size_t)32 << 20;  // the default chunk keeps 4 T chunk near this

constexpr int32_t kPdIsLeaf = (int32_t)(1u << 31);
constexpr int32_t kPdDefLeft = (int32_t)(1u << 30);
constexpr int32_t kPdFidMask = (int32_t)((1u << 30) - 1u);

// The call's targets, as kernel arguments: n column ids, wave-uniform
struct PdTargets {
    int32_t n;
    int32_t id[kPdMaxTargets];
};

// CAT (a handle with categorical splits): a node flagged kSCat takes go_right_cat on the pool entry its `val` bits name.
// `grid` points at the chunk's first grid point, rows = the chunk's grid points, tiles = ceil(rows / 64); workgroup b walks tile
// b % tiles through trees kPdWaves * (b / tiles) ...
template <bool CAT>
__global__ void __launch_bounds__(kPdWaves * 64) pd_walk_kernel(const tahoe_sparse_node *__restrict__ nodes,
                                                                const int32_t *__restrict__ trees, const float2 *__restrict__ frac,
                                                                const uint32_t *__restrict__ cat_pool, uint32_t cat_words,
                                                                const float *__restrict__ grid, size_t rows, unsigned tiles,
                                                                int num_trees, float missing, PdTargets tg, float *__restrict__ ws,
                                                                size_t ws_stride)
{
    __shared__ float xs[kPdMaxTargets * 64];                  // [target][point of the tile]
    __shared__ uint2 stack[kPdWaves][kPdStack * 64];          // per wave [slot][lane]: {node, weight bits}
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned tile = blockIdx.x % tiles;
    const int t = (int)(blockIdx.x / tiles) * kPdWaves + wave;
    const size_t row0 = (size_t)tile * 64;
    const int nt = tg.n;
    {   // the tile's rows are one contiguous run of the row-major grid
        const float *src = grid + row0 * (size_t)nt;
        const size_t have = (min(rows, row0 + 64) - row0) * (size_t)nt;
        for (int e = threadIdx.x; e < nt * 64; e += kPdWaves * 64) xs[(e % nt) * 64 + e / nt] = (size_t)e < have ? src[e] : 0.0f;
    }
    __syncthreads();
    if (t >= num_trees) return;
    const size_t base = (size_t)trees[t];
    const tahoe_sparse_node *root = nodes + base;
    const float2 *fr = frac + base;
    uint2 *stk = &stack[wave][lane];
    uint32_t node = 0u;
    float w = 1.0f, acc = 0.0f;
    int sp = 0;
    for (;;) {  // create() guarantees children after their parent and inside the tree: the walk terminates
        const tahoe_sparse_node n = root[node];
        const float2 f2 = fr[node];  // beside the node: one round trip per step
        bool pop = false;
        if (n.bits & kPdIsLeaf) {
            acc = __fadd_rn(acc, __fmul_rn(w, n.val));
            pop = true;
        } else {
            const int fid = n.bits & (CAT ? kSCatFidMask : kPdFidMask);
            int ti = -1;
            for (int j = 0; j < nt; ++j) ti = tg.id[j] == fid ? j : ti;
            const uint32_t left = (uint32_t)n.left_idx;
            if (ti >= 0) {  // a target: predict's branch for the grid value, the weight unchanged
                const float x = xs[ti * 64 + lane];
                const bool def_left = (n.bits & kPdDefLeft) != 0;
                if (CAT && (n.bits & kSCat)) node = left + go_right_cat(x, cat_pool, __float_as_uint(n.val), cat_words, def_left, missing);
                else node = left + go_right(x, n.val, def_left, missing);
            } else if (f2.x != 0.0f) {  // left now; the right sibling waits
                if (f2.y != 0.0f && sp < kPdStack) {  // (create() refuses a leaf deeper than kPdStack edges: sp < kPdStack here)
                    stk[sp * 64] = make_uint2(left + 1u, __float_as_uint(__fmul_rn(w, f2.y)));
                    ++sp;
                }
                node = left;
                w = __fmul_rn(w, f2.x);
            } else if (f2.y != 0.0f) {
                node = left + 1u;
                w = __fmul_rn(w, f2.y);
            } else {
                pop = true;  // (no cover below: unreachable after create()'s positive-sum check)
            }
        }
        if (pop) {
            if (sp == 0) break;
            --sp;
            const uint2 e = stk[sp * 64];
            node = e.x;
            w = __uint_as_float(e.y);
        }
    }
    if (row0 + lane < rows) ws[(size_t)t * ws_stride + row0 + lane] = acc;
}

// pd[g][c] = the float32 sum from +0.0f of ws[c * class_trees + j][g], j ascending (the stored trees are class-major: that is
// class c's trees in the caller's order).  Thread i: point i % rows of class i / rows.
__global__ void __launch_bounds__(kPdSumThreads) pd_sum_kernel(const float *__restrict__ ws, size_t ws_stride, int class_trees,
                                                               int num_classes, float *__restrict__ pd, size_t rows)
{
    const size_t i = (size_t)blockIdx.x * kPdSumThreads + threadIdx.x;
    if (i >= rows * (size_t)num_classes) return;
    const size_t g = i % rows, c = i / rows;
    const float *p = ws + c * (size_t)class_trees * ws_stride + g;
    float sum = 0.0f;
    int j = 0;
    for (; j + 16 <= class_trees; j += 16) {  // 16 loads in flight, 16 adds in tree order
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = p[(size_t)(j + k) * ws_stride];
#pragma unroll
        for (int k = 0; k < 16; ++k) sum = __fadd_rn(sum, v[k]);
    }
    for (; j < class_trees; ++j) sum = __fadd_rn(sum, p[(size_t)j * ws_stride]);
    pd[g * (size_t)num_classes + c] = sum;
}

// The checks of TAHOE_CREATE_PARTIAL_DEPENDENCE on the caller's trees, before a device is touched
tahoe_status pd_validate_sparse(const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers, const tahoe_forest_params *p)
{
    struct Frame {
        int32_t node;
        int depth;
    };
    std::vector<Frame> stack;
    for (int t = 0; t < p->num_trees; ++t) {
        const tahoe_sparse_node *tn = nodes + trees[t];
        const float *tc = covers + trees[t];
        stack.assign(1, Frame{0, 0});
        while (!stack.empty()) {
            const Frame fr = stack.back();
            stack.pop_back();
            const tahoe_sparse_node &n = tn[fr.node];
            if (fr.depth > kPdStack)  // a leaf, or a node above one
                return fail(TAHOE_ERR_UNSUPPORTED, "tree %d: a leaf lies more than %d edges below the root "
                                                   "(TAHOE_CREATE_PARTIAL_DEPENDENCE: the depth of its walk's stack)", t, kPdStack);
            if (n.bits & kPdIsLeaf) continue;
            const float wl = tc[n.left_idx], wr = tc[n.left_idx + 1];
            if (!std::isfinite(wl) || !std::isfinite(wr) || !(wl >= 0.0f) || !(wr >= 0.0f) || !((double)wl + (double)wr > 0.0))
                return fail(TAHOE_ERR_INVALID_FOREST,
                            "tree %d node %d: child covers %g and %g (TAHOE_CREATE_PARTIAL_DEPENDENCE needs finite covers >= 0 with a "
                            "positive sum at every reachable internal node)", t, fr.node, (double)wl, (double)wr);
            const float tot = wl + wr;  // the float32 sum the fractions divide by
            if (!std::isfinite(tot))
                return fail(TAHOE_ERR_INVALID_FOREST, "tree %d node %d: the float32 sum of the child covers %g and %g is not finite "
                                                      "(TAHOE_CREATE_PARTIAL_DEPENDENCE)", t, fr.node, (double)wl, (double)wr);
            stack.push_back(Frame{n.left_idx + 1, fr.depth + 1});
            stack.push_back(Frame{n.left_idx, fr.depth + 1});
        }
    }
    return TAHOE_OK;
}

// The fraction table (in the stored node order) and the workspace of a validated forest
tahoe_status pd_build_sparse(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers)
{
    tahoe_pdstate *pd = new (std::nothrow) tahoe_pdstate();
    if (!pd) return fail(TAHOE_ERR_NO_MEMORY, "pd_build_sparse");
    f->pd = pd;
    const int T = f->p.num_trees, C = f->num_classes, Tc = f->class_trees;
    const size_t N = (size_t)f->p.num_nodes;
    std::vector<float2> fr(N, make_float2(0.0f, 0.0f));  // the caller's numbering
    for (int t = 0; t < T; ++t) {
        const size_t a = (size_t)trees[t], b = t + 1 < T ? (size_t)trees[t + 1] : N;
        for (size_t i = a; i < b; ++i) {
            if (nodes[i].bits & kPdIsLeaf) continue;
            const size_t l = a + (size_t)nodes[i].left_idx;
            const float cl = covers[l], cr = covers[l + 1];
            const float tot = cl + cr;  // three IEEE float32 operations, each rounded once
            fr[i] = make_float2(cl / tot, cr / tot);
        }
    }
    std::vector<float2> stored;
    if (C > 1) {  // class-major, each tree's node range moved as a block (create_sparse)
        for (int q = 0; q < T; ++q) {
            const int t = (q % Tc) * C + q / Tc;
            const size_t a = (size_t)trees[t], b = t + 1 < T ? (size_t)trees[t + 1] : N;
            stored.insert(stored.end(), fr.begin() + a, fr.begin() + b);
        }
    } else {
        stored.swap(fr);
    }
    if (const tahoe_status s = hip_status(upload(&pd->frac, stored, &f->device_bytes), "upload(partial dependence fractions)")) return s;
    // the chunk: TAHOE_PD_CHUNK_ROWS rounded up to whole 64-point tiles, or what keeps the workspace near kPdWorkspaceBytes; at
    // most 2^34 tree values, so that every launch's workgroup count stays far below 2^31
    const size_t Tn = (size_t)std::max(T, 1);
    size_t chunk = f->knobs.pd_chunk_rows > 0 ? (size_t)f->knobs.pd_chunk_rows : kPdWorkspaceBytes / (4 * Tn);
    chunk = std::min(chunk, ((size_t)1 << 34) / Tn);
    chunk = std::max<size_t>((chunk + (f->knobs.pd_chunk_rows > 0 ? 63 : 0)) / 64 * 64, 64);
    pd->chunk = chunk;
    const size_t bytes = 4 * Tn * chunk;
    if (const tahoe_status s = hip_status(hipMalloc(reinterpret_cast<void **>(&pd->ws), bytes), "hipMalloc(partial dependence workspace)"))
        return s;
    f->device_bytes += bytes;
    return TAHOE_OK;
}

void pd_destroy(tahoe_forest *f)
{
    tahoe_pdstate *pd = f->pd;
    if (!pd) return;
    if (pd->frac) (void)hipFree(pd->frac);
    if (pd->ws) (void)hipFree(pd->ws);
    delete pd;
    f->pd = nullptr;
}

}  // namespace tahoe

using namespace tahoe;

extern "C" tahoe_status tahoe_forest_predict_partial_dependence(tahoe_forest *f, float *pd_dev, const int32_t *targets, int num_targets,
                                                                const float *grid_dev, size_t grid_rows, void *stream)
{
    const char *fn = "tahoe_forest_predict_partial_dependence";
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "%s: null forest", fn);
    if (const tahoe_status s = refuse_oblivious(f, fn)) return s;
    if (const tahoe_status s = refuse_vector(f, fn)) return s;
    if (!f->sp)
        return fail(TAHOE_ERR_UNSUPPORTED, "%s: not served on a %s handle (a dense model goes through tahoe_dense_to_sparse_ex and "
                                           "tahoe_sparse_forest_create_ex)", fn, f->num_classes > 1 ? "multi-class dense" : "dense");
    if (!f->pd)
        return fail(TAHOE_ERR_UNSUPPORTED, "%s: the sparse handle was created without TAHOE_CREATE_PARTIAL_DEPENDENCE and has no "
                                           "cover fractions and no workspace", fn);
    if (num_targets < 0 || num_targets > kPdMaxTargets)
        return fail(TAHOE_ERR_INVALID_ARG, "%s: num_targets %d is not in [0, %d]", fn, num_targets, kPdMaxTargets);
    if (num_targets > 0 && !targets) return fail(TAHOE_ERR_INVALID_ARG, "%s: targets is NULL with num_targets %d", fn, num_targets);
    PdTargets tg{};
    tg.n = num_targets;
    for (int j = 0; j < num_targets; ++j) {
        if (targets[j] < 0 || targets[j] >= f->p.num_cols)
            return fail(TAHOE_ERR_INVALID_ARG, "%s: targets[%d] = %d is outside [0, num_cols = %d)", fn, j, targets[j], f->p.num_cols);
        for (int k = 0; k < j; ++k)
            if (targets[k] == targets[j])
                return fail(TAHOE_ERR_INVALID_ARG, "%s: targets[%d] = %d repeats targets[%d]", fn, j, targets[j], k);
        tg.id[j] = targets[j];
    }
    if (grid_rows == 0) return TAHOE_OK;
    if (!pd_dev || (num_targets > 0 && !grid_dev)) return fail(TAHOE_ERR_INVALID_ARG, "%s: null argument (pd_dev or grid_dev)", fn);
    const size_t limit = SIZE_MAX / sizeof(float), C = (size_t)f->num_classes;
    if (grid_rows > limit / C || (num_targets > 0 && grid_rows > limit / (size_t)num_targets))
        return fail(TAHOE_ERR_INVALID_ARG, "%s: grid_rows x num_targets or grid_rows x classes floats overflow size_t (grid_rows %zu)",
                    fn, grid_rows);
    const tahoe_pdstate *pd = f->pd;
    DeviceGuard on_device(f->device);
    hipStream_t s = (hipStream_t)stream;
    const tahoe_sparse_node *sn = nullptr;
    const int32_t *st = nullptr;
    const uint32_t *cat_pool = nullptr;
    uint32_t cat_words = 0;
    sparse_device_views(f, &sn, &st);
    sparse_cat_view(f, &cat_pool, &cat_words);
    const int T = f->p.num_trees;
    const unsigned tree_blocks = (unsigned)((T + kPdWaves - 1) / kPdWaves);
    for (size_t row0 = 0; row0 < grid_rows; row0 += pd->chunk) {  // chunk after chunk, in stream order, through the one workspace
        const size_t n = std::min(pd->chunk, grid_rows - row0);
        const unsigned tiles = (unsigned)((n + 63) / 64);
        const float *g = num_targets > 0 ? grid_dev + row0 * (size_t)num_targets : nullptr;
        const dim3 wgrid(tiles * tree_blocks), wblock(kPdWaves * 64);
        if (T == 0)
            ;  // no trees, no walk (HIP refuses a grid of 0 workgroups): the sum over no trees below writes +0.0f
        else if (cat_pool)
            hipLaunchKernelGGL((pd_walk_kernel<true>), wgrid, wblock, 0, s, sn, st, pd->frac, cat_pool, cat_words, g, n, tiles, T,
                               f->p.missing, tg, pd->ws, pd->chunk);
        else
            hipLaunchKernelGGL((pd_walk_kernel<false>), wgrid, wblock, 0, s, sn, st, pd->frac, nullptr, 0u, g, n, tiles, T, f->p.missing,
                               tg, pd->ws, pd->chunk);
        TAHOE_HIP_TRY(hipGetLastError());
        const dim3 sgrid((unsigned)((n * C + kPdSumThreads - 1) / kPdSumThreads));
        hipLaunchKernelGGL(pd_sum_kernel, sgrid, dim3(kPdSumThreads), 0, s, pd->ws, pd->chunk, f->class_trees, f->num_classes,
                           pd_dev + row0 * C, n);
        TAHOE_HIP_TRY(hipGetLastError());
    }
    return TAHOE_OK;
}
