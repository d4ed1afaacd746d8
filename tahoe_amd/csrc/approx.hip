// Saabas contributions (XGBoost approx_contribs): per (row, tree) one root-to-leaf walk that adds, at every internal node on the
// path, the change of the node mean along the branch taken to the node's feature.  Create (TAHOE_CREATE_APPROX_CONTRIBS) computes
// the node means in float64 on the host and stores each child's delta next to its parent's split:
//   dense   recs[p][n_inner] uint4 {thr, meta, d_left, d_right} per normalised heap node of internal tree p (class-major, after
//           re-layout: the deltas move with the swapped children and the exchange bit inverts the decision, as in go_right_meta);
//           meta = fid (29 bits) | pad << 29 | exchange << 30 | def_left << 31, pad = the normalisation below a shallow leaf
//   sparse  dd[node] float2 {d(left_idx), d(left_idx + 1)} parallel to the stored sparse nodes
// Kernel: lane = row, each lane walks its row's trees in order, so the float32 sums need no exchange between lanes.  The row's
// accumulator is a private row of an LDS slab (SLAB) or its own row of phi_dev (wide rows); whole rows are written at the end of
// every class with the AVG division and the bias column.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "forest_internal.h"

struct tahoe_astate {
    uint4 *recs = nullptr;   // dense: [T][n_inner] records
    float2 *dd = nullptr;    // sparse: [num_nodes] child deltas, parallel to the stored nodes
    float *bias = nullptr;   // [C] the bias column of tahoe_forest_predict_contribs
    float *div = nullptr;    // [C] (float)Tc with TAHOE_OUT_AVG, else 1.0f
    bool slab = false;       // accumulate in LDS (else in place in phi_dev)
    int waves = 1;           // waves (64 rows each) per workgroup
    int stride = 0;          // floats per slab row: num_cols + 1 made odd (a lane's row starts on its own bank)
    size_t lds_bytes = 0;    // per workgroup
};

namespace tahoe {

constexpr uint32_t kApproxFidMask = 0x1fffffffu;
constexpr uint32_t kApproxPad = 1u << 29;
constexpr int kApproxMaxCols = 1 << 29;
constexpr size_t kApproxSlabBudget = 64 * 1024;  // LDS per workgroup of the slab form when several waves' slabs fit

// One wave's rows of the workgroup: zero the accumulators of class c, walk class c's trees, write the rows out.  Every wave of
// the workgroup runs the same class loop, so the barriers are uniform.
// CAT (a sparse handle with categorical splits): a node flagged kSCat takes go_right_cat on the pool entry its `val` bits name,
// as sparse_kernel does; the deltas are per child whatever the split's kind.  The pool and its length come in the two arguments
// that only the dense form reads (recs, depth): this kernel reads blockDim, a hidden argument that lies behind the declared ones,
// so an appended argument would change an immediate in every existing instantiation.
template <bool SPARSE, bool SLAB, bool CAT = false>
__global__ __launch_bounds__(256) void approx_kernel(float *__restrict__ phi, const float *__restrict__ data, size_t rows, int F,
                                                     int C, int Tc, int depth, const uint4 *__restrict__ recs,
                                                     const tahoe_sparse_node *__restrict__ snodes, const int32_t *__restrict__ strees,
                                                     const float2 *__restrict__ dd, const float *__restrict__ bias,
                                                     const float *__restrict__ div, float missing, int stride)
{
    static_assert(SPARSE || !CAT, "categorical splits exist on sparse handles only");
    const uint32_t *__restrict__ cat_pool = reinterpret_cast<const uint32_t *>(recs);  // CAT only
    const uint32_t cat_words = (uint32_t)depth;
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const size_t row0 = ((size_t)blockIdx.x * (blockDim.x >> 6) + wave) * 64;  // this wave's first row
    const size_t row = row0 + lane;
    const bool row_ok = row < rows;
    const int nr = row0 < rows ? (int)std::min<size_t>(64, rows - row0) : 0;
    const size_t F1 = (size_t)F + 1, out_row = (size_t)C * F1;
    const float *x = data + (row_ok ? row : 0) * (size_t)F;
    float *wslab = SLAB ? slab + (size_t)wave * 64 * stride : nullptr;
    const size_t n_inner = ((size_t)1 << (CAT ? 0 : depth)) - 1;  // (CAT: depth carries the pool length)
    for (int c = 0; c < C; ++c) {
        // ---- zero the accumulators ----
        if (SLAB) {
            for (int i = 0; i < F; ++i) wslab[lane * stride + i] = 0.0f;  // odd stride: the 64 lanes hit 64 banks
        } else {
            for (int r = 0; r < nr; ++r)
                for (int i = lane; i < F; i += 64) phi[(row0 + r) * out_row + (size_t)c * F1 + i] = 0.0f;
            __syncthreads();
        }
        float *acc = SLAB ? wslab + lane * stride : phi + (row_ok ? row : 0) * out_row + (size_t)c * F1;
        // ---- the walks, tree order, root to leaf ----
        if (row_ok) {
            for (int k = 0; k < Tc; ++k) {
                const int p = c * Tc + k;
                if (SPARSE) {
                    const tahoe_sparse_node *tn = snodes + strees[p];
                    const float2 *td = dd + strees[p];
                    int32_t i = 0;
                    for (;;) {
                        const tahoe_sparse_node n = tn[i];
                        if (n.bits < 0) break;  // a leaf
                        const float2 d = td[i];
                        const int fid = n.bits & (CAT ? kSCatFidMask : 0x3fffffff);
                        const uint32_t r = (CAT && (n.bits & kSCat))
                                               ? go_right_cat(x[fid], cat_pool, __float_as_uint(n.val), cat_words, ((uint32_t)n.bits >> 30) & 1u, missing)
                                               : go_right(x[fid], n.val, ((uint32_t)n.bits >> 30) & 1u, missing);
                        acc[fid] += r ? d.y : d.x;
                        i = n.left_idx + (int32_t)r;
                    }
                } else {
                    const uint4 *t = recs + (size_t)p * n_inner;
                    uint32_t i = 0;
                    for (int l = 0; l < depth; ++l) {
                        const uint4 n = t[i];
                        if (n.y & kApproxPad) break;  // padding below a leaf (its whole subtree is padding)
                        const uint32_t fid = n.y & kApproxFidMask;
                        const uint32_t r = go_right_meta(x[fid], __uint_as_float(n.x), n.y, missing);
                        acc[fid] += __uint_as_float(r ? n.w : n.z);
                        i = 2u * i + 1u + r;
                    }
                }
            }
        }
        __syncthreads();
        // ---- whole rows out: the AVG division and the bias column ----
        const float dv = div[c], b = bias[c];
        for (int r = 0; r < nr; ++r) {
            float *o = phi + (row0 + r) * out_row + (size_t)c * F1;
            for (int i = lane; i < F; i += 64) {
                const float v = SLAB ? wslab[r * stride + i] : o[i];
                o[i] = v / dv;
            }
            if (lane == 0) o[F] = b;
        }
        if (SLAB) __syncthreads();  // the slab is zeroed again for the next class
    }
}

static tahoe_status finish_build(tahoe_forest *f, tahoe_astate *ap, const std::vector<float> &h_bias, const std::vector<float> &h_div)
{
    const int F = f->p.num_cols;
    ap->stride = (F + 1) | 1;
    const size_t wave_bytes = (size_t)64 * ap->stride * sizeof(float);
    // the slab while two waves' slabs fit a CU: on K3 (F = 256, one 66-KB wave slab per workgroup) it takes 258 ms per 1 M rows
    // against 581 ms in place (profiles/approx_contribs), the read-modify-write of phi_dev costing more than the lost occupancy
    ap->slab = 2 * wave_bytes <= (size_t)f->lds_limit;
    if (f->knobs.approx_form == 1) ap->slab = wave_bytes <= (size_t)f->lds_limit;  // TAHOE_APPROX_FORM
    if (f->knobs.approx_form == 2) ap->slab = false;
    ap->waves = ap->slab ? (int)std::max<size_t>(1, std::min<size_t>(4, kApproxSlabBudget / wave_bytes)) : 4;
    ap->lds_bytes = ap->slab ? ap->waves * wave_bytes : 0;
    hipError_t e;
    if ((e = upload(&ap->bias, h_bias, &f->device_bytes)) != hipSuccess || (e = upload(&ap->div, h_div, &f->device_bytes)) != hipSuccess)
        return fail(TAHOE_ERR_HIP, "approx_build: upload failed: %s", hipGetErrorString(e));
    const void *k = sparse_has_cats(f) ? reinterpret_cast<const void *>(&approx_kernel<true, true, true>)
                    : f->sp            ? reinterpret_cast<const void *>(&approx_kernel<true, true>)
                                       : reinterpret_cast<const void *>(&approx_kernel<false, true>);
    if (ap->slab && (e = allow_max_lds(k, f->lds_limit)) != hipSuccess)
        return fail(TAHOE_ERR_HIP, "hipFuncSetAttribute(approx) failed: %s", hipGetErrorString(e));
    return TAHOE_OK;
}

static tahoe_status check_cols(const tahoe_forest *f)
{
    if (f->p.num_cols > kApproxMaxCols)
        return fail(TAHOE_ERR_UNSUPPORTED, "TAHOE_CREATE_APPROX_CONTRIBS supports num_cols <= 2^29 (got %d)", f->p.num_cols);
    return TAHOE_OK;
}

tahoe_status approx_build(tahoe_forest *f, const tahoe_dense_node *nodes, const std::vector<InnerNode> &h_inner,
                          const std::vector<unsigned char> &h_real)
{
    if (tahoe_status s = check_cols(f)) return s;
    tahoe_astate *ap = new (std::nothrow) tahoe_astate();
    if (!ap) return fail(TAHOE_ERR_NO_MEMORY, "approx_build");
    f->ap = ap;
    const size_t T = (size_t)f->p.num_trees, n_inner = f->n_inner;
    const size_t per = (size_t)tahoe_tree_num_nodes(f->p.depth);
    const size_t C = (size_t)f->num_classes, Tc = (size_t)f->class_trees;
    std::vector<uint4> recs(T * n_inner);
    parallel_for(T, 4, [&](size_t lo, size_t hi) {
        std::vector<double> E(per);
        std::vector<size_t> orig(n_inner);
        for (size_t p = lo; p < hi; ++p) {
            const tahoe_dense_node *tree = nodes + (C > 1 ? (p % Tc) * C + p / Tc : p) * per;  // the caller's tree
            // node means, bottom-up over the caller's heap (children after parents); unreachable nodes are never read
            for (size_t i = per; i-- > 0;) {
                if ((tree[i].bits >> 31) & 1) {
                    E[i] = (double)tree[i].val;
                } else if (2 * i + 2 < per) {
                    const double wl = tree[2 * i + 1].weight, wr = tree[2 * i + 2].weight;
                    E[i] = (wl * E[2 * i + 1] + wr * E[2 * i + 2]) / (wl + wr);
                } else {
                    E[i] = 0.0;
                }
            }
            // stored heap position s holds the caller's node orig[s]; an exchange bit swaps the children
            const InnerNode *in = &h_inner[p * n_inner];
            const unsigned char *re = &h_real[p * n_inner];
            uint4 *out = &recs[p * n_inner];
            orig[0] = 0;
            for (size_t s = 0; s < n_inner; ++s) {
                size_t ol = 0, or_ = 0;
                if (re[s]) {
                    const size_t o = orig[s];
                    const bool ex = (in[s].meta & kMetaExchange) != 0;
                    ol = ex ? 2 * o + 2 : 2 * o + 1;
                    or_ = ex ? 2 * o + 1 : 2 * o + 2;
                    const float dl = (float)(E[ol] - E[o]), dr = (float)(E[or_] - E[o]);
                    memcpy(&out[s].x, &in[s].thr, 4);
                    out[s].y = in[s].meta;  // fid < 2^29: bit 29 is free for the pad flag
                    memcpy(&out[s].z, &dl, 4);
                    memcpy(&out[s].w, &dr, 4);
                } else {
                    out[s] = make_uint4(0u, kApproxPad, 0u, 0u);
                }
                if (2 * s + 2 < n_inner) {
                    orig[2 * s + 1] = ol;
                    orig[2 * s + 2] = or_;
                }
            }
        }
    });
    std::vector<float> h_bias, h_div;
    contribs_bias(f, nodes, h_bias, h_div);
    const hipError_t e = upload(&ap->recs, recs, &f->device_bytes);
    if (e != hipSuccess) return fail(TAHOE_ERR_HIP, "approx_build: upload failed: %s", hipGetErrorString(e));
    return finish_build(f, ap, h_bias, h_div);
}

tahoe_status approx_build_sparse(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers)
{
    if (tahoe_status s = check_cols(f)) return s;
    tahoe_astate *ap = new (std::nothrow) tahoe_astate();
    if (!ap) return fail(TAHOE_ERR_NO_MEMORY, "approx_build_sparse");
    f->ap = ap;
    const int T = f->p.num_trees, C = f->num_classes, Tc = f->class_trees;
    const size_t N = (size_t)f->p.num_nodes;
    // child deltas in the caller's numbering; node means bottom-up per tree (children lie after their parent)
    std::vector<float2> dd(N, make_float2(0.0f, 0.0f));
    parallel_for((size_t)T, 16, [&](size_t lo, size_t hi) {
        std::vector<double> E;
        for (size_t t = lo; t < hi; ++t) {
            const size_t a = (size_t)trees[t], b = t + 1 < (size_t)T ? (size_t)trees[t + 1] : N;
            const tahoe_sparse_node *tn = nodes + a;
            const float *tc = covers + a;
            saabas_means(tn, tc, b - a, E, [&](size_t i) { return tn[i].val; });
            for (size_t i = 0; i < b - a; ++i) {
                if (tn[i].bits < 0) continue;
                const size_t l = (size_t)tn[i].left_idx;
                dd[a + i] = make_float2(saabas_delta(E, l, i), saabas_delta(E, l + 1, i));
            }
        }
    });
    // the stored order: a multi-class forest's trees are class-major, each tree's node range moved as a block (create_sparse)
    std::vector<float2> stored;
    if (C > 1) {
        for (int q = 0; q < T; ++q) {
            const int t = (q % Tc) * C + q / Tc;
            const size_t a = (size_t)trees[t], b = t + 1 < T ? (size_t)trees[t + 1] : N;
            stored.insert(stored.end(), dd.begin() + a, dd.begin() + b);
        }
    } else {
        stored.swap(dd);
    }
    std::vector<float> h_bias, h_div;
    contribs_bias_sparse(f, trees, nodes, covers, h_bias, h_div);
    const hipError_t e = upload(&ap->dd, stored, &f->device_bytes);
    if (e != hipSuccess) return fail(TAHOE_ERR_HIP, "approx_build_sparse: upload failed: %s", hipGetErrorString(e));
    return finish_build(f, ap, h_bias, h_div);
}

void approx_destroy(tahoe_forest *f)
{
    tahoe_astate *ap = f->ap;
    if (!ap) return;
    if (ap->recs) (void)hipFree(ap->recs);
    if (ap->dd) (void)hipFree(ap->dd);
    if (ap->bias) (void)hipFree(ap->bias);
    if (ap->div) (void)hipFree(ap->div);
    delete ap;
    f->ap = nullptr;
}

}  // namespace tahoe

using namespace tahoe;

extern "C" tahoe_status tahoe_forest_predict_contribs_approx(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows,
                                                             void *stream)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_contribs_approx: null forest");
    if (oblivious_serves(f, TAHOE_CREATE_APPROX_CONTRIBS))
        return oblivious_predict_shap(f, TAHOE_CREATE_APPROX_CONTRIBS, phi_dev, data_dev, rows, (hipStream_t)stream,
                                      "tahoe_forest_predict_contribs_approx");
    if (vector_serves_approx(f))
        return vector_predict_approx(f, phi_dev, data_dev, rows, (hipStream_t)stream, "tahoe_forest_predict_contribs_approx");
    if (const tahoe_status st = refuse_oblivious(f, "tahoe_forest_predict_contribs_approx")) return st;
    if (const tahoe_status st = refuse_vector(f, "tahoe_forest_predict_contribs_approx")) return st;
    if (!f->ap)
        return fail(TAHOE_ERR_UNSUPPORTED, "tahoe_forest_predict_contribs_approx: the handle was created without "
                                           "TAHOE_CREATE_APPROX_CONTRIBS and has no node deltas");
    if (rows == 0) return TAHOE_OK;
    if (!phi_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_contribs_approx: null argument");
    if (tahoe_status st = check_shap_out(f, rows, 1, "tahoe_forest_predict_contribs_approx")) return st;
    const tahoe_astate *ap = f->ap;
    DeviceGuard on_device(f->device);
    const size_t per_block = (size_t)ap->waves * 64;
    const dim3 grid((unsigned)((rows + per_block - 1) / per_block)), block((unsigned)per_block);
    hipStream_t s = (hipStream_t)stream;
    const int F = f->p.num_cols, Cn = f->num_classes, Tc = f->class_trees;
    const tahoe_sparse_node *sn = nullptr;
    const int32_t *st = nullptr;
    const uint32_t *cat_pool = nullptr;
    uint32_t cat_words = 0;
    if (f->sp) sparse_device_views(f, &sn, &st);
    if (f->sp) sparse_cat_view(f, &cat_pool, &cat_words);
    if (cat_pool && ap->slab)
        hipLaunchKernelGGL((approx_kernel<true, true, true>), grid, block, ap->lds_bytes, s, phi_dev, data_dev, rows, F, Cn, Tc,
                           (int)cat_words, reinterpret_cast<const uint4 *>(cat_pool), sn, st, ap->dd, ap->bias, ap->div, f->p.missing, ap->stride);
    else if (cat_pool)
        hipLaunchKernelGGL((approx_kernel<true, false, true>), grid, block, 0, s, phi_dev, data_dev, rows, F, Cn, Tc, (int)cat_words,
                           reinterpret_cast<const uint4 *>(cat_pool), sn, st, ap->dd, ap->bias, ap->div, f->p.missing, ap->stride);
    else if (f->sp && ap->slab)
        hipLaunchKernelGGL((approx_kernel<true, true>), grid, block, ap->lds_bytes, s, phi_dev, data_dev, rows, F, Cn, Tc, 0, nullptr,
                           sn, st, ap->dd, ap->bias, ap->div, f->p.missing, ap->stride);
    else if (f->sp)
        hipLaunchKernelGGL((approx_kernel<true, false>), grid, block, 0, s, phi_dev, data_dev, rows, F, Cn, Tc, 0, nullptr, sn, st,
                           ap->dd, ap->bias, ap->div, f->p.missing, ap->stride);
    else if (ap->slab)
        hipLaunchKernelGGL((approx_kernel<false, true>), grid, block, ap->lds_bytes, s, phi_dev, data_dev, rows, F, Cn, Tc, f->depth,
                           ap->recs, nullptr, nullptr, nullptr, ap->bias, ap->div, f->p.missing, ap->stride);
    else
        hipLaunchKernelGGL((approx_kernel<false, false>), grid, block, 0, s, phi_dev, data_dev, rows, F, Cn, Tc, f->depth, ap->recs,
                           nullptr, nullptr, nullptr, ap->bias, ap->div, f->p.missing, ap->stride);
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}
