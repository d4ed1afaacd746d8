// Saabas contributions on a vector-leaf handle (tahoe_vector_forest_create_ex with TAHOE_CREATE_VECTOR_APPROX; DESIGN.md section
// 29).  A Saabas walk never branches on a leaf value, so the K outputs of a forest share every walk: one walk per (row, tree)
// feeds a block of KB outputs, where approx_kernel on the T x K-tree expansion walks the same splits K times.
//
// Tables, built once at create from float64 node means (saabas_means: the expression of approx_build_sparse):
//   dd[num_nodes][kp]  row i = the deltas d_k = (float)(E_k(i) - E_k(parent of i)) of node i as a child, k = 0..K-1 adjacent,
//                      kp = K rounded up to a multiple of KB and the padding 0: the walk fetches the taken child's block of KB
//                      deltas with one aligned load.  Keyed by the node's index in the handle's own VNode array (roots' rows: 0).
//   bias[K]            the bias column of tahoe_forest_predict_contribs on this handle (contribs_bias_vector)
// Kernel: lane = row; a lane walks its row's trees in order, root to leaf, so each (row, k, feature) sum is one float32 chain
// with no exchange between lanes and no atomics.  The accumulators of a lane are the KB (num_cols + 1) floats of its row's class
// block, laid out [k][num_cols + 1] as in phi_dev: a lane-private row of an LDS slab (SLAB), or the row's own floats of phi_dev
// (wide rows).  A row's class block is contiguous in phi_dev, so the wave writes it in one coalesced pass per row, AVG division
// and bias slots in that pass.
//
// Bits: per (row, k, feature) the adds are those of approx_kernel on class k of the expansion, in its order; neither KB, the
// form, the batch nor the waves of a workgroup take part in any of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "forest_internal.h"
#include "vector_internal.h"

namespace tahoe {

constexpr size_t kVecApproxSlabBudget = 64 * 1024;  // LDS per workgroup of the slab form when several waves' slabs fit
// The widest wave slab (64 lanes x KB (num_cols + 1) floats) the class-block rule takes: see vector_approx_shape
constexpr size_t kVecApproxWaveSlabMax = 40 * 1024;

template <int KB>
__device__ __forceinline__ void load_deltas(const float *__restrict__ d, float (&v)[KB])
{
    if constexpr (KB == 1) {
        v[0] = d[0];
    } else if constexpr (KB == 2) {
        const float2 a = *reinterpret_cast<const float2 *>(d);
        v[0] = a.x;
        v[1] = a.y;
    } else {
#pragma unroll
        for (int q = 0; q < KB / 4; ++q) {
            const float4 a = reinterpret_cast<const float4 *>(d)[q];
            v[4 * q + 0] = a.x;
            v[4 * q + 1] = a.y;
            v[4 * q + 2] = a.z;
            v[4 * q + 3] = a.w;
        }
    }
}

// One wave's 64 rows of the workgroup, for the class blocks k0 = blockIdx.y KB, + gridDim.y KB, ...: zero the accumulators, walk
// every tree, write the rows' class blocks out.  Every wave of the workgroup runs the same loop, so the barriers are uniform.
template <int KB, bool SLAB>
__global__ __launch_bounds__(256) void vector_approx_kernel(float *__restrict__ phi, const float *__restrict__ data, size_t rows, int F,
                                                            int K, int kp, int num_trees, const VNode *__restrict__ nodes,
                                                            const int32_t *__restrict__ roots, const float *__restrict__ dd,
                                                            const float *__restrict__ bias, float div, float missing, int stride)
{
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const size_t row0 = ((size_t)blockIdx.x * (blockDim.x >> 6) + wave) * 64;  // this wave's first row
    const size_t row = row0 + lane;
    const bool row_ok = row < rows;
    const int nr = row0 < rows ? (int)min((size_t)64, rows - row0) : 0;
    const size_t F1 = (size_t)F + 1, out_row = (size_t)K * F1;
    const float *x = data + (row_ok ? row : 0) * (size_t)F;
    float *wslab = SLAB ? slab + (size_t)wave * 64 * stride : nullptr;
    // where lane's first float of a row's class block lies: class lane / F1, column lane % F1 (the write-out steps from there)
    const size_t lane_k = (size_t)lane / F1, lane_col = (size_t)lane - lane_k * F1;

    for (int k0 = (int)blockIdx.y * KB; k0 < K; k0 += (int)gridDim.y * KB) {
        const int nk = min(KB, K - k0);     // outputs of this block
        const size_t n = (size_t)nk * F1;   // floats of a row's class block
        float *block0 = phi + row0 * out_row + (size_t)k0 * F1;  // the class block of the wave's first row
        // ---- zero the accumulators ----
        if (SLAB) {
            for (size_t i = 0; i < n; ++i) wslab[lane * stride + i] = 0.0f;  // odd stride: the 64 lanes hit 64 banks
        } else {
            for (int r = 0; r < nr; ++r)
                for (size_t i = lane; i < n; i += 64) block0[r * out_row + i] = 0.0f;
            __syncthreads();
        }
        float *acc = SLAB ? wslab + lane * stride : block0 + (row_ok ? lane : 0) * out_row;
        // ---- the walks: tree order, root to leaf; a level is one node gather, one feature read and KB adds ----
        if (row_ok) {
            for (int t = 0; t < num_trees; ++t) {
                const size_t root = (size_t)roots[t];
                const VNode *tn = nodes + root;
                const float *td = dd + root * (size_t)kp + (size_t)k0;
                // the taken child's node and its deltas are fetched together, before the adds: two round trips a level (node,
                // feature), the deltas' riding on the next node's
                VNode nd = tn[0];
                while (!(nd.bits & kVIsLeaf)) {
                    const uint32_t fid = nd.bits & kVFidMask;
                    const uint32_t i = nd.left_idx + go_right(x[fid], nd.val, (nd.bits & kVDefLeft) != 0u, missing);
                    nd = tn[i];
                    float d[KB];
                    load_deltas<KB>(td + (size_t)i * (size_t)kp, d);
                    float *cell = acc + fid;
#pragma unroll
                    for (int j = 0; j < KB; ++j)
                        if (j < nk) cell[(size_t)j * F1] += d[j];
                }
            }
        }
        __syncthreads();
        // ---- one coalesced pass per row over its class block: the AVG division, and the bias in slot F of every class ----
        for (int r = 0; r < nr; ++r) {
            float *o = block0 + r * out_row;
            const float *s = SLAB ? wslab + r * stride : o;
            size_t k = lane_k, col = lane_col;
            for (size_t i = lane; i < n; i += 64) {
                o[i] = col == (size_t)F ? bias[k0 + k] : s[i] / div;
                for (col += 64; col >= F1; col -= F1) ++k;
            }
        }
        if (SLAB) __syncthreads();  // the slab is zeroed again for the next class block
    }
}

// kernel(kb, slab) for the runtime class block and form
template <class Fn>
static inline void with_instance(int kb, bool slab, Fn &&fn)
{
    auto form = [&](auto c) {
        if (slab) fn(c, std::true_type{});
        else fn(c, std::false_type{});
    };
    if (kb == 8) form(std::integral_constant<int, 8>{});
    else if (kb == 4) form(std::integral_constant<int, 4>{});
    else if (kb == 2) form(std::integral_constant<int, 2>{});
    else form(std::integral_constant<int, 1>{});
}

static size_t wave_slab_bytes(int F, int kb) { return (size_t)64 * (((size_t)kb * ((size_t)F + 1)) | 1) * sizeof(float); }

// Class block and form of a handle, from num_cols, K and the device's LDS (DESIGN.md section 29 has the measurements):
//   in place  where two wave slabs of one output do not fit the LDS (approx.hip's rule), with class block 4 (2 or 1 where K rounded
//             up to one of them is smaller): the accumulators cost no LDS there, and of the blocks 4 measured fastest at 64 and
//             at 200 columns;
//   the slab  elsewhere, with the largest class block -- of 8, 4, 2, not above K rounded up to one of them -- whose wave slab
//             stays within kVecApproxWaveSlabMax (four waves a CU), else 1: a walk shared by more outputs does not make up for
//             the waves its slab crowds out.
// TAHOE_VECTOR_SHAP_KB forces the class block (the form then follows the two-wave-slabs rule for that block), TAHOE_APPROX_FORM
// the form (1: the slab wherever one wave's slab fits the LDS, 2: in place).  Neither changes a bit of the result.
static void vector_approx_shape(const tahoe_forest *f, VectorApprox *va)
{
    const int F = f->p.num_cols, K = f->num_classes;
    const size_t lds = (size_t)f->lds_limit;
    int cap = 1;
    while (cap < 8 && cap < K) cap *= 2;
    const int forced = f->knobs.vector_shap_kb;
    int kb;
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) {
        kb = forced;
    } else if (2 * wave_slab_bytes(F, 1) > lds) {
        kb = std::min(cap, 4);
    } else {
        for (kb = cap; kb > 1 && wave_slab_bytes(F, kb) > kVecApproxWaveSlabMax;) kb /= 2;
    }
    const size_t wave_bytes = wave_slab_bytes(F, kb);
    va->slab = 2 * wave_bytes <= lds;
    if (f->knobs.approx_form == 1) va->slab = wave_bytes <= lds;  // TAHOE_APPROX_FORM
    if (f->knobs.approx_form == 2) va->slab = false;
    va->class_block = kb;
    va->kp = (K + kb - 1) / kb * kb;
    va->stride = va->slab ? (int)(wave_bytes / (64 * sizeof(float))) : 0;
    va->waves = va->slab ? (int)std::max<size_t>(1, std::min<size_t>(4, kVecApproxSlabBudget / wave_bytes)) : 4;
    va->lds_bytes = va->slab ? va->waves * wave_bytes : 0;
    va->grid_blocks = f->knobs.vector_shap_grid != 0;  // TAHOE_VECTOR_SHAP_GRID; the rule: over gridDim.y
}

tahoe_status vector_approx_build(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *leaf_values,
                                 const float *covers)
{
    VectorApprox *va = new (std::nothrow) VectorApprox();
    if (!va) return fail(TAHOE_ERR_NO_MEMORY, "vector_approx_build");
    f->vl->approx = va;
    vector_approx_shape(f, va);
    const size_t T = (size_t)f->p.num_trees, N = (size_t)f->p.num_nodes, K = (size_t)f->num_classes, kp = (size_t)va->kp;
    if (N > SIZE_MAX / sizeof(float) / kp)
        return fail(TAHOE_ERR_INVALID_ARG, "TAHOE_CREATE_VECTOR_APPROX: num_nodes x leaf_dim floats overflow size_t");
    std::vector<float> dd(N * kp, 0.0f);
    parallel_for(T, 16, [&](size_t lo, size_t hi) {
        std::vector<double> E;
        for (size_t t = lo; t < hi; ++t) {
            const size_t a = (size_t)trees[t], b = t + 1 < T ? (size_t)trees[t + 1] : N;
            const tahoe_sparse_node *tn = nodes + a;
            for (size_t k = 0; k < K; ++k) {
                saabas_means(tn, covers + a, b - a, E, [&](size_t i) { return leaf_values[(size_t)tn[i].left_idx * K + k]; });
                for (size_t i = 0; i < b - a; ++i) {
                    if (tn[i].bits < 0) continue;
                    const size_t l = (size_t)tn[i].left_idx;
                    dd[(a + l) * kp + k] = saabas_delta(E, l, i);
                    dd[(a + l + 1) * kp + k] = saabas_delta(E, l + 1, i);
                }
            }
        }
    });
    std::vector<float> h_bias, h_div;
    contribs_bias_vector(f, trees, nodes, leaf_values, covers, h_bias, h_div);
    va->div = h_div.empty() ? 1.0f : h_div[0];  // every tree feeds every output: one divisor
    tahoe_status s = TAHOE_OK;
    if ((s = hip_status(upload(&va->dd, dd, &f->device_bytes), "upload(vector deltas)")) ||
        (s = hip_status(upload(&va->bias, h_bias, &f->device_bytes), "upload(bias)")))
        return s;
    hipError_t e = hipSuccess;
    if (va->slab)
        with_instance(va->class_block, true, [&](auto c, auto sl) {
            e = allow_max_lds(reinterpret_cast<const void *>(&vector_approx_kernel<decltype(c)::value, decltype(sl)::value>), f->lds_limit);
        });
    return hip_status(e, "hipFuncSetAttribute(vector_approx)");
}

void vector_approx_destroy(tahoe_forest *f)
{
    VectorApprox *va = f->vl ? f->vl->approx : nullptr;
    if (!va) return;
    if (va->dd) (void)hipFree(va->dd);
    if (va->bias) (void)hipFree(va->bias);
    delete va;
    f->vl->approx = nullptr;
}

bool vector_serves_approx(const tahoe_forest *f) { return f->vl && f->vl->approx; }

tahoe_status vector_predict_approx(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                   const char *fn)
{
    if (rows == 0) return TAHOE_OK;
    if (!phi_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "%s: null argument", fn);
    if (tahoe_status st = check_shap_out(f, rows, 1, fn)) return st;
    const VectorApprox *va = f->vl->approx;
    DeviceGuard on_device(f->device);
    const int K = f->num_classes, kb = va->class_block;
    const size_t per_block = (size_t)va->waves * 64;
    const dim3 grid((unsigned)((rows + per_block - 1) / per_block), va->grid_blocks ? (unsigned)((K + kb - 1) / kb) : 1u);
    with_instance(kb, va->slab, [&](auto c, auto sl) {
        hipLaunchKernelGGL((vector_approx_kernel<decltype(c)::value, decltype(sl)::value>), grid, dim3((unsigned)per_block),
                           va->lds_bytes, stream, phi_dev, data_dev, rows, f->p.num_cols, K, va->kp, f->p.num_trees, f->vl->nodes,
                           f->vl->roots, va->dd, va->bias, va->div, f->p.missing, va->stride);
    });
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

}  // namespace tahoe
