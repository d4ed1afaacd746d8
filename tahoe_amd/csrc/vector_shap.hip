// Path-dependent TreeSHAP on a vector-leaf handle (tahoe_vector_forest_create_ex with TAHOE_CREATE_CONTRIBS; DESIGN.md section
// 26).  The K outputs of a leaf share its path: features, bounds, zero fractions, lengths and round numbers are those of every
// class of the K-fold expansion, and only the leaf value, which enters a path term last, differs.  So the tables hold one set of
// bins (contribs.hip builds them: contribs_tables_vector) and the kernel runs the extend recursion and the unwound-path sum once
// per (row, bin) for a block of KB classes, where contribs_kernel on the expansion runs them once per class.
//
// Bits: phi[row][k][.] is what contribs_kernel gives for class k of the expansion.  The bins are that class's bins, bin b goes to
// wave b % 4, a lane's term is (total * (o ? 1 - z : -z)) * leaf in that association, terms of one feature add in round order,
// the four wave slabs add as ((s0 + s1) + s2) + s3 and are divided by (float)num_trees with AVG.  Neither KB nor the rows of a
// tile take part in any of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "forest_internal.h"
#include "contribs_internal.h"
#include "treeshap_lanes.h"
#include "vector_internal.h"

namespace tahoe {

constexpr size_t kVecShapLdsBudget = 80 * 1024;  // two workgroups per CU, as contribs_kernel's tiles
constexpr int kVecShapMinRows = 4;               // a class block wider than 1 must leave a tile of at least this many rows

// One workgroup = a tile of R rows (staged in LDS) x all bins x the class blocks k0 = blockIdx.y KB, + gridDim.y KB, ...; wave w
// evaluates bins w, w + 4, ... into its own KB slabs [R][F] of LDS, one per class of the block; per class the four wave slabs are
// summed in wave order and written out.  LDS: tile [R][F] | slabs [4][KB][R][F].  The recursion of a (bin, row) is contribs_tile's
// statements (contribs.hip), kept in step by hand: treeshap_lanes.h says why they are not one function.
// SPARE = false: phi[rows][K][F + 1] (vector_contribs_kernel).  SPARE = true: the same values into row F of each (row, k) matrix of
// out[rows][K][F + 1][F + 1] (tahoe_forest_predict_interactions on a handle with TAHOE_CREATE_VECTOR_INTERACTIONS,
// vector_contribs_spare_kernel).
template <int KB, bool SPARE>
__device__ __forceinline__ void vector_contribs_tile(float *__restrict__ phi, const float *__restrict__ data, size_t rows, int F, int K,
                                                     int R, const uint4 *__restrict__ elems, const float *__restrict__ one_minus_z,
                                                     const uint32_t *__restrict__ bin_info, int bins,
                                                     const float *__restrict__ leaves, const float *__restrict__ bias, float div,
                                                     float missing)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (SPARE) phi += (size_t)F * (F + 1);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row0 = (size_t)blockIdx.x * R;
    const int nr = (int)min((size_t)R, rows - row0);
    const int tile_n = nr * F;
    const size_t slab_n = (size_t)R * F;
    float *tile = smem;
    float *slab = smem + slab_n * (1 + (size_t)wave * KB);  // this wave's KB slabs, class j of the block at slab + j slab_n
    const float *src = data + row0 * F;
    for (int i = tid; i < tile_n; i += 256) tile[i] = src[i];
    const size_t mat = (size_t)(F + 1) * (F + 1);
    const size_t out_row = SPARE ? (size_t)K * mat : (size_t)K * (F + 1);

    for (int k0 = (int)blockIdx.y * KB; k0 < K; k0 += (int)gridDim.y * KB) {
        const int nk = min(KB, K - k0);  // classes of this block
#pragma unroll
        for (int j = 0; j < KB; ++j)
            if (j < nk)
                for (int i = lane; i < tile_n; i += 64) slab[j * slab_n + i] = 0.0f;
        __syncthreads();
        for (int b = wave; b < bins; b += kContribWaves) {
            const uint4 e = elems[(size_t)b * 64 + lane];
            const float om = one_minus_z[(size_t)b * 64 + lane];
            const uint32_t info = bin_info[b];
            const int steps = (int)(info & 0xffu), rounds = (int)(info >> 8);
            const float lower = __uint_as_float(e.x), upper = __uint_as_float(e.y), z = __uint_as_float(e.z);
            const int fid = elem_fid(e.w), rank = elem_rank(e.w), ud = elem_ud(e.w), round = elem_round(e.w);
            const bool missing_ok = elem_missing_ok(e.w), nan_ok = elem_nan_ok(e.w);
            const int gs = lane - rank;  // lane of the path's root element
            // the block's leaf values: a root lane reads them (.x is its vector's index; a padding lane names vector 0, which
            // exists where a bin does), the other lanes of the path take them from it
            float leaf[KB];
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                float own = 0.0f;
                if (rank == 0 && j < nk) own = leaves[(size_t)e.x * (size_t)K + (size_t)(k0 + j)];
                leaf[j] = lane_read(own, gs);
            }
            const float zdiv = z / (float)(ud + 1);
            const float udp1 = (float)(ud + 1);
            const int split = unwind_split(z, ud);
            for (int r = 0; r < nr; ++r) {
                const bool o = follows(tile[r * F + fid], lower, upper, missing_ok, nan_ok, missing);
                const uint32_t zo = e.z | (o ? 0x80000000u : 0u);
                // extend: after step d, lanes of rank <= d hold the permutation weights of the first d + 1 elements
                float pw = rank == 0 ? 1.0f : 0.0f;
                for (int d = 1; d < steps; ++d) {
                    const uint32_t s = lane_read_u(zo, min(gs + d, 63));
                    const float zd = __uint_as_float(s & 0x7fffffffu), od = (s >> 31) ? 1.0f : 0.0f;
                    const float left = from_left_lane(pw);
                    const float inv = c_inv[d + 1];
                    const float a = (float)max(d - rank, 0) * inv, bb = (float)rank * inv;
                    const float np = pw * zd * a + od * left * bb;
                    pw = d <= ud ? np : pw;
                }
                // unwound-path sum of this lane's element
                float next = lane_read(pw, gs + ud);
                float total = 0.0f;
                for (int i = steps - 2; i >= 0; --i) {
                    const float pwi = lane_read(pw, min(gs + i, 63));
                    const float pre = (float)(ud - i) * zdiv;
                    const float tmp = next * udp1 * c_inv[i + 1];
                    const float t_one = total + tmp, n_one = pwi - tmp * pre;
                    const float t_zero = pre > 0.0f ? total + pwi * __builtin_amdgcn_rcpf(pre) : total;
                    if (i < ud && (!o || i >= split)) {
                        total = o ? t_one : t_zero;
                        next = o ? n_one : next;
                    }
                }
                // a followed element's weights below `split` come from the other end (unwind_split, treeshap_lanes.h)
                if (__any(o && split > 0)) {
                    float prev = 0.0f;
                    for (int i = 0; i < steps - 1; ++i) {
                        const float pwi = lane_read(pw, min(gs + i, 63));
                        const float q = (pwi - prev * (float)i * c_inv[ud + 1]) * __builtin_amdgcn_rcpf((float)(ud - i) * zdiv);
                        if (o && i < split) {
                            total += q;
                            prev = q;
                        }
                    }
                }
                const float tw = total * (o ? om : -z);  // (one - zero), shared by the block's classes
                // two lanes of a bin on one feature add in lane order (round = earlier lanes of the bin on that feature)
                float *cell = slab + r * F + fid;
                for (int k = 0; k < rounds; ++k)
                    if (rank != 0 && round == k) {
                        float v[KB];
#pragma unroll
                        for (int j = 0; j < KB; ++j)
                            if (j < nk) v[j] = cell[j * slab_n];
#pragma unroll
                        for (int j = 0; j < KB; ++j)
                            if (j < nk) cell[j * slab_n] = v[j] + tw * leaf[j];
                    }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            if (j >= nk) continue;
            const float *s0 = smem + slab_n * (1 + j), *s1 = s0 + KB * slab_n, *s2 = s1 + KB * slab_n, *s3 = s2 + KB * slab_n;
            float *out = phi + row0 * out_row + (size_t)(k0 + j) * (SPARE ? mat : (F + 1));
            for (int i = tid; i < tile_n; i += 256) {
                const int r = i / F, col = i - r * F;
                const float v = ((s0[i] + s1[i]) + s2[i]) + s3[i];
                out[r * out_row + col] = v / div;
            }
            for (int r = tid; r < nr; r += 256) out[r * out_row + F] = bias[k0 + j];
        }
        __syncthreads();
    }
}

#define TAHOE_VECTOR_SHAP_PARAMS                                                                                                  \
    float *__restrict__ phi, const float *__restrict__ data, size_t rows, int F, int K, int R, const uint4 *__restrict__ elems,  \
        const float *__restrict__ one_minus_z, const uint32_t *__restrict__ bin_info, int bins,                                   \
        const float *__restrict__ leaves, const float *__restrict__ bias, float div, float missing
template <int KB>
__global__ __launch_bounds__(256) void vector_contribs_kernel(TAHOE_VECTOR_SHAP_PARAMS)
{
    vector_contribs_tile<KB, false>(phi, data, rows, F, K, R, elems, one_minus_z, bin_info, bins, leaves, bias, div, missing);
}
template <int KB>
__global__ __launch_bounds__(256) void vector_contribs_spare_kernel(TAHOE_VECTOR_SHAP_PARAMS)
{
    vector_contribs_tile<KB, true>(phi, data, rows, F, K, R, elems, one_minus_z, bin_info, bins, leaves, bias, div, missing);
}
#undef TAHOE_VECTOR_SHAP_PARAMS

// Rows of a tile for class block kb: the largest power of two <= 64 whose tile and 4 kb slabs fit the budget; for kb == 1 at
// least 1 (the column limit of contribs_tables_vector has made sure that one row fits the device), else 0 where fewer than
// min_rows fit
static size_t tile_rows(int F, int kb, size_t min_rows)
{
    const size_t per_row = (1 + 4 * (size_t)kb) * (size_t)F * sizeof(float);
    size_t R = 64;
    while (R > 1 && R * per_row > kVecShapLdsBudget) R /= 2;
    if (kb == 1) return R;
    return (R * per_row <= kVecShapLdsBudget && R >= min_rows) ? R : 0;
}

tahoe_status vector_shap_build(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *leaf_values,
                               const float *covers, unsigned flags)
{
    VectorPathTables h;
    if (const tahoe_status s = contribs_tables_vector(f, trees, nodes, leaf_values, covers, h)) return s;
    VectorShap *sh = new (std::nothrow) VectorShap();
    if (!sh) return fail(TAHOE_ERR_NO_MEMORY, "vector_shap_build");
    f->vl->shap = sh;
    sh->contribs = (flags & TAHOE_CREATE_CONTRIBS) != 0;
    sh->interventional = (flags & TAHOE_CREATE_INTERVENTIONAL) != 0;
    sh->interactions = (flags & TAHOE_CREATE_VECTOR_INTERACTIONS) != 0;
    const int F = f->p.num_cols, K = f->num_classes;
    sh->bins = (int)h.bin_info.size();
    sh->paths = h.paths;
    sh->path_elems = h.path_elems;
    // every tree feeds every class: one divisor, class_bias's (h.div, which a handle without TAHOE_CREATE_CONTRIBS does not get)
    sh->div = ((f->p.output & TAHOE_OUT_AVG) != 0 && f->class_trees > 0) ? (float)f->class_trees : 1.0f;
    // The class block: the largest of 8, 4, 2 -- not above K rounded up to one of them -- that leaves a tile of >= 4 rows, else 1.
    // TAHOE_VECTOR_SHAP_KB forces one that leaves a tile of >= 1 row.  Neither changes a bit of the result.
    const int kb = pick_class_block(f->knobs.vector_shap_kb, K, [&](int c, bool forced) {
        return tile_rows(F, c, forced ? 1 : kVecShapMinRows) != 0;
    });
    sh->class_block = kb;
    sh->rows_per_tile = (int)tile_rows(F, kb, 1);
    sh->lds_bytes = (1 + 4 * (size_t)kb) * (size_t)sh->rows_per_tile * (size_t)F * sizeof(float);
    sh->grid_blocks = f->knobs.vector_shap_grid != 0;  // TAHOE_VECTOR_SHAP_GRID; the rule: over gridDim.y
    size_t *total = &f->device_bytes;
    tahoe_status s = TAHOE_OK;
    if ((s = hip_status(upload(&sh->elems, h.elems, total), "upload(path elements)")) ||
        (s = hip_status(upload(&sh->bin_info, h.bin_info, total), "upload(bin_info)")))
        return s;
    if (sh->interventional) vector_iv_shape(f, sh);
    if (!sh->contribs) return TAHOE_OK;  // only what the interventional game reads: no one_minus_z, no TreeSHAP bias
    if ((s = hip_status(upload(&sh->one_minus_z, h.one_minus_z, total), "upload(one_minus_z)")) ||
        (s = hip_status(upload(&sh->bias, h.bias, total), "upload(bias)")))
        return s;
    hipError_t e = hipSuccess;
    with_class_block(kb, [&](auto c) {
        e = allow_max_lds(reinterpret_cast<const void *>(&vector_contribs_kernel<decltype(c)::value>), f->lds_limit);
    });
    if (e != hipSuccess || !sh->interactions) return hip_status(e, "hipFuncSetAttribute(vector_contribs)");
    // TAHOE_CREATE_VECTOR_INTERACTIONS: no table of its own, the shape of vector_interactions_kernel and the LDS of the two kernels
    with_class_block(kb, [&](auto c) {
        e = allow_max_lds(reinterpret_cast<const void *>(&vector_contribs_spare_kernel<decltype(c)::value>), f->lds_limit);
    });
    if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(vector_contribs_spare)");
    return vector_inter_build(f, sh);
}

void vector_shap_destroy(tahoe_forest *f)
{
    VectorShap *sh = f->vl ? f->vl->shap : nullptr;
    if (!sh) return;
    if (sh->elems) (void)hipFree(sh->elems);
    if (sh->one_minus_z) (void)hipFree(sh->one_minus_z);
    if (sh->bin_info) (void)hipFree(sh->bin_info);
    if (sh->bias) (void)hipFree(sh->bias);
    delete sh;
    f->vl->shap = nullptr;
}

bool vector_serves_contribs(const tahoe_forest *f) { return f->vl && f->vl->shap && f->vl->shap->contribs; }

tahoe_status vector_predict_contribs(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                     const char *fn)
{
    if (rows == 0) return TAHOE_OK;
    if (!phi_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "%s: null argument", fn);
    if (tahoe_status st = check_shap_out(f, rows, 1, fn)) return st;
    const VectorShap *sh = f->vl->shap;
    DeviceGuard on_device(f->device);
    const int K = f->num_classes, kb = sh->class_block;
    const size_t R = (size_t)sh->rows_per_tile;
    const dim3 grid((unsigned)((rows + R - 1) / R), sh->grid_blocks ? (unsigned)((K + kb - 1) / kb) : 1u);
    with_class_block(kb, [&](auto c) {
        hipLaunchKernelGGL(vector_contribs_kernel<decltype(c)::value>, grid, dim3(256), sh->lds_bytes, stream, phi_dev, data_dev, rows,
                           f->p.num_cols, K, (int)R, sh->elems, sh->one_minus_z, sh->bin_info, sh->bins, f->vl->leaves, sh->bias,
                           sh->div, f->p.missing);
    });
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

tahoe_status vector_launch_contribs_spare(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows, hipStream_t stream)
{
    const VectorShap *sh = f->vl->shap;
    const int K = f->num_classes, kb = sh->class_block;
    const size_t R = (size_t)sh->rows_per_tile;
    const dim3 grid((unsigned)((rows + R - 1) / R), sh->grid_blocks ? (unsigned)((K + kb - 1) / kb) : 1u);
    with_class_block(kb, [&](auto c) {
        hipLaunchKernelGGL(vector_contribs_spare_kernel<decltype(c)::value>, grid, dim3(256), sh->lds_bytes, stream, out_dev, data_dev,
                           rows, f->p.num_cols, K, (int)R, sh->elems, sh->one_minus_z, sh->bin_info, sh->bins, f->vl->leaves, sh->bias,
                           sh->div, f->p.missing);
    });
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

}  // namespace tahoe
