// Interventional TreeSHAP on a vector-leaf handle (tahoe_vector_forest_create_ex with TAHOE_CREATE_INTERVENTIONAL; DESIGN.md
// section 27).  The work of interventional_kernel per (row, bin) is a loop over the B background rows -- ballots, popcounts and
// one table read -- that never touches a leaf value: the leaf enters once, after the loop.  The K outputs of a leaf share its
// path, so the handle holds one set of bins and one set of background masks, and the kernel runs the background loop once per
// (row, bin) for a block of KB classes, where interventional_kernel on the K-fold expansion runs it once per class.
//
// Bits: phi[row][k][.] is what interventional_kernel gives for class k of the expansion.  The bins are that class's bins, bin b
// goes to wave b % 4, a lane's weights add in background order, its term is (o ? acc : -acc) * leaf in that association, terms of
// one feature add in round order, the four wave slabs add as ((s0 + s1) + s2) + s3, divided by (float)B, then by (float)num_trees
// with AVG (else by 1.0f).  Neither KB nor the rows of a tile take part in any of it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "forest_internal.h"
#include "contribs_internal.h"
#include "treeshap_lanes.h"
#include "vector_internal.h"

namespace tahoe {

// One workgroup = a tile of R rows (staged in LDS) x all bins x the class blocks k0 = blockIdx.y KB, + gridDim.y KB, ...; wave w
// evaluates bins w, w + 4, ... into its own KB slabs [R][F] of LDS, one per class of the block; per class the four wave slabs are
// summed in wave order and written out.  LDS: tile [R][F] | slabs [4][KB][R][F] | W [32 x 32] (WLDS; else the weight table is
// read from global memory).  The body of a (bin, row) is interventional_kernel's: background_weight_sum
// (treeshap_lanes.h).
template <int KB, bool WLDS>
__global__ __launch_bounds__(256) void vector_interventional_kernel(float *__restrict__ phi, const float *__restrict__ data,
                                                                    size_t rows, int F, int K, int R,
                                                                    const uint4 *__restrict__ elems,
                                                                    const uint32_t *__restrict__ bin_info, int bins,
                                                                    const float *__restrict__ leaves,
                                                                    const unsigned long long *__restrict__ masks, int B,
                                                                    const float *__restrict__ consts, float div, float missing)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row0 = (size_t)blockIdx.x * R;
    const int nr = (int)min((size_t)R, rows - row0);
    const int tile_n = nr * F;
    const size_t slab_n = (size_t)R * F;
    float *tile = smem;
    float *slab = smem + slab_n * (1 + (size_t)wave * KB);  // this wave's KB slabs, class j of the block at slab + j slab_n
    float *wl = smem + slab_n * (1 + 4 * KB);
    if (WLDS)
        for (int i = tid; i < kIvTable; i += 256) wl[i] = consts[i];
    const float *w = WLDS ? wl : consts;
    const float *src = data + row0 * F;
    for (int i = tid; i < tile_n; i += 256) tile[i] = src[i];
    const size_t out_row = (size_t)K * (F + 1);
    const float fB = (float)B;

    for (int k0 = (int)blockIdx.y * KB; k0 < K; k0 += (int)gridDim.y * KB) {
        const int nk = min(KB, K - k0);  // classes of this block
#pragma unroll
        for (int j = 0; j < KB; ++j)
            if (j < nk)
                for (int i = lane; i < tile_n; i += 64) slab[j * slab_n + i] = 0.0f;
        __syncthreads();
        for (int b = wave; b < bins; b += kContribWaves) {
            const uint4 e = elems[(size_t)b * 64 + lane];
            const int rounds = (int)(bin_info[b] >> 8);
            const float lower = __uint_as_float(e.x), upper = __uint_as_float(e.y);
            const int fid = elem_fid(e.w), rank = elem_rank(e.w), ud = elem_ud(e.w), round = elem_round(e.w);
            const bool missing_ok = elem_missing_ok(e.w), nan_ok = elem_nan_ok(e.w);
            const int gs = lane - rank;  // lane of the path's root element
            float leaf[KB];  // the block's leaf values
            load_leaf_block<KB>(leaf, leaves, e.x, K, k0, nk, rank, gs);
            // the lanes of this lane's path but its root: gs + 1 .. gs + ud (a path never leaves its bin)
            const unsigned long long pm = ud == 0 ? 0ull : ((1ull << ud) - 1ull) << (gs + 1);
            const unsigned long long *mb = masks + (size_t)b * B;
            for (int r = 0; r < nr; ++r) {
                const bool o = rank != 0 && follows(tile[r * F + fid], lower, upper, missing_ok, nan_ok, missing);
                const float acc = background_weight_sum(o, pm, mb, B, w, lane);
                const float s = o ? acc : -acc;  // shared by the block's classes
                // two lanes of a bin on one feature add in lane order (round = earlier lanes of the bin on that feature)
                float *cell = slab + r * F + fid;
                for (int q = 0; q < rounds; ++q)
                    if (rank != 0 && round == q) add_leaf_block<KB>(cell, slab_n, nk, [&](int j) { return s * leaf[j]; });
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            if (j >= nk) continue;
            const float *s0 = smem + slab_n * (1 + j), *s1 = s0 + KB * slab_n, *s2 = s1 + KB * slab_n, *s3 = s2 + KB * slab_n;
            float *out = phi + row0 * out_row + (size_t)(k0 + j) * (F + 1);
            for (int i = tid; i < tile_n; i += 256) {
                const int r = i / F, col = i - r * F;
                const float v = ((s0[i] + s1[i]) + s2[i]) + s3[i];
                out[r * out_row + col] = v / fB / div;
            }
            for (int r = tid; r < nr; r += 256) out[r * out_row + F] = consts[kIvTable + k0 + j];
        }
        __syncthreads();
    }
}

// kernel(kb, wlds) for the runtime class block; the table leaves LDS only where one row with a class block of 1 fills it
template <class Fn>
static inline void with_iv_form(int kb, bool wlds, Fn &&fn)
{
    with_class_block(kb, [&](auto c) {
        if constexpr (decltype(c)::value > 1) fn(c, std::true_type{});
        else if (wlds) fn(c, std::true_type{});
        else fn(c, std::false_type{});
    });
}

// Rows of a tile for class block kb: the largest power of two <= kIvMaxTileRows whose tile, 4 kb slabs and the weight table fit
// the budget, 0 where not even one row does
static size_t iv_tile_rows(int F, int kb)
{
    const size_t per_row = (1 + 4 * (size_t)kb) * (size_t)F * sizeof(float), table = kIvTable * sizeof(float);
    size_t R = kIvMaxTileRows;
    while (R > 1 && R * per_row + table > kIvLdsBudget) R /= 2;
    return R * per_row + table <= kIvLdsBudget ? R : 0;
}

// The class block first, the tile second: the block divides the number of background loops, a tile row only amortises a bin's
// 1.3 KB of elements.  KB = the largest of 8, 4, 2 -- not above K rounded up to one of them -- that leaves a row within the
// budget; else 1 with iv_shape's fallback of interventional.hip: one row in the whole LDS, the table in LDS if it still fits.
// TAHOE_VECTOR_SHAP_KB forces a block that leaves a row, TAHOE_VECTOR_SHAP_GRID the placement of the blocks
// (VectorShap::grid_blocks serves both kernels).  None of them changes a bit of the result.
void vector_iv_shape(const tahoe_forest *f, VectorShap *sh)
{
    const int F = f->p.num_cols, K = f->num_classes;
    const int kb = pick_class_block(f->knobs.vector_shap_kb, K, [&](int c, bool) { return iv_tile_rows(F, c) != 0; });
    const size_t per_row = (1 + 4 * (size_t)kb) * (size_t)F * sizeof(float), table = kIvTable * sizeof(float);
    const size_t R = std::max<size_t>(iv_tile_rows(F, kb), 1);  // (kb == 1: check_contrib_cols has made sure that one row fits the device)
    sh->iv_class_block = kb;
    sh->iv_rows = (int)R;
    sh->iv_wlds = R * per_row + table <= (size_t)f->lds_limit;
    sh->iv_lds_bytes = R * per_row + (sh->iv_wlds ? table : 0);
}

bool vector_serves_interventional(const tahoe_forest *f) { return f->vl && f->vl->shap && f->vl->shap->interventional; }

hipError_t vector_iv_allow_lds(const tahoe_forest *f)
{
    const VectorShap *sh = f->vl->shap;
    hipError_t e = hipSuccess;
    with_iv_form(sh->iv_class_block, sh->iv_wlds, [&](auto kb, auto wlds) {
        e = allow_max_lds(reinterpret_cast<const void *>(&vector_interventional_kernel<decltype(kb)::value, decltype(wlds)::value>),
                          f->lds_limit);
    });
    return e;
}

tahoe_status vector_predict_interventional(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                           const char *fn)
{
    const VectorShap *sh = f->vl->shap;
    const tahoe_istate *iv = f->iv;
    const int K = f->num_classes, kb = sh->iv_class_block;
    const size_t R = (size_t)sh->iv_rows, tiles = (rows + R - 1) / R;
    if (tiles > 0x7fffffffu) return fail(TAHOE_ERR_INVALID_ARG, "%s: too many rows for one launch: %zu", fn, rows);
    DeviceGuard on_device(f->device);
    const dim3 grid((unsigned)tiles, sh->grid_blocks ? (unsigned)((K + kb - 1) / kb) : 1u);
    with_iv_form(kb, sh->iv_wlds, [&](auto c, auto wlds) {
        hipLaunchKernelGGL((vector_interventional_kernel<decltype(c)::value, decltype(wlds)::value>), grid, dim3(256), sh->iv_lds_bytes,
                           stream, phi_dev, data_dev, rows, f->p.num_cols, K, (int)R, sh->elems, sh->bin_info, sh->bins, f->vl->leaves,
                           iv->masks, (int)iv->bg_rows, iv->consts, sh->div, f->p.missing);
    });
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

}  // namespace tahoe
