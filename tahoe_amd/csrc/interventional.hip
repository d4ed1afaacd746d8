// Interventional TreeSHAP (Lundberg et al. 2020, "Independent Tree SHAP"; SHAP's feature_perturbation="interventional"):
// per-feature contributions of v(S) = mean over background rows r of f(x_S, r_{N \ S}).  It reads the 64-lane path bins that
// create builds for TAHOE_CREATE_CONTRIBS (contribs.hip) and uses only their bounds and missing / NaN flags, never the covers.
// On a vector-leaf handle created with TAHOE_CREATE_INTERVENTIONAL the background is built here, by the same body, and the
// contributions come from vector_iv.hip.
//
// For one pair (x, r) and one path with leaf value v: A = the path's features where only x follows every edge of the feature,
// B = those where only r does; a feature where neither does kills the path.  Then i in A gets +v (|A| - 1)! |B|! / (|A| + |B|)!,
// j in B gets -v |A|! (|B| - 1)! / (|A| + |B|)!, the path's other features nothing.  One lane per path element: the wave ballots
// its elements' one-fractions for the row (Mx) once per (row, bin); tahoe_forest_set_background has stored the ballots of every
// background row (Mr) per bin; D = Mx ^ Mr marks the elements on which x and r differ, and per lane a = |D & its path's Mx|,
// b = |D & its path's ~Mx|, dead = b < |its path's ~Mx| (an element that both fail).  The weight comes from one 32 x 32 table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "forest_internal.h"
#include "contribs_internal.h"
#include "treeshap_lanes.h"
#include "vector_internal.h"

namespace tahoe {

// One wave per bin: masks[b][r] = ballot over the bin's lanes of "background row r follows this element" (rank-0 lanes: 0).
// SETS (both kernels): the handle's path elements carry category sets, the one-fraction is follows_set() (contribs_internal.h).
template <bool SETS = false>
__global__ __launch_bounds__(256) void background_mask_kernel(unsigned long long *__restrict__ masks, const float *__restrict__ bg,
                                                              size_t B, int F, size_t bins, const uint4 *__restrict__ elems,
                                                              float missing, const uint32_t *__restrict__ elem_set,
                                                              const uint32_t *__restrict__ set_pool, uint32_t set_words)
{
    const int lane = threadIdx.x & 63;
    const size_t b = (size_t)blockIdx.x * kContribWaves + (size_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (b >= bins) return;
    const uint4 e = elems[b * 64 + lane];
    const float lower = __uint_as_float(e.x), upper = __uint_as_float(e.y);
    const int fid = elem_fid(e.w), rank = elem_rank(e.w);
    const bool missing_ok = elem_missing_ok(e.w), nan_ok = elem_nan_ok(e.w);
    unsigned long long *out = masks + b * B;
    ElemSet es{};
    bool gather = false;
    if constexpr (SETS) {
        es = elem_set_load(elem_set, set_pool, set_words, b * 64 + lane);
        gather = elem_sets_gather(es);
    }
    for (size_t r = 0; r < B; ++r) {
        bool o;
        if constexpr (SETS) o = rank != 0 && follows_set(bg[r * F + fid], lower, upper, missing_ok, nan_ok, missing, es, set_pool, set_words, gather);
        else o = rank != 0 && follows(bg[r * F + fid], lower, upper, missing_ok, nan_ok, missing);
        const unsigned long long m = __ballot(o);
        if (lane == 0) out[r] = m;
    }
}

// One workgroup = a tile of R rows (staged in LDS) x all bins; wave w evaluates bins w, w + 4, ... of each class into its own
// slab [R][F] of LDS, as contribs_tile does.  Per (row, bin) each lane sums its weights over the background rows in order in a
// register; the sum times +-leaf goes into the slab in the bin's round order; the four slabs are summed in wave order, divided
// by B, then by (float)Tc with AVG.  Every row sees the same operations in the same order whatever its batch, tile or position.
// WLDS: the weight table sits in LDS after the slabs (else, for the widest rows, it is read from global memory).
template <bool WLDS, bool SETS = false>
__global__ __launch_bounds__(256) void interventional_kernel(float *__restrict__ phi, const float *__restrict__ data, size_t rows,
                                                             int F, int C, int R, const uint4 *__restrict__ elems,
                                                             const uint32_t *__restrict__ bin_info,
                                                             const int *__restrict__ class_bins,
                                                             const float *__restrict__ class_div,
                                                             const unsigned long long *__restrict__ masks, int B,
                                                             const float *__restrict__ consts, float missing,
                                                             const uint32_t *__restrict__ elem_set,
                                                             const uint32_t *__restrict__ set_pool, uint32_t set_words)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row0 = (size_t)blockIdx.x * R;
    const int nr = (int)min((size_t)R, rows - row0);
    const int tile_n = nr * F;
    const size_t slab_n = (size_t)R * F;
    float *tile = smem;
    float *slab = smem + slab_n * (1 + wave);
    const float *s0 = smem + slab_n, *s1 = s0 + slab_n, *s2 = s1 + slab_n, *s3 = s2 + slab_n;
    float *wl = smem + 5 * slab_n;
    if (WLDS)
        for (int i = tid; i < kIvTable; i += 256) wl[i] = consts[i];
    const float *w = WLDS ? wl : consts;
    const float *src = data + row0 * F;
    for (int i = tid; i < tile_n; i += 256) tile[i] = src[i];
    const size_t out_row = (size_t)C * (F + 1);
    const float fB = (float)B;

    for (int c = 0; c < C; ++c) {
        for (int i = lane; i < tile_n; i += 64) slab[i] = 0.0f;
        __syncthreads();
        const int b_end = class_bins[c + 1];
        for (int b = class_bins[c] + wave; b < b_end; b += kContribWaves) {
            const uint4 e = elems[(size_t)b * 64 + lane];
            const int rounds = (int)(bin_info[b] >> 8);
            const float lower = __uint_as_float(e.x), upper = __uint_as_float(e.y);
            const int fid = elem_fid(e.w), rank = elem_rank(e.w), ud = elem_ud(e.w), round = elem_round(e.w);
            const bool missing_ok = elem_missing_ok(e.w), nan_ok = elem_nan_ok(e.w);
            const int gs = lane - rank;  // lane of the path's root element
            const float leaf = lane_read(lower, gs);
            // the lanes of this lane's path but its root: gs + 1 .. gs + ud (a path never leaves its bin)
            const unsigned long long pm = ud == 0 ? 0ull : ((1ull << ud) - 1ull) << (gs + 1);
            const unsigned long long *mb = masks + (size_t)b * B;
            ElemSet es{};
            bool gather = false;
            if constexpr (SETS) {
                es = elem_set_load(elem_set, set_pool, set_words, (size_t)b * 64 + lane);
                gather = elem_sets_gather(es);
            }
            for (int r = 0; r < nr; ++r) {
                bool o;
                if constexpr (SETS) o = rank != 0 && follows_set(tile[r * F + fid], lower, upper, missing_ok, nan_ok, missing, es, set_pool, set_words, gather);
                else o = rank != 0 && follows(tile[r * F + fid], lower, upper, missing_ok, nan_ok, missing);
                const float acc = background_weight_sum(o, pm, mb, B, w, lane);
                const float term = (o ? acc : -acc) * leaf;
                // two lanes of a bin on one feature add in lane order, as in contribs_tile
                for (int k = 0; k < rounds; ++k)
                    if (rank != 0 && round == k) slab[r * F + fid] += term;
            }
        }
        __syncthreads();
        const float div = class_div[c];
        for (int i = tid; i < tile_n; i += 256) {
            const int r = i / F, col = i - r * F;
            const float v = ((s0[i] + s1[i]) + s2[i]) + s3[i];
            phi[(row0 + r) * out_row + (size_t)c * (F + 1) + col] = v / fB / div;
        }
        for (int r = tid; r < nr; r += 256) phi[(row0 + r) * out_row + (size_t)c * (F + 1) + F] = consts[kIvTable + c];
        __syncthreads();
    }
}

#define TAHOE_IV_KERNEL_ARGS                                                                                                  \
    float *, const float *, size_t, int, int, int, const uint4 *, const uint32_t *, const int *, const float *,              \
        const unsigned long long *, int, const float *, float, const uint32_t *, const uint32_t *, uint32_t
template __global__ void interventional_kernel<true>(TAHOE_IV_KERNEL_ARGS);
template __global__ void interventional_kernel<false>(TAHOE_IV_KERNEL_ARGS);
template __global__ void interventional_kernel<true, true>(TAHOE_IV_KERNEL_ARGS);
template __global__ void interventional_kernel<false, true>(TAHOE_IV_KERNEL_ARGS);
#undef TAHOE_IV_KERNEL_ARGS

namespace {

// Rows of a workgroup's tile and its LDS bytes, by num_cols alone: the largest power of two <= kIvMaxTileRows whose row tile, four
// slabs and the weight table fit kIvLdsBudget, else one row in the whole LDS (the table in LDS if it still fits)
struct IvShape {
    int rows;
    bool wlds;
    size_t lds_bytes;
};

IvShape iv_shape(const tahoe_forest *f)
{
    const size_t per_row = 5 * (size_t)f->p.num_cols * sizeof(float), table = kIvTable * sizeof(float);
    size_t R = kIvMaxTileRows;
    while (R > 1 && R * per_row + table > kIvLdsBudget) R /= 2;
    const bool wlds = R * per_row + table <= (size_t)f->lds_limit;
    return {(int)R, wlds, R * per_row + (wlds ? table : 0)};
}

void free_istate(tahoe_istate *iv)
{
    if (!iv) return;
    if (iv->masks) (void)hipFree(iv->masks);
    if (iv->consts) (void)hipFree(iv->consts);
    delete iv;
}

// Where a handle's path bins live: tahoe_cstate (dense, sparse and multi-class handles: every class's bins, class-major) or the
// one set of a vector-leaf handle created with TAHOE_CREATE_INTERVENTIONAL, which carries no category sets
struct IvBins {
    const uint4 *elems;
    size_t bins;
    const uint32_t *elem_set, *set_pool;
    uint32_t set_words;
};

IvBins iv_bins(const tahoe_forest *f)
{
    if (f->vl) return {f->vl->shap->elems, (size_t)f->vl->shap->bins, nullptr, nullptr, 0u};
    const tahoe_cstate *cs = f->cs;
    return {cs->elems, cs->bins, cs->elem_set, cs->set_pool, cs->set_words};
}

// The kernels that read the background may need more than the default 64 KiB of dynamic LDS
hipError_t iv_allow_lds(const tahoe_forest *f)
{
    if (f->vl) return vector_iv_allow_lds(f);
    hipError_t e = hipSuccess;
    if ((e = allow_max_lds(reinterpret_cast<const void *>(&interventional_kernel<true>), f->lds_limit)) != hipSuccess ||
        (e = allow_max_lds(reinterpret_cast<const void *>(&interventional_kernel<false>), f->lds_limit)) != hipSuccess ||
        (f->cs->elem_set &&
         ((e = allow_max_lds(reinterpret_cast<const void *>(&interventional_kernel<true, true>), f->lds_limit)) != hipSuccess ||
          (e = allow_max_lds(reinterpret_cast<const void *>(&interventional_kernel<false, true>), f->lds_limit)) != hipSuccess)))
        return e;
    return hipSuccess;
}

}  // namespace

void launch_background_masks(unsigned long long *masks, const float *bg_dev, size_t bg_rows, int num_cols, size_t bins,
                             const uint4 *elems, float missing, hipStream_t stream)
{
    hipLaunchKernelGGL(background_mask_kernel<false>, dim3((unsigned)((bins + kContribWaves - 1) / kContribWaves)), dim3(256), 0, stream,
                       masks, bg_dev, bg_rows, num_cols, bins, elems, missing, nullptr, nullptr, 0u);
}

void interventional_destroy(tahoe_forest *f)
{
    if (!f->iv) return;
    f->device_bytes -= f->iv->bytes;
    free_istate(f->iv);
    f->iv = nullptr;
}

}  // namespace tahoe

using namespace tahoe;

extern "C" tahoe_status tahoe_forest_set_background(tahoe_forest *f, const float *bg_dev, size_t bg_rows, void *stream)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_background: null forest");
    if (tahoe_status st = need_background_tables(f, "tahoe_forest_set_background")) return st;
    if (bg_rows > 0 && !bg_dev) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_background: null background");
    if (f->ob) return oblivious_set_background(f, bg_dev, bg_rows, (hipStream_t)stream);  // no path bins: a histogram of leaf indices
    // one body for both kinds of handle: a vector-leaf handle has num_classes = K, class_trees = num_trees and one set of bins
    const IvBins pb = iv_bins(f);
    const size_t F = (size_t)f->p.num_cols, C = (size_t)f->num_classes, bins = pb.bins;
    if (F > 0 && bg_rows > SIZE_MAX / sizeof(float) / F)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_background: rows x num_cols floats overflow size_t (rows %zu)", bg_rows);
    if (bg_rows > (size_t)INT32_MAX)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_set_background: %zu background rows (at most 2^31 - 1)", bg_rows);
    DeviceGuard on_device(f->device);
    hipStream_t s = (hipStream_t)stream;
    if (bg_rows == 0) {
        interventional_destroy(f);
        return TAHOE_OK;
    }
    if (bins > 0 && bg_rows > SIZE_MAX / sizeof(unsigned long long) / bins)
        return fail(TAHOE_ERR_NO_MEMORY, "tahoe_forest_set_background: %zu bins x %zu rows of 8-byte masks overflow size_t", bins,
                    bg_rows);
    const size_t mask_bytes = std::max<size_t>(bins * bg_rows * sizeof(unsigned long long), 1);
    const size_t const_bytes = (kIvTable + C) * sizeof(float);

    // the weight table and the bias column are made on the host; the old background stays until the new one is complete
    std::vector<float> h_consts(kIvTable + C, 0.0f);
    for (int p = 1; p < 32; ++p)
        for (int q = 0; p + q < 32; ++q) {
            double binom = 1.0;  // C(p + q, q), exact in float64 (<= C(31, 15))
            for (int k = 1; k <= q; ++k) binom = binom * (double)(p + k) / (double)k;
            h_consts[p * 32 + q] = (float)(1.0 / ((double)p * binom));
        }
    tahoe_istate *iv = new (std::nothrow) tahoe_istate();
    if (!iv) return fail(TAHOE_ERR_NO_MEMORY, "tahoe_forest_set_background");
    float *sums = nullptr;
    auto bail = [&](tahoe_status st) {
        if (sums) (void)hipFree(sums);
        free_istate(iv);
        (void)hipGetLastError();  // a failed allocation is not the caller's next error
        return st;
    };
    if (hipMalloc(reinterpret_cast<void **>(&iv->masks), mask_bytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&iv->consts), const_bytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&sums), bg_rows * C * sizeof(float)) != hipSuccess)
        return bail(fail(TAHOE_ERR_NO_MEMORY, "tahoe_forest_set_background: %zu bytes of background masks (%zu bins x %zu rows) do "
                                              "not fit on the device; the previous background is kept",
                         mask_bytes, bins, bg_rows));
    iv->bg_rows = bg_rows;
    iv->bytes = mask_bytes + const_bytes;
    if (bins > 0) {
        if (pb.elem_set)
            hipLaunchKernelGGL(background_mask_kernel<true>, dim3((unsigned)((bins + kContribWaves - 1) / kContribWaves)), dim3(256), 0, s,
                               iv->masks, bg_dev, bg_rows, (int)F, bins, pb.elems, f->p.missing, pb.elem_set, pb.set_pool,
                               pb.set_words);
        else
            launch_background_masks(iv->masks, bg_dev, bg_rows, (int)F, bins, pb.elems, f->p.missing, s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return bail(fail(TAHOE_ERR_HIP, "tahoe_forest_set_background: mask kernel: %s", hipGetErrorString(e)));
    }
    // raw_c(r): tahoe_forest_predict_raw's bits (the same under every strategy); DIRECT serves every dense shape and allocates
    // nothing (on a sparse handle it is sparse_kernel, on a vector-leaf handle vector_direct_kernel).  The caller's strategy
    // setting is restored.
    const int saved = f->strategy;
    f->strategy = TAHOE_STRATEGY_DIRECT;
    const tahoe_status st = tahoe_forest_predict_raw(f, sums, bg_dev, bg_rows, stream);
    f->strategy = saved;
    if (st != TAHOE_OK) return bail(st);
    std::vector<float> raw(bg_rows * C);
    hipError_t e = hipMemcpyAsync(raw.data(), sums, raw.size() * sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return bail(fail(TAHOE_ERR_HIP, "tahoe_forest_set_background: %s", hipGetErrorString(e)));
    const size_t Tc = (size_t)f->class_trees;
    const bool avg = (f->p.output & TAHOE_OUT_AVG) != 0 && Tc > 0;
    for (size_t c = 0; c < C; ++c) {
        double sum = 0.0;
        for (size_t r = 0; r < bg_rows; ++r) sum += (double)raw[r * C + c];
        double m = sum / (double)bg_rows;
        if (avg) m /= (double)Tc;
        h_consts[kIvTable + c] = (float)(m + (double)f->p.global_bias);
    }
    e = hipMemcpyAsync(iv->consts, h_consts.data(), const_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return bail(fail(TAHOE_ERR_HIP, "tahoe_forest_set_background: %s", hipGetErrorString(e)));
    (void)hipFree(sums);
    sums = nullptr;
    if ((e = iv_allow_lds(f)) != hipSuccess)
        return bail(fail(TAHOE_ERR_HIP, "hipFuncSetAttribute(interventional) failed: %s", hipGetErrorString(e)));
    interventional_destroy(f);
    f->iv = iv;
    f->device_bytes += iv->bytes;
    return TAHOE_OK;
}

extern "C" tahoe_status tahoe_forest_predict_contribs_interventional(tahoe_forest *f, float *phi_dev, const float *data_dev,
                                                                     size_t rows, void *stream)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_contribs_interventional: null forest");
    if (tahoe_status st = need_background_tables(f, "tahoe_forest_predict_contribs_interventional")) return st;
    if (f->ob)
        return oblivious_predict_interventional(f, phi_dev, data_dev, rows, (hipStream_t)stream,
                                                "tahoe_forest_predict_contribs_interventional");
    if (!f->iv)
        return fail(TAHOE_ERR_UNSUPPORTED, "tahoe_forest_predict_contribs_interventional: no background set "
                                           "(tahoe_forest_set_background)");
    if (rows == 0) return TAHOE_OK;
    if (!phi_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_contribs_interventional: null argument");
    if (tahoe_status st = check_shap_out(f, rows, 1, "tahoe_forest_predict_contribs_interventional")) return st;
    if (f->vl)
        return vector_predict_interventional(f, phi_dev, data_dev, rows, (hipStream_t)stream, "tahoe_forest_predict_contribs_interventional");
    const int F = f->p.num_cols, C = f->num_classes;
    const IvShape sh = iv_shape(f);
    const size_t grid = (rows + (size_t)sh.rows - 1) / (size_t)sh.rows;
    if (grid > 0x7fffffffu)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_contribs_interventional: too many rows for one launch: %zu", rows);
    const tahoe_cstate *cs = f->cs;
    const tahoe_istate *iv = f->iv;
    DeviceGuard on_device(f->device);
    auto launch = [&](auto wlds, auto sets) {
        hipLaunchKernelGGL((interventional_kernel<decltype(wlds)::value, decltype(sets)::value>), dim3((unsigned)grid), dim3(256),
                           sh.lds_bytes, (hipStream_t)stream, phi_dev, data_dev, rows, F, C, sh.rows, cs->elems, cs->bin_info,
                           cs->class_bins, cs->class_div, iv->masks, (int)iv->bg_rows, iv->consts, f->p.missing, cs->elem_set,
                           cs->set_pool, cs->set_words);
    };
    if (sh.wlds) {
        if (cs->elem_set) launch(std::true_type{}, std::true_type{});
        else launch(std::true_type{}, std::false_type{});
    } else if (cs->elem_set) {
        launch(std::false_type{}, std::true_type{});
    } else {
        launch(std::false_type{}, std::false_type{});
    }
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}
