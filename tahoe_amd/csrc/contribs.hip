// Per-feature contributions: path-dependent TreeSHAP (Lundberg et al. 2018, Algorithm 2) in the lane-per-path-element form of
// GPUTreeShap (Mitchell et al. 2022).  Create (TAHOE_CREATE_CONTRIBS) turns every reachable leaf into a path -- its ancestors'
// features, repeated ones merged into one element -- and packs the paths into 64-lane bins; the kernel evaluates, for each row,
// every bin with one lane per path element: one-fraction by the library's branch rule, the extend recursion across the lanes of
// a path, one unwound-path sum per lane, and the lane's term added into its row's phi[feature] in a fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "forest_internal.h"
#include "contribs_internal.h"
#include "treeshap_lanes.h"

namespace tahoe {

// One workgroup = a tile of R rows (staged in LDS) x all bins; wave w evaluates bins w, w + 4, ... of each class into its own
// slab [R][F] of LDS; the four slabs are then summed in wave order and written out.  Every row sees the same operations in the
// same order whatever its batch, tile or position: results are bitwise reproducible.
// SPARE = false: phi[rows][C][F + 1] (contribs_kernel).  SPARE = true: the same values into row F of each (row, class) matrix of
// out[rows][C][F + 1][F + 1] (tahoe_forest_predict_interactions, contribs_spare_kernel).
// SETS (a handle whose path elements carry category sets): the one-fraction is follows_set() on elem_set / set_pool.
template <bool SPARE, bool SETS>
__device__ __forceinline__ void contribs_tile(float *__restrict__ phi, const float *__restrict__ data, size_t rows, int F, int C,
                                              int R, const uint4 *__restrict__ elems, const float *__restrict__ one_minus_z,
                                              const uint32_t *__restrict__ bin_info, const int *__restrict__ class_bins,
                                              const float *__restrict__ bias, const float *__restrict__ class_div, float missing,
                                              const uint32_t *__restrict__ elem_set, const uint32_t *__restrict__ set_pool,
                                              uint32_t set_words)
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
    float *slab = smem + slab_n * (1 + wave);
    const float *s0 = smem + slab_n, *s1 = s0 + slab_n, *s2 = s1 + slab_n, *s3 = s2 + slab_n;
    const float *src = data + row0 * F;
    for (int i = tid; i < tile_n; i += 256) tile[i] = src[i];
    const size_t mat = (size_t)(F + 1) * (F + 1);
    const size_t out_row = SPARE ? (size_t)C * mat : (size_t)C * (F + 1);

    for (int c = 0; c < C; ++c) {
        for (int i = lane; i < tile_n; i += 64) slab[i] = 0.0f;
        __syncthreads();
        const int b_end = class_bins[c + 1];
        for (int b = class_bins[c] + wave; b < b_end; b += kContribWaves) {
            const uint4 e = elems[(size_t)b * 64 + lane];
            const float om = one_minus_z[(size_t)b * 64 + lane];
            const uint32_t info = bin_info[b];
            const int steps = (int)(info & 0xffu), rounds = (int)(info >> 8);
            const float lower = __uint_as_float(e.x), upper = __uint_as_float(e.y), z = __uint_as_float(e.z);
            const int fid = elem_fid(e.w), rank = elem_rank(e.w), ud = elem_ud(e.w), round = elem_round(e.w);
            const bool missing_ok = elem_missing_ok(e.w), nan_ok = elem_nan_ok(e.w);
            const int gs = lane - rank;  // lane of the path's root element
            const float leaf = lane_read(lower, gs);
            const float zdiv = z / (float)(ud + 1);
            const float udp1 = (float)(ud + 1);
            const int split = unwind_split(z, ud);
            ElemSet es{};
            bool gather = false;
            if constexpr (SETS) {
                es = elem_set_load(elem_set, set_pool, set_words, (size_t)b * 64 + lane);
                gather = elem_sets_gather(es);
            }
            for (int r = 0; r < nr; ++r) {
                bool o;
                if constexpr (SETS) o = follows_set(tile[r * F + fid], lower, upper, missing_ok, nan_ok, missing, es, set_pool, set_words, gather);
                else o = follows(tile[r * F + fid], lower, upper, missing_ok, nan_ok, missing);
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
                const float term = total * (o ? om : -z) * leaf;  // (one - zero) x leaf
                // two lanes of a bin on one feature add in lane order (round = earlier lanes of the bin on that feature)
                for (int k = 0; k < rounds; ++k)
                    if (rank != 0 && round == k) slab[r * F + fid] += term;
            }
        }
        __syncthreads();
        const float div = class_div[c];
        for (int i = tid; i < tile_n; i += 256) {
            const int r = i / F, col = i - r * F;
            const float v = ((s0[i] + s1[i]) + s2[i]) + s3[i];
            phi[(row0 + r) * out_row + (size_t)c * (SPARE ? mat : (F + 1)) + col] = v / div;
        }
        for (int r = tid; r < nr; r += 256) phi[(row0 + r) * out_row + (size_t)c * (SPARE ? mat : (F + 1)) + F] = bias[c];
        __syncthreads();
    }
}

template <bool SETS = false>
__global__ __launch_bounds__(256) void contribs_kernel(float *__restrict__ phi, const float *__restrict__ data, size_t rows, int F,
                                                       int C, int R, const uint4 *__restrict__ elems,
                                                       const float *__restrict__ one_minus_z,
                                                       const uint32_t *__restrict__ bin_info, const int *__restrict__ class_bins,
                                                       const float *__restrict__ bias, const float *__restrict__ class_div,
                                                       float missing, const uint32_t *__restrict__ elem_set,
                                                       const uint32_t *__restrict__ set_pool, uint32_t set_words)
{
    contribs_tile<false, SETS>(phi, data, rows, F, C, R, elems, one_minus_z, bin_info, class_bins, bias, class_div, missing, elem_set,
                               set_pool, set_words);
}

// ---- SHAP interaction values (tahoe_forest_predict_interactions) ----
// Output: out[row][c] is an (F + 1) x (F + 1) matrix M.  contribs_spare_kernel first writes phi, with contribs_kernel's exact
// bits, into its row F (a row that ends up all zero but the bias corner, so it serves as scratch); interactions_kernel then
// writes the rest.  Off-diagonal: for every path, every conditioning element k (rank 1 .. L - 2) and every element j of rank > k,
// the term leaf (o_j - z_j)(o_k - z_k) U_j(P \ {k}) / 2 goes into both M[fid_k][fid_j] and M[fid_j][fid_k], where U_j(P \ {k})
// is j's unwound-path sum on the path with k removed (XGBoost's PredictInteractionContributions, GPUTreeShap's conditioned
// TreeSHAP).  Lanes of one bin that hit the same feature pair at the same k add in lane order (one round per earlier lane on
// that pair); both entries of a pair see the same adds in the same order, so M is exactly symmetric.  Diagonal: M[i][i] =
// phi_i - sum_{j != i} M[i][j] (ascending j from 0.0f), with phi_i read back from row F.
//
// Two forms, fixed per handle at create by F alone:
//   SLABS (4 (F^2 + F / 4) floats per row fit 80 KiB, F <= 71): a workgroup of R rows; wave w evaluates bins w, w + 4, ... of a
//     class into its own LDS slab [R][F][F]; the slabs are summed in wave order, as contribs_kernel does.
//   in place (wider rows): wave w of a workgroup owns row 4 blockIdx + w and evaluates every bin of a class in order, adding
//     straight into that row's matrix in the output; dependent read-modify-writes of one wave are separated by an explicit
//     s_waitcnt vmcnt(0).
constexpr int kInterSlabMaxBytes = 80 * 1024;
constexpr int kInterMaxRows = 32;  // rows of a tile: one bit each in the per-lane one-fraction mask

template <bool SETS = false>
__global__ __launch_bounds__(256) void contribs_spare_kernel(float *__restrict__ out, const float *__restrict__ data, size_t rows,
                                                             int F, int C, int R, const uint4 *__restrict__ elems,
                                                             const float *__restrict__ one_minus_z,
                                                             const uint32_t *__restrict__ bin_info,
                                                             const int *__restrict__ class_bins, const float *__restrict__ bias,
                                                             const float *__restrict__ class_div, float missing,
                                                             const uint32_t *__restrict__ elem_set,
                                                             const uint32_t *__restrict__ set_pool, uint32_t set_words)
{
    contribs_tile<true, SETS>(out, data, rows, F, C, R, elems, one_minus_z, bin_info, class_bins, bias, class_div, missing, elem_set,
                              set_pool, set_words);
}

// The off-diagonal terms of bins b_first, b_first + b_step, ... < b_end for the nr rows of `tile` (row r at tile + r F), added
// into acc + r acc_row + a ld + b for the pair (a, b).
template <bool SLABS, bool SETS>
__device__ __forceinline__ void interaction_bins(float *acc, size_t acc_row, int ld, const float *tile, int nr, int F, int b_first,
                                                 int b_end, int b_step, const uint4 *__restrict__ elems,
                                                 const float *__restrict__ one_minus_z, const uint32_t *__restrict__ bin_info,
                                                 float missing, const uint32_t *__restrict__ elem_set,
                                                 const uint32_t *__restrict__ set_pool, uint32_t set_words)
{
    const int lane = threadIdx.x & 63;
    if (nr == 0) return;  // a wave past the last row (in place)
    for (int b = b_first; b < b_end; b += b_step) {
        const int steps = (int)(bin_info[b] & 0xffu);
        if (steps < 3) continue;  // no path with two features
        const uint4 e = elems[(size_t)b * 64 + lane];
        const float om = one_minus_z[(size_t)b * 64 + lane];
        const float lower = __uint_as_float(e.x), upper = __uint_as_float(e.y), z = __uint_as_float(e.z);
        const int fid = elem_fid(e.w), rank = elem_rank(e.w), ud = elem_ud(e.w);
        const bool missing_ok = elem_missing_ok(e.w), nan_ok = elem_nan_ok(e.w);
        const int gs = lane - rank;  // lane of the path's root element
        const float leaf = lane_read(lower, gs);
        // one-fractions of this lane's element, bit r for row r
        uint32_t omask = 0;
        if constexpr (SETS) {
            const ElemSet es = elem_set_load(elem_set, set_pool, set_words, (size_t)b * 64 + lane);
            const bool gather = elem_sets_gather(es);
            for (int r = 0; r < nr; ++r)
                omask |= (follows_set(tile[r * F + fid], lower, upper, missing_ok, nan_ok, missing, es, set_pool, set_words, gather) ? 1u : 0u) << r;
        } else {
            for (int r = 0; r < nr; ++r) omask |= (follows(tile[r * F + fid], lower, upper, missing_ok, nan_ok, missing) ? 1u : 0u) << r;
        }
        // on the path without element k, element j (rank > k) has unique depth ud - 1
        const int udk = ud - 1;
        const float zdiv = z / (float)max(ud, 1);
        const float udkp1 = (float)ud;
        for (int k = 1; k <= steps - 2; ++k) {
            const int lk = min(gs + k, 63);
            const int fk = (int)lane_read_u((uint32_t)fid, lk);
            const float om_k = lane_read(om, lk), z_k = lane_read(z, lk);
            const uint32_t omask_k = lane_read_u(omask, lk);
            const bool pair = rank > k;
            const uint64_t pairs = __ballot(pair);
            if (pairs == 0) continue;
            // order of the adds: earlier lanes of the bin on the same unordered pair {fid, fk} (row-independent)
            const uint32_t key = pair ? (uint32_t)min(fid, fk) << 15 | (uint32_t)max(fid, fk) : 0xffffffffu;
            int round = 0;
            for (uint64_t m = pairs; m; m &= m - 1) {
                const int l = __builtin_ctzll(m);
                round += ((uint32_t)__builtin_amdgcn_readlane((int)key, l) == key && l < lane) ? 1 : 0;
            }
            int rounds = 0;
            while (__ballot(pair && round >= rounds)) ++rounds;
            const int nrk = rank > k ? rank - 1 : rank;  // position on the path without element k
            const bool skip_left = rank == k + 1;        // the left neighbour on that path is two lanes down
            for (int r = 0; r < nr; ++r) {
                const bool o = (omask >> r) & 1u, ok = (omask_k >> r) & 1u;
                const uint32_t zo = e.z | (o ? 0x80000000u : 0u);
                // extend over the path without element k: after step d, positions <= d hold the permutation weights
                float pw = rank == 0 ? 1.0f : 0.0f;
                for (int d = 1; d < steps - 1; ++d) {
                    const uint32_t s = lane_read_u(zo, min(gs + (d < k ? d : d + 1), 63));
                    const float zd = __uint_as_float(s & 0x7fffffffu), od = (s >> 31) ? 1.0f : 0.0f;
                    const float left1 = from_left_lane(pw);
                    const float left2 = from_left_lane(left1);
                    const float left = skip_left ? left2 : left1;
                    const float inv = c_inv[d + 1];
                    const float a = (float)max(d - nrk, 0) * inv, bb = (float)nrk * inv;
                    const float np = pw * zd * a + od * left * bb;
                    pw = d <= udk ? np : pw;
                }
                // unwound-path sum of this lane's element on that path
                float next = lane_read(pw, min(gs + ud, 63));
                float total = 0.0f;
                for (int i = steps - 3; i >= 0; --i) {
                    const float pwi = lane_read(pw, min(gs + (i < k ? i : i + 1), 63));
                    const float pre = (float)(udk - i) * zdiv;
                    const float tmp = next * udkp1 * c_inv[i + 1];
                    const float t_one = total + tmp, n_one = pwi - tmp * pre;
                    const float t_zero = pre > 0.0f ? total + pwi * __builtin_amdgcn_rcpf(pre) : total;
                    if (i < udk) {
                        total = o ? t_one : t_zero;
                        next = o ? n_one : next;
                    }
                }
                const float term = total * (o ? om : -z) * leaf * ((ok ? om_k : -z_k) * 0.5f);
                float *pa = acc + r * acc_row + (size_t)fk * ld + fid, *pb = acc + r * acc_row + (size_t)fid * ld + fk;
                for (int q = 0; q < rounds; ++q) {
                    if (pair && round == q) {
                        *pa += term;
                        *pb += term;
                    }
                    if (!SLABS) vm_drain();
                }
            }
        }
    }
}

template <bool SLABS, bool SETS = false>
__global__ __launch_bounds__(256) void interactions_kernel(float *out, const float *__restrict__ data, size_t rows, int F, int C,
                                                           int R, const uint4 *__restrict__ elems,
                                                           const float *__restrict__ one_minus_z,
                                                           const uint32_t *__restrict__ bin_info,
                                                           const int *__restrict__ class_bins, const float *__restrict__ bias,
                                                           const float *__restrict__ class_div, float missing,
                                                           const uint32_t *__restrict__ elem_set,
                                                           const uint32_t *__restrict__ set_pool, uint32_t set_words)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F1 = F + 1;
    const size_t mat = (size_t)F1 * F1;
    const size_t tile_rows = SLABS ? (size_t)R : (size_t)R * kContribWaves;
    const size_t row0 = (size_t)blockIdx.x * tile_rows;
    const int nt = (int)min(tile_rows, rows - row0);
    float *tile = smem;
    const float *src = data + row0 * F;
    for (int i = tid; i < nt * F; i += 256) tile[i] = src[i];
    __syncthreads();

    if (SLABS) {
        const int FF = F * F;
        const size_t slab_n = (size_t)R * FF;
        float *s0 = smem + (size_t)R * F, *s1 = s0 + slab_n, *s2 = s1 + slab_n, *s3 = s2 + slab_n;
        float *slab = s0 + slab_n * wave;
        for (int c = 0; c < C; ++c) {
            for (int i = lane; i < nt * FF; i += 64) slab[i] = 0.0f;
            __syncthreads();
            interaction_bins<true, SETS>(slab, (size_t)FF, F, tile, nt, F, class_bins[c] + wave, class_bins[c + 1], kContribWaves,
                                         elems, one_minus_z, bin_info, missing, elem_set, set_pool, set_words);
            __syncthreads();
            const float div = class_div[c];
            for (int i = tid; i < nt * FF; i += 256) s0[i] = (((s0[i] + s1[i]) + s2[i]) + s3[i]) / div;
            __syncthreads();
            // diagonal: phi_i (row F of the output) - the row's off-diagonal sum in ascending j
            for (int t = tid; t < nt * F; t += 256) {
                const int r = t / F, i = t - r * F;
                float *m = s0 + (size_t)r * FF + (size_t)i * F;
                float sum = 0.0f;
                for (int j = 0; j < F; ++j)
                    if (j != i) sum += m[j];
                m[i] = out[((row0 + r) * C + c) * mat + (size_t)F * F1 + i] - sum;
            }
            __syncthreads();
            for (int r = 0; r < nt; ++r)
                for (int p = tid; p < F1 * F1; p += 256) {
                    const int a = p / F1, b = p - a * F1;
                    out[((row0 + r) * C + c) * mat + p] = a < F && b < F ? s0[r * FF + a * F + b] : (a == F && b == F ? bias[c] : 0.0f);
                }
            __syncthreads();
        }
    } else {
        const int rw0 = wave * R;
        const int nr = max(0, min(R, nt - rw0));
        const float *wtile = tile + (size_t)rw0 * F;
        const size_t row_stride = (size_t)C * mat;
        for (int c = 0; c < C; ++c) {
            float *acc = out + ((row0 + rw0) * C + c) * mat;
            for (int r = 0; r < nr; ++r)
                for (size_t i = lane; i < (size_t)F * F1; i += 64) acc[r * row_stride + i] = 0.0f;
            vm_drain();
            interaction_bins<false, SETS>(acc, row_stride, F1, wtile, nr, F, class_bins[c], class_bins[c + 1], 1, elems, one_minus_z,
                                          bin_info, missing, elem_set, set_pool, set_words);
            const float div = class_div[c];
            for (int r = 0; r < nr; ++r) {
                float *m = acc + r * row_stride;
                if (div != 1.0f) {  // x / 1.0f is x: skipping the pass changes no bit
                    for (size_t i = lane; i < (size_t)F * F1; i += 64) m[i] = m[i] / div;
                    vm_drain();
                }
                for (int i = lane; i < F; i += 64) {
                    const float *mi = m + (size_t)i * F1;
                    float sum = 0.0f;
                    for (int j = 0; j < F; ++j)
                        if (j != i) sum += mi[j];
                    m[(size_t)i * F1 + i] = m[(size_t)F * F1 + i] - sum;
                    m[(size_t)i * F1 + F] = 0.0f;
                }
                vm_drain();
                for (int i = lane; i < F; i += 64) m[(size_t)F * F1 + i] = 0.0f;
            }
        }
    }
}

#define TAHOE_SHAP_KERNEL_ARGS                                                                                                     \
    float *, const float *, size_t, int, int, int, const uint4 *, const float *, const uint32_t *, const int *, const float *,   \
        const float *, float, const uint32_t *, const uint32_t *, uint32_t
template __global__ void contribs_kernel<false>(TAHOE_SHAP_KERNEL_ARGS);
template __global__ void contribs_kernel<true>(TAHOE_SHAP_KERNEL_ARGS);
template __global__ void contribs_spare_kernel<false>(TAHOE_SHAP_KERNEL_ARGS);
template __global__ void contribs_spare_kernel<true>(TAHOE_SHAP_KERNEL_ARGS);
template __global__ void interactions_kernel<true>(TAHOE_SHAP_KERNEL_ARGS);
template __global__ void interactions_kernel<false>(TAHOE_SHAP_KERNEL_ARGS);
template __global__ void interactions_kernel<true, true>(TAHOE_SHAP_KERNEL_ARGS);
template __global__ void interactions_kernel<false, true>(TAHOE_SHAP_KERNEL_ARGS);
#undef TAHOE_SHAP_KERNEL_ARGS

tahoe_status contribs_validate(const tahoe_dense_node *nodes, const tahoe_forest_params *p)
{
    const size_t per = (size_t)tahoe_tree_num_nodes(p->depth);
    for (int t = 0; t < p->num_trees; ++t) {
        const tahoe_dense_node *tree = nodes + (size_t)t * per;
        std::vector<size_t> stack{0};
        while (!stack.empty()) {
            const size_t i = stack.back();
            stack.pop_back();
            if ((tree[i].bits >> 31) & 1) continue;  // leaf
            const size_t l = 2 * i + 1, r = 2 * i + 2;
            if (r >= per) continue;  // a non-leaf on the bottom level: create's structural check reports it
            const float wl = tree[l].weight, wr = tree[r].weight;
            if (!std::isfinite(wl) || !std::isfinite(wr) || !(wl >= 0.0f) || !(wr >= 0.0f) || !((double)wl + (double)wr > 0.0))
                return fail(TAHOE_ERR_INVALID_FOREST,
                            "tree %d node %zu: child weights %g and %g (TAHOE_CREATE_CONTRIBS needs finite covers >= 0 with a "
                            "positive sum at every reachable internal node)",
                            t, i, (double)wl, (double)wr);
            stack.push_back(r);
            stack.push_back(l);
        }
    }
    return TAHOE_OK;
}

namespace {

struct TreePaths {
    std::vector<uint4> elems;       // paths one after the other, root element first, rank / length / round not yet set
    std::vector<float> om;          // 1 - zero fraction of each element
    std::vector<unsigned char> len;  // elements per path
    double expect = 0.0;             // E_t (tree_expect)
    // category sets (a tree with categorical splits): per element 0 = none, else 1 + its index in sets; a set is its pool
    // entry, header first
    std::vector<uint32_t> set_of;
    std::vector<std::vector<uint32_t>> sets;
};

struct Elem {
    int fid;
    float lower, upper;
    bool missing_ok, nan_ok;
    double rho;
    // the categorical edges of the feature, folded: ids below 32 set.size() are allowed where their bit is set, every other
    // non-missing value (beyond the words, negative, >= 2^24, NaN) iff outside_ok
    bool has_set = false, outside_ok = true;
    std::vector<uint32_t> set;
    // One more edge: the path needs member == need of a split with nw words.  A shorter set is zero-extended; the ids a
    // growing element gains were outside its words so far.
    void fold(const uint32_t *words, size_t nw, bool need)
    {
        has_set = true;
        if (nw > set.size()) set.resize(nw, outside_ok ? ~0u : 0u);
        for (size_t i = 0; i < set.size(); ++i) {
            const uint32_t w = i < nw ? words[i] : 0u;
            set[i] &= need ? w : ~w;
        }
        outside_ok = outside_ok && !need;
    }
};

inline uint32_t float_word(float v)
{
    uint32_t w;
    memcpy(&w, &v, 4);
    return w;
}

// The two node formats as one tree for tree_paths: val, bits (fid[0:29] | def_left << 30 | is_leaf << 31 in both), the left
// child (the right one follows it), a node's cover, and what a leaf's root element carries in .x (leaf_word: the leaf value).
struct DenseTree {
    const tahoe_dense_node *n;
    int cat(size_t) const { return -1; }
    float val(size_t i) const { return n[i].val; }
    uint32_t leaf_word(size_t i) const { return float_word(n[i].val); }
    int32_t bits(size_t i) const { return n[i].bits; }
    size_t left(size_t i) const { return 2 * i + 1; }
    double cover(size_t i) const { return n[i].weight; }
};
struct SparseTree {
    const tahoe_sparse_node *n;
    const float *covers;  // parallel to n
    const tahoe_categorical_splits *cats = nullptr;  // the handle's categorical splits (null: none) ...
    int32_t root = 0;                                // ... whose node[] counts from the forest's first node: n = nodes + root
    // the categorical split at node i, or -1 (a numeric node, whose val is its threshold)
    int cat(size_t i) const
    {
        if (!cats) return -1;
        const int32_t g = root + (int32_t)i;
        const int32_t *end = cats->node + cats->num_splits, *it = std::lower_bound(cats->node, end, g);
        return it != end && *it == g ? (int)(it - cats->node) : -1;
    }
    float val(size_t i) const { return n[i].val; }
    uint32_t leaf_word(size_t i) const { return float_word(n[i].val); }
    int32_t bits(size_t i) const { return n[i].bits; }
    size_t left(size_t i) const { return (size_t)n[i].left_idx; }
    double cover(size_t i) const { return covers[i]; }
};
// A tree of a vector-leaf handle for tree_paths: a leaf's root element carries the index of the leaf's vector
struct VectorTree : SparseTree {
    uint32_t leaf_word(size_t i) const { return (uint32_t)n[i].left_idx; }
};
// ... of a handle created with TAHOE_CREATE_INTERVENTIONAL alone: every cover reads 1.  tree_paths uses covers for z and 1 - z
// only -- features, bounds, missing_ok / nan_ok and lengths do not depend on them -- and that game reads neither.
struct VectorTreeUnit : VectorTree {
    double cover(size_t) const { return 1.0; }
};
// ... and for tree_expect: element k of the leaf's vector as the leaf value
struct VectorTreeK : SparseTree {
    const float *leaves;
    size_t K, k;
    float val(size_t i) const { return ((n[i].bits >> 31) & 1) ? leaves[(size_t)n[i].left_idx * K + k] : n[i].val; }
};

// E_t: the sum over reachable leaves, pre-order (left before right), of leaf x the product of the cover ratios of its edges,
// multiplied root first (float64).  The bias column of every TreeSHAP form and of the Saabas form (approx.hip).
template <typename Tree>
double tree_expect(const Tree &tree)
{
    struct Frame {
        size_t node;
        double prod;
    };
    std::vector<Frame> stack{{0, 1.0}};
    double expect = 0.0;
    while (!stack.empty()) {
        const Frame fr = stack.back();
        stack.pop_back();
        if ((tree.bits(fr.node) >> 31) & 1) {
            expect += (double)tree.val(fr.node) * fr.prod;
            continue;
        }
        const size_t l = tree.left(fr.node);
        const double wl = tree.cover(l), wr = tree.cover(l + 1);
        stack.push_back({l + 1, fr.prod * (wr / (wl + wr))});
        stack.push_back({l, fr.prod * (wl / (wl + wr))});
    }
    return expect;
}

template <typename Tree>
void tree_paths(const Tree &tree, TreePaths &out, const tahoe_categorical_splits *cats = nullptr)
{
    struct Edge {
        size_t node;
        bool right;
    };
    std::vector<Edge> edges;  // the path from the root: as long as the deepest leaf (sparse trees are not bounded by 32 levels)
    // iterative pre-order walk (left before right): leaves in heap order left to right
    struct Frame {
        size_t node, parent;
        int depth;
        bool right;
    };
    std::vector<Frame> stack{{0, 0, 0, false}};
    std::vector<Elem> el;
    while (!stack.empty()) {
        const Frame fr = stack.back();
        stack.pop_back();
        if (fr.depth > 0) {
            if (edges.size() < (size_t)fr.depth) edges.resize((size_t)fr.depth);
            edges[fr.depth - 1] = {fr.parent, fr.right};
        }
        if (!((tree.bits(fr.node) >> 31) & 1)) {
            const size_t l = tree.left(fr.node);
            stack.push_back({l + 1, fr.node, fr.depth + 1, true});
            stack.push_back({l, fr.node, fr.depth + 1, false});
            continue;
        }
        // repeated features are merged into their first element: at most 31 distinct ones (checked at create)
        el.clear();
        for (int k = 0; k < fr.depth; ++k) {
            const size_t a = edges[k].node;
            const int fid = tree.bits(a) & 0x3fffffff;
            const bool def_left = (tree.bits(a) >> 30) & 1;
            const float thr = tree.val(a);
            const double wl = tree.cover(tree.left(a)), wr = tree.cover(tree.left(a) + 1);
            const double rho = (edges[k].right ? wr : wl) / (wl + wr);
            size_t j = 0;
            while (j < el.size() && el[j].fid != fid) ++j;
            if (j == el.size()) el.push_back(Elem{fid, -INFINITY, NAN, true, true, 1.0, false, true, {}});
            Elem &m = el[j];
            m.rho *= rho;
            const int split = tree.cat(a);
            if (split >= 0) {  // member == (right != members_left); missing takes the default branch, NaN is no member
                const bool ml = cats->members_left && cats->members_left[split];
                m.fold(cats->words + cats->offset[split], (size_t)(cats->offset[split + 1] - cats->offset[split]),
                       edges[k].right != ml);
                m.missing_ok = m.missing_ok && (edges[k].right != def_left);
            } else if (edges[k].right) {  // x >= thr; NaN never satisfies it, missing does iff the default is right
                m.lower = (std::isnan(thr) || std::isnan(m.lower)) ? NAN : std::max(m.lower, thr);
                m.nan_ok = false;
                m.missing_ok = m.missing_ok && !def_left;
            } else {  // !(x >= thr); a NaN threshold sends every non-missing row left
                if (!std::isnan(thr)) m.upper = std::isnan(m.upper) ? thr : std::min(m.upper, thr);
                m.missing_ok = m.missing_ok && def_left;
            }
        }
        const int ne = (int)el.size();
        if (ne == 0) continue;  // a root leaf: all of it is bias
        uint4 root;
        root.x = tree.leaf_word(fr.node);
        root.y = 0u;
        const float one = 1.0f;
        memcpy(&root.z, &one, 4);
        root.w = 0u;
        out.elems.push_back(root);
        out.om.push_back(0.0f);
        for (int j = 0; j < ne; ++j) {
            uint4 u;
            // below kContribMinZ the zero fraction is stored as 0 (1 - z still from float64): the kernels' pre = (ud - i) z /
            // (ud + 1) is then 0 or >= 2^-126, never subnormal, so rcp(pre) stays finite.  Exact Shapley values are multilinear
            // in z with slopes <= |leaf|, so a path term changes by less than 2^-121 |leaf| per element cut.
            const float zf = el[j].rho < kContribMinZ ? 0.0f : (float)el[j].rho;
            memcpy(&u.x, &el[j].lower, 4);
            memcpy(&u.y, &el[j].upper, 4);
            memcpy(&u.z, &zf, 4);
            u.w = elem_word(el[j].fid, 0, 1, 0, el[j].missing_ok, el[j].nan_ok);
            out.elems.push_back(u);
            out.om.push_back((float)(1.0 - el[j].rho));
            if (el[j].has_set) {
                out.set_of.resize(out.elems.size(), 0u);
                out.sets.emplace_back(1, (el[j].outside_ok ? kSetOutsideOk : 0u) | (uint32_t)el[j].set.size());
                out.sets.back().insert(out.sets.back().end(), el[j].set.begin(), el[j].set.end());
                out.set_of.back() = (uint32_t)out.sets.size();
            }
        }
        out.len.push_back((unsigned char)(ne + 1));
    }
}

}  // namespace

// The bias column of every class from E_t of the caller's trees: sum_t E_t over class c's trees c, c + C, ... in order, / Tc with
// TAHOE_OUT_AVG, + global_bias, in float64, rounded once; div[c] = (float)Tc with AVG, else 1.0f.
static void class_bias(const tahoe_forest *f, const std::vector<double> &expect, std::vector<float> &bias, std::vector<float> &div)
{
    const int C = f->num_classes;
    const size_t Tc = (size_t)f->class_trees;
    const bool avg = (f->p.output & TAHOE_OUT_AVG) != 0 && Tc > 0;
    bias.assign((size_t)C, 0.0f);
    div.assign((size_t)C, 1.0f);
    for (int c = 0; c < C; ++c) {
        double sum = 0.0;
        for (size_t k = 0; k < Tc; ++k) sum += expect[k * (size_t)C + (size_t)c];
        bias[(size_t)c] = (float)((avg ? sum / (double)Tc : sum) + (double)f->p.global_bias);
        div[(size_t)c] = avg ? (float)Tc : 1.0f;
    }
}

void contribs_bias(const tahoe_forest *f, const tahoe_dense_node *nodes, std::vector<float> &bias, std::vector<float> &div)
{
    const size_t T = (size_t)f->p.num_trees, per = (size_t)tahoe_tree_num_nodes(f->p.depth);
    std::vector<double> expect(T);
    parallel_for(T, 16, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; ++t) expect[t] = tree_expect(DenseTree{nodes + t * per});
    });
    class_bias(f, expect, bias, div);
}

void contribs_bias_sparse(const tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers,
                          std::vector<float> &bias, std::vector<float> &div)
{
    const size_t T = (size_t)f->p.num_trees;
    std::vector<double> expect(T);
    parallel_for(T, 16, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; ++t) expect[t] = tree_expect(SparseTree{nodes + trees[t], covers + trees[t]});
    });
    class_bias(f, expect, bias, div);
}

// TAHOE_ERR_UNSUPPORTED unless a row tile and four slabs of one row each fit the LDS: 20 B per column
static tahoe_status check_contrib_cols(const tahoe_forest *f)
{
    const int F = f->p.num_cols;
    if (F > kContribMaxCols || 5 * (size_t)F * sizeof(float) > (size_t)f->lds_limit)
        return fail(TAHOE_ERR_UNSUPPORTED, "TAHOE_CREATE_CONTRIBS needs 20 B of LDS per column (num_cols %d; device offers %d B)", F,
                    f->lds_limit);
    return TAHOE_OK;
}

// The paths of every tree packed into 64-lane bins, on the host
struct PathBins {
    std::vector<uint4> elems;
    std::vector<float> om;
    std::vector<uint32_t> info;
    std::vector<uint32_t> set, pool;  // category sets: per lane 1 + the offset of its set's header, and the pool
    std::vector<int> class_bins;
    bool any_sets = false;
    size_t n_paths = 0, n_elems = 0;
};

// Next-fit packing of each class's paths, in tree order then leaf order: class c's trees are c, c + C, ... (Tc of them).  Padding
// lanes, ranks, lengths, rounds and bin_info are set here; the trees' paths are released as they are packed.
static void pack_paths(std::vector<TreePaths> &trees, int C, size_t Tc, PathBins &out)
{
    std::vector<uint4> &h_elems = out.elems;
    std::vector<float> &h_om = out.om;
    std::vector<uint32_t> &h_info = out.info;
    // category sets: the pool (identical sets share one entry) and, per lane, 1 + the offset of its set's header
    bool &any_sets = out.any_sets;
    for (const TreePaths &tp : trees) any_sets = any_sets || !tp.sets.empty();
    std::vector<uint32_t> &h_set = out.set, &h_pool = out.pool;
    std::map<std::vector<uint32_t>, uint32_t> pool_at;
    std::vector<uint32_t> tree_at;  // per set of the current tree: 1 + its header's offset
    std::vector<int> &h_class_bins = out.class_bins;
    h_class_bins.assign(C + 1, 0);
    size_t &n_paths = out.n_paths, &n_elems = out.n_elems;
    uint4 pad;
    {
        const float one = 1.0f;
        pad.x = pad.y = 0u;
        memcpy(&pad.z, &one, 4);
        pad.w = 0u;
    }
    for (int c = 0; c < C; ++c) {
        h_class_bins[c] = (int)(h_elems.size() / 64);
        size_t start = h_elems.size();
        int fill = 0, steps = 0;
        auto flush = [&]() {
            if (fill == 0) return;
            h_elems.resize(start + 64, pad);
            h_om.resize(start + 64, 0.0f);
            if (any_sets) h_set.resize(start + 64, 0u);
            int rounds = 0;
            for (int l = 0; l < 64; ++l) {
                uint4 &u = h_elems[start + l];
                if (elem_rank(u.w) == 0) continue;
                int round = 0;
                for (int k = 0; k < l; ++k) {
                    const uint4 &v = h_elems[start + k];
                    if (elem_rank(v.w) != 0 && elem_fid(v.w) == elem_fid(u.w)) ++round;
                }
                u.w |= (uint32_t)round << kElemRoundShift;
                rounds = std::max(rounds, round + 1);
            }
            h_info.push_back((uint32_t)steps | (uint32_t)rounds << 8);
            start = h_elems.size();
            fill = 0;
            steps = 0;
        };
        for (size_t k = 0; k < Tc; ++k) {
            const size_t t = k * (size_t)C + (size_t)c;
            TreePaths &tp = trees[t];
            size_t off = 0;
            tree_at.clear();
            for (const std::vector<uint32_t> &set : tp.sets) {
                const auto it = pool_at.emplace(set, (uint32_t)h_pool.size()).first;
                if (it->second == h_pool.size()) h_pool.insert(h_pool.end(), set.begin(), set.end());
                tree_at.push_back(it->second + 1u);
            }
            for (unsigned char len : tp.len) {
                if (fill + len > 64) flush();
                for (int j = 0; j < len; ++j) {
                    uint4 u = tp.elems[off + j];
                    u.w = (u.w & ~kElemRankLenMask) | (uint32_t)j << kElemRankShift | (uint32_t)(len - 1) << kElemLenShift;
                    h_elems.push_back(u);
                    h_om.push_back(tp.om[off + j]);
                    if (any_sets) {
                        const uint32_t local = off + j < tp.set_of.size() ? tp.set_of[off + j] : 0u;
                        h_set.push_back(local ? tree_at[local - 1u] : 0u);
                    }
                }
                fill += len;
                steps = std::max(steps, (int)len);
                off += len;
                ++n_paths;
                n_elems += len;
            }
            std::vector<uint4>().swap(tp.elems);
            std::vector<float>().swap(tp.om);
            std::vector<std::vector<uint32_t>>().swap(tp.sets);
        }
        flush();
    }
    h_class_bins[C] = (int)(h_elems.size() / 64);
}

// The path tables from the paths of every tree (caller's tree numbering): packing, bias and LDS shapes.
static tahoe_status build_tables(tahoe_forest *f, std::vector<TreePaths> &trees)
{
    const int F = f->p.num_cols;
    // LDS: the row tile and four slabs, R rows each; R is the largest power of two <= 64 that fits 80 KiB (two workgroups
    // per CU), else the whole LDS
    size_t R = 64;
    const size_t per_row = 5 * (size_t)F * sizeof(float);
    while (R > 1 && R * per_row > 80 * 1024) R /= 2;
    if (const tahoe_status s = check_contrib_cols(f)) return s;

    std::vector<float> h_bias, h_div;
    {
        std::vector<double> expect(trees.size());
        for (size_t t = 0; t < trees.size(); ++t) expect[t] = trees[t].expect;
        class_bias(f, expect, h_bias, h_div);
    }
    PathBins bins;
    pack_paths(trees, f->num_classes, (size_t)f->class_trees, bins);
    const std::vector<uint4> &h_elems = bins.elems;
    const std::vector<float> &h_om = bins.om;
    const std::vector<uint32_t> &h_info = bins.info, &h_set = bins.set, &h_pool = bins.pool;
    const std::vector<int> &h_class_bins = bins.class_bins;
    const bool any_sets = bins.any_sets;
    const size_t n_paths = bins.n_paths, n_elems = bins.n_elems;

    tahoe_cstate *cs = new (std::nothrow) tahoe_cstate();
    if (!cs) return fail(TAHOE_ERR_NO_MEMORY, "contribs_build");
    f->cs = cs;
    cs->bins = h_info.size();
    cs->paths = n_paths;
    cs->path_elems = n_elems;
    cs->rows_per_tile = (int)R;
    cs->lds_bytes = R * per_row;
    // interactions: four LDS slabs of F x F floats and the row per tile row where that fits 80 KiB, else in place in the output,
    // one row per wave (rows are then the only parallelism: a wave walks every bin of its row)
    const size_t inter_row = ((size_t)F + 4 * (size_t)F * F) * sizeof(float);
    cs->inter_slabs = inter_row <= (size_t)kInterSlabMaxBytes && inter_row <= (size_t)f->lds_limit;
    size_t RI = 1;
    if (cs->inter_slabs)
        for (RI = kInterMaxRows; RI > 1 && RI * inter_row > (size_t)kInterSlabMaxBytes;) RI /= 2;
    cs->inter_rows = (int)RI;
    cs->inter_lds_bytes = cs->inter_slabs ? RI * inter_row : kContribWaves * (size_t)F * sizeof(float);
    size_t *total = &f->device_bytes;
    hipError_t e;
    if ((e = upload(&cs->elems, h_elems, total)) != hipSuccess || (e = upload(&cs->one_minus_z, h_om, total)) != hipSuccess ||
        (e = upload(&cs->bin_info, h_info, total)) != hipSuccess || (e = upload(&cs->class_bins, h_class_bins, total)) != hipSuccess ||
        (e = upload(&cs->bias, h_bias, total)) != hipSuccess || (e = upload(&cs->class_div, h_div, total)) != hipSuccess)
        return fail(TAHOE_ERR_HIP, "contribs_build: upload failed: %s", hipGetErrorString(e));
    if (any_sets) {
        if (h_pool.size() >= 0xffffffffu) return fail(TAHOE_ERR_UNSUPPORTED, "contribs_build: %zu words of category sets (at most 2^32 - 2)", h_pool.size());
        cs->set_words = (uint32_t)h_pool.size();
        if ((e = upload(&cs->elem_set, h_set, total)) != hipSuccess || (e = upload(&cs->set_pool, h_pool, total)) != hipSuccess)
            return fail(TAHOE_ERR_HIP, "contribs_build: upload of the category sets failed: %s", hipGetErrorString(e));
    }
    if ((e = allow_max_lds(reinterpret_cast<const void *>(&contribs_kernel<false>), f->lds_limit)) != hipSuccess)
        return fail(TAHOE_ERR_HIP, "hipFuncSetAttribute(contribs) failed: %s", hipGetErrorString(e));
    if ((e = allow_max_lds(reinterpret_cast<const void *>(&contribs_spare_kernel<false>), f->lds_limit)) != hipSuccess ||
        (e = allow_max_lds(reinterpret_cast<const void *>(&interactions_kernel<true>), f->lds_limit)) != hipSuccess ||
        (e = allow_max_lds(reinterpret_cast<const void *>(&interactions_kernel<false>), f->lds_limit)) != hipSuccess)
        return fail(TAHOE_ERR_HIP, "hipFuncSetAttribute(interactions) failed: %s", hipGetErrorString(e));
    if (any_sets &&
        ((e = allow_max_lds(reinterpret_cast<const void *>(&contribs_kernel<true>), f->lds_limit)) != hipSuccess ||
         (e = allow_max_lds(reinterpret_cast<const void *>(&contribs_spare_kernel<true>), f->lds_limit)) != hipSuccess ||
         (e = allow_max_lds(reinterpret_cast<const void *>(&interactions_kernel<true, true>), f->lds_limit)) != hipSuccess ||
         (e = allow_max_lds(reinterpret_cast<const void *>(&interactions_kernel<false, true>), f->lds_limit)) != hipSuccess))
        return fail(TAHOE_ERR_HIP, "hipFuncSetAttribute(contribs, category sets) failed: %s", hipGetErrorString(e));
    return TAHOE_OK;
}

tahoe_status contribs_build(tahoe_forest *f, const tahoe_dense_node *nodes)
{
    const size_t T = (size_t)f->p.num_trees;
    const size_t per = (size_t)tahoe_tree_num_nodes(f->p.depth);
    std::vector<TreePaths> trees(T);  // in the caller's tree numbering
    parallel_for(T, 4, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; ++t) {
            tree_paths(DenseTree{nodes + t * per}, trees[t]);
            trees[t].expect = tree_expect(DenseTree{nodes + t * per});
        }
    });
    return build_tables(f, trees);
}

tahoe_status contribs_validate_sparse(const int32_t *trees, const tahoe_sparse_node *nodes, const float *covers,
                                      const tahoe_forest_params *p, bool path_limit, bool check_covers)
{
    // per reachable internal node, the covers of its two children; per reachable leaf, the distinct features of its path (the
    // element word's 5-bit rank and length fields, and interventional.hip's 32 x 32 weight table, hold at most 31)
    std::vector<int> count((size_t)std::max(p->num_cols, 1), 0);  // uses of each feature on the current path
    std::vector<int> path;                                        // features of the current path, root first
    struct Frame {
        int32_t node;
        int depth;
    };
    std::vector<Frame> stack;
    for (int t = 0; t < p->num_trees; ++t) {
        const tahoe_sparse_node *tn = nodes + trees[t];
        const float *tc = check_covers ? covers + trees[t] : nullptr;
        int distinct = 0;
        path.clear();
        stack.assign(1, Frame{0, 0});
        while (!stack.empty()) {
            const Frame fr = stack.back();
            stack.pop_back();
            while ((int)path.size() > fr.depth) {  // back up to this node's parent
                if (--count[(size_t)path.back()] == 0) --distinct;
                path.pop_back();
            }
            const tahoe_sparse_node &n = tn[fr.node];
            if (n.bits & (int32_t)(1u << 31)) {
                if (path_limit && distinct > 31)
                    return fail(TAHOE_ERR_UNSUPPORTED,
                                "tree %d: a leaf's path has %d distinct features (TAHOE_CREATE_CONTRIBS supports at most 31)", t,
                                distinct);
                continue;
            }
            const int fid = n.bits & 0x3fffffff;
            if (count[(size_t)fid]++ == 0) ++distinct;
            path.push_back(fid);
            const float wl = tc ? tc[n.left_idx] : 1.0f, wr = tc ? tc[n.left_idx + 1] : 1.0f;
            if (!std::isfinite(wl) || !std::isfinite(wr) || !(wl >= 0.0f) || !(wr >= 0.0f) || !((double)wl + (double)wr > 0.0))
                return fail(TAHOE_ERR_INVALID_FOREST,
                            "tree %d node %d: child covers %g and %g (TAHOE_CREATE_CONTRIBS needs finite covers >= 0 with a "
                            "positive sum at every reachable internal node)",
                            t, fr.node, (double)wl, (double)wr);
            stack.push_back(Frame{n.left_idx + 1, fr.depth + 1});
            stack.push_back(Frame{n.left_idx, fr.depth + 1});
        }
        for (int fid : path) count[(size_t)fid] = 0;
    }
    return TAHOE_OK;
}

tahoe_status contribs_build_sparse(tahoe_forest *f, const int32_t *tree_roots, const tahoe_sparse_node *nodes, const float *covers,
                                   const tahoe_categorical_splits *cats)
{
    const size_t T = (size_t)f->p.num_trees;
    std::vector<TreePaths> trees(T);  // in the caller's tree numbering
    parallel_for(T, 4, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; ++t) {
            tree_paths(SparseTree{nodes + tree_roots[t], covers + tree_roots[t], cats, tree_roots[t]}, trees[t], cats);
            trees[t].expect = tree_expect(SparseTree{nodes + tree_roots[t], covers + tree_roots[t]});
        }
    });
    return build_tables(f, trees);
}

void contribs_bias_vector(const tahoe_forest *f, const int32_t *tree_roots, const tahoe_sparse_node *nodes, const float *leaf_values,
                          const float *covers, std::vector<float> &bias, std::vector<float> &div)
{
    const size_t T = (size_t)f->p.num_trees, K = (size_t)f->num_classes;
    std::vector<double> expect(T * K);  // [tree][k]: what class_bias reads on the expansion's tree t * K + k
    parallel_for(T, 4, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; ++t) {
            const SparseTree tree{nodes + tree_roots[t], covers + tree_roots[t]};
            for (size_t k = 0; k < K; ++k) expect[t * K + k] = tree_expect(VectorTreeK{tree, leaf_values, K, k});
        }
    });
    class_bias(f, expect, bias, div);
}

tahoe_status contribs_tables_vector(const tahoe_forest *f, const int32_t *tree_roots, const tahoe_sparse_node *nodes,
                                    const float *leaf_values, const float *covers, VectorPathTables &out)
{
    if (const tahoe_status s = check_contrib_cols(f)) return s;
    const size_t T = (size_t)f->p.num_trees;
    std::vector<TreePaths> trees(T);
    parallel_for(T, 4, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; ++t) {
            if (!covers) {
                tree_paths(VectorTreeUnit{VectorTree{SparseTree{nodes + tree_roots[t], nullptr}}}, trees[t]);
                continue;
            }
            tree_paths(VectorTree{SparseTree{nodes + tree_roots[t], covers + tree_roots[t]}}, trees[t]);
        }
    });
    if (covers) contribs_bias_vector(f, tree_roots, nodes, leaf_values, covers, out.bias, out.div);
    PathBins bins;
    pack_paths(trees, 1, T, bins);  // one set of bins: what the sparse handle builds for one class of the expansion
    out.elems.swap(bins.elems);
    if (covers) out.one_minus_z.swap(bins.om);
    out.bin_info.swap(bins.info);
    out.paths = bins.n_paths;
    out.path_elems = bins.n_elems;
    return TAHOE_OK;
}

void contribs_destroy(tahoe_forest *f)
{
    tahoe_cstate *cs = f->cs;
    if (!cs) return;
    if (cs->elems) (void)hipFree(cs->elems);
    if (cs->one_minus_z) (void)hipFree(cs->one_minus_z);
    if (cs->bin_info) (void)hipFree(cs->bin_info);
    if (cs->class_bins) (void)hipFree(cs->class_bins);
    if (cs->bias) (void)hipFree(cs->bias);
    if (cs->class_div) (void)hipFree(cs->class_div);
    if (cs->elem_set) (void)hipFree(cs->elem_set);
    if (cs->set_pool) (void)hipFree(cs->set_pool);
    delete cs;
    f->cs = nullptr;
}

}  // namespace tahoe

using namespace tahoe;

extern "C" tahoe_status tahoe_forest_predict_contribs(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows,
                                                      void *stream)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_contribs: null forest");
    if (oblivious_serves(f, TAHOE_CREATE_CONTRIBS))
        return oblivious_predict_shap(f, TAHOE_CREATE_CONTRIBS, phi_dev, data_dev, rows, (hipStream_t)stream,
                                      "tahoe_forest_predict_contribs");
    if (vector_serves_contribs(f))
        return vector_predict_contribs(f, phi_dev, data_dev, rows, (hipStream_t)stream, "tahoe_forest_predict_contribs");
    if (tahoe_status st = need_path_tables(f, "tahoe_forest_predict_contribs")) return st;
    if (rows == 0) return TAHOE_OK;
    if (!phi_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_contribs: null argument");
    if (tahoe_status st = check_shap_out(f, rows, 1, "tahoe_forest_predict_contribs")) return st;
    const tahoe_cstate *cs = f->cs;
    DeviceGuard on_device(f->device);
    const size_t R = (size_t)cs->rows_per_tile;
    const size_t grid = (rows + R - 1) / R;
    auto launch = [&](auto sets) {
        hipLaunchKernelGGL(contribs_kernel<decltype(sets)::value>, dim3((unsigned)grid), dim3(256), cs->lds_bytes, (hipStream_t)stream,
                           phi_dev, data_dev, rows, f->p.num_cols, f->num_classes, (int)R, cs->elems, cs->one_minus_z, cs->bin_info,
                           cs->class_bins, cs->bias, cs->class_div, f->p.missing, cs->elem_set, cs->set_pool, cs->set_words);
    };
    if (cs->elem_set) launch(std::true_type{});
    else launch(std::false_type{});
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}


extern "C" tahoe_status tahoe_forest_predict_interactions(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows,
                                                          void *stream)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_interactions: null forest");
    if (oblivious_serves(f, TAHOE_CREATE_INTERACTIONS))
        return oblivious_predict_interactions(f, out_dev, data_dev, rows, (hipStream_t)stream, "tahoe_forest_predict_interactions");
    if (vector_serves_interactions(f))
        return vector_predict_interactions(f, out_dev, data_dev, rows, (hipStream_t)stream, "tahoe_forest_predict_interactions");
    if (tahoe_status st = need_path_tables(f, "tahoe_forest_predict_interactions")) return st;
    if (rows == 0) return TAHOE_OK;
    if (!out_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_interactions: null argument");
    if (tahoe_status st = check_shap_out(f, rows, 2, "tahoe_forest_predict_interactions")) return st;
    const int F = f->p.num_cols, C = f->num_classes;
    const tahoe_cstate *cs = f->cs;
    DeviceGuard on_device(f->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t R = (size_t)cs->rows_per_tile;
    auto spare = [&](auto sets) {
        hipLaunchKernelGGL(contribs_spare_kernel<decltype(sets)::value>, dim3((unsigned)((rows + R - 1) / R)), dim3(256), cs->lds_bytes,
                           s, out_dev, data_dev, rows, F, C, (int)R, cs->elems, cs->one_minus_z, cs->bin_info, cs->class_bins, cs->bias,
                           cs->class_div, f->p.missing, cs->elem_set, cs->set_pool, cs->set_words);
    };
    if (cs->elem_set) spare(std::true_type{});
    else spare(std::false_type{});
    TAHOE_HIP_TRY(hipGetLastError());
    const size_t RI = (size_t)cs->inter_rows, per_block = cs->inter_slabs ? RI : RI * kContribWaves;
    const dim3 grid((unsigned)((rows + per_block - 1) / per_block));
    auto inter = [&](auto slabs, auto sets) {
        hipLaunchKernelGGL((interactions_kernel<decltype(slabs)::value, decltype(sets)::value>), grid, dim3(256), cs->inter_lds_bytes,
                           s, out_dev, data_dev, rows, F, C, (int)RI, cs->elems, cs->one_minus_z, cs->bin_info, cs->class_bins, cs->bias,
                           cs->class_div, f->p.missing, cs->elem_set, cs->set_pool, cs->set_words);
    };
    if (cs->inter_slabs) {
        if (cs->elem_set) inter(std::true_type{}, std::true_type{});
        else inter(std::true_type{}, std::false_type{});
    } else if (cs->elem_set) {
        inter(std::false_type{}, std::true_type{});
    } else {
        inter(std::false_type{}, std::false_type{});
    }
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}
