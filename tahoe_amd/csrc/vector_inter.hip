// SHAP interaction values on a vector-leaf handle (tahoe_vector_forest_create_ex with TAHOE_CREATE_CONTRIBS |
// TAHOE_CREATE_VECTOR_INTERACTIONS).  As in vector_shap.hip the K outputs of a leaf share its path, and in
// the term of interaction_bins (contribs.hip), total * (o ? om : -z) * leaf * ((ok ? om_k : -z_k) * 0.5f) = (tw * leaf) * h, only
// the leaf value depends on the output.  So the pair rounds, the extend recursion over the path without the conditioning element
// and the unwound sum run once per (row, bin, conditioning element) for a block of KB classes, where interactions_kernel on the
// T x K-tree expansion runs them once per class.  phi comes from vector_contribs_spare_kernel (vector_shap.hip), which writes it
// into row F of every matrix first.
//
// Bits: out[row][k] is what interactions_kernel gives for class k of the expansion.  The form is chosen as there, by F alone.
// Slabs: bin b goes to wave b % 4, the terms of a pair add in the row-independent round order of the bin, the four partial sums
// combine as ((s0 + s1) + s2) + s3 and are divided by div.  In place: every bin in order, straight into the output, then / div.
// Both: diagonal = phi_i - (off-diagonal sum of row i, ascending from 0.0f).  The pair rounds and the conditioned unwound sum are
// interaction_bins' statements (contribs.hip), kept in step by hand: treeshap_lanes.h says why they are not one function.
// Neither KB, the rows of a tile nor the placement of the class blocks takes part in any sum.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "forest_internal.h"
#include "contribs_internal.h"
#include "treeshap_lanes.h"
#include "vector_internal.h"

namespace tahoe {

constexpr size_t kVecInterLdsBudget = 80 * 1024;  // interactions_kernel's: two workgroups per CU
constexpr int kVecInterMaxRows = 32;              // rows of a tile: one bit each in the per-lane one-fraction mask

// Both entries of a pair receive the same adds in the same order, so the slab form keeps each unordered pair once: the strict
// upper triangle of an F x F matrix, row-major.  (a, b) with a < b < F -> [0, F (F - 1) / 2)
__host__ __device__ __forceinline__ int tri_index(int a, int b, int F) { return a * (2 * F - a - 1) / 2 + (b - a - 1); }

// The off-diagonal terms of bins b_first, b_first + b_step, ... < b_end for the nr rows of `tile` (row r at tile + r F) and the nk
// classes k0 .. k0 + nk - 1.  SLABS: the pair {a, b} of row r, class j adds into acc[j acc_class + r acc_row + tri_index(a, b)].
// In place: into acc[j acc_class + r acc_row + a ld + b] and its mirror, each round followed by a drain of the wave's stores.
template <int KB, bool SLABS>
__device__ __forceinline__ void vector_interaction_bins(float *acc, size_t acc_row, size_t acc_class, int ld, const float *tile, int nr,
                                                        int F, int K, int k0, int nk, int b_first, int b_end, int b_step,
                                                        const uint4 *__restrict__ elems, const float *__restrict__ one_minus_z,
                                                        const uint32_t *__restrict__ bin_info, const float *__restrict__ leaves,
                                                        float missing)
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
        float leaf[KB];  // the block's leaf values
        load_leaf_block<KB>(leaf, leaves, e.x, K, k0, nk, rank, gs);
        // one-fractions of this lane's element, bit r for row r (a root lane's bounds are not bounds: its bit is never read)
        uint32_t omask = 0;
        for (int r = 0; r < nr; ++r) omask |= (follows(tile[r * F + fid], lower, upper, missing_ok, nan_ok, missing) ? 1u : 0u) << r;
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
            // where this lane's pair lives (a pair's two features differ: a path's elements are distinct features)
            const size_t at = !pair ? 0 : SLABS ? (size_t)tri_index(min(fid, fk), max(fid, fk), F) : (size_t)fk * ld + fid;
            const size_t at_t = pair ? (size_t)fid * ld + fk : 0;  // the mirrored entry (in place)
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
                // what the block's classes share; class j's term is tw * leaf[j] * h, left to right
                const float tw = total * (o ? om : -z);
                const float h = (ok ? om_k : -z_k) * 0.5f;
                float *pa = acc + r * acc_row + at, *pb = acc + r * acc_row + at_t;
                for (int q = 0; q < rounds; ++q) {
                    if (pair && round == q) {
                        if (SLABS) {
                            add_leaf_block<KB>(pa, acc_class, nk, [&](int j) { return tw * leaf[j] * h; });
                        } else {
                            float va[KB], vb[KB];
#pragma unroll
                            for (int j = 0; j < KB; ++j)
                                if (j < nk) {
                                    va[j] = pa[j * acc_class];
                                    vb[j] = pb[j * acc_class];
                                }
#pragma unroll
                            for (int j = 0; j < KB; ++j)
                                if (j < nk) {
                                    const float term = tw * leaf[j] * h;
                                    pa[j * acc_class] = va[j] + term;
                                    pb[j * acc_class] = vb[j] + term;
                                }
                        }
                    }
                    if (!SLABS) vm_drain();  // one drain covers the read-modify-writes of the block's matrices
                }
            }
        }
    }
}

// SLABS: one workgroup = a tile of R <= 32 rows x all bins x the class blocks k0 = blockIdx.y KB, + gridDim.y KB, ...; wave w
// evaluates bins w, w + 4, ... into its own KB triangles per row.  LDS: tile [R][F] | tri [4][KB][R][F (F - 1) / 2].
// In place (R = 1): wave w of a workgroup owns row 4 blockIdx.x + w and the KB matrices of a class block in the output; the
// zeroing, divisor, diagonal and row-F passes per class are those of interactions_kernel<false>.  LDS: tile [4][F].
template <int KB, bool SLABS>
__global__ __launch_bounds__(256) void vector_interactions_kernel(float *out, const float *__restrict__ data, size_t rows, int F, int K,
                                                                  int R, const uint4 *__restrict__ elems,
                                                                  const float *__restrict__ one_minus_z,
                                                                  const uint32_t *__restrict__ bin_info, int bins,
                                                                  const float *__restrict__ leaves, const float *__restrict__ bias,
                                                                  float div, float missing)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F1 = F + 1;
    const size_t mat = (size_t)F1 * F1;
    const size_t tile_rows = SLABS ? (size_t)R : (size_t)kContribWaves;
    const size_t row0 = (size_t)blockIdx.x * tile_rows;
    const int nt = (int)min(tile_rows, rows - row0);
    float *tile = smem;
    const float *src = data + row0 * F;
    for (int i = tid; i < nt * F; i += 256) tile[i] = src[i];
    __syncthreads();

    if (SLABS) {
        const int P = F * (F - 1) / 2;  // pairs of a row
        const size_t RP = (size_t)R * P;
        float *tri = smem + (size_t)R * F;
        float *mine = tri + (size_t)wave * KB * RP;  // this wave's triangles: class j of the block, row r at mine + j RP + r P
        for (int k0 = (int)blockIdx.y * KB; k0 < K; k0 += (int)gridDim.y * KB) {
            const int nk = min(KB, K - k0);  // classes of this block
#pragma unroll
            for (int j = 0; j < KB; ++j)
                if (j < nk)
                    for (int i = lane; i < nt * P; i += 64) mine[j * RP + i] = 0.0f;
            __syncthreads();
            vector_interaction_bins<KB, true>(mine, (size_t)P, RP, 0, tile, nt, F, K, k0, nk, wave, bins, kContribWaves, elems,
                                              one_minus_z, bin_info, leaves, missing);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                if (j >= nk) continue;
                float *s0 = tri + j * RP;
                const float *s1 = s0 + KB * RP, *s2 = s1 + KB * RP, *s3 = s2 + KB * RP;
                for (int i = tid; i < nt * P; i += 256) s0[i] = (((s0[i] + s1[i]) + s2[i]) + s3[i]) / div;
            }
            __syncthreads();
            // diagonal: phi_i (row F of the output) - the row's off-diagonal sum in ascending j, straight into the output
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                if (j >= nk) continue;
                const float *s0 = tri + j * RP;
                for (int t = tid; t < nt * F; t += 256) {
                    const int r = t / F, i = t - r * F;
                    const float *m = s0 + (size_t)r * P;
                    float sum = 0.0f;
                    for (int c = 0; c < F; ++c)
                        if (c != i) sum += m[tri_index(min(i, c), max(i, c), F)];
                    float *M = out + ((row0 + r) * K + (size_t)(k0 + j)) * mat;
                    M[(size_t)i * F1 + i] = M[(size_t)F * F1 + i] - sum;
                }
            }
            __syncthreads();
            // the rest of the matrix: the triangle mirrored, row and column F zero but the bias corner
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                if (j >= nk) continue;
                const float *s0 = tri + j * RP;
                const float bj = bias[k0 + j];
                for (int r = 0; r < nt; ++r) {
                    float *M = out + ((row0 + r) * K + (size_t)(k0 + j)) * mat;
                    const float *m = s0 + (size_t)r * P;
                    for (int p = tid; p < F1 * F1; p += 256) {
                        const int a = p / F1, b = p - a * F1;
                        if (a < F && b < F) {
                            if (a != b) M[p] = m[tri_index(min(a, b), max(a, b), F)];
                        } else {
                            M[p] = (a == F && b == F) ? bj : 0.0f;
                        }
                    }
                }
            }
            __syncthreads();
        }
    } else {
        const int nr = wave < nt ? 1 : 0;
        const float *wtile = tile + (size_t)wave * F;
        for (int k0 = (int)blockIdx.y * KB; k0 < K; k0 += (int)gridDim.y * KB) {
            const int nk = min(KB, K - k0);
            if (nr == 0) break;  // a wave past the last row
            float *acc = out + ((row0 + wave) * K + (size_t)k0) * mat;
            for (int j = 0; j < nk; ++j)
                for (size_t i = lane; i < (size_t)F * F1; i += 64) acc[j * mat + i] = 0.0f;
            vm_drain();
            vector_interaction_bins<KB, false>(acc, 0, mat, F1, wtile, nr, F, K, k0, nk, 0, bins, 1, elems, one_minus_z, bin_info,
                                               leaves, missing);
            for (int j = 0; j < nk; ++j) {
                float *m = acc + j * mat;
                if (div != 1.0f) {  // x / 1.0f is x: skipping the pass changes no bit
                    for (size_t i = lane; i < (size_t)F * F1; i += 64) m[i] = m[i] / div;
                    vm_drain();
                }
                for (int i = lane; i < F; i += 64) {
                    const float *mi = m + (size_t)i * F1;
                    float sum = 0.0f;
                    for (int c = 0; c < F; ++c)
                        if (c != i) sum += mi[c];
                    m[(size_t)i * F1 + i] = m[(size_t)F * F1 + i] - sum;
                    m[(size_t)i * F1 + F] = 0.0f;
                }
                vm_drain();
                for (int i = lane; i < F; i += 64) m[(size_t)F * F1 + i] = 0.0f;
            }
        }
    }
}

// kernel(kb, slabs) for the runtime class block and form
template <class Fn>
static inline void with_inter_shape(int kb, bool slabs, Fn &&fn)
{
    with_class_block(kb, [&](auto c) {
        if (slabs) fn(c, std::true_type{});
        else fn(c, std::false_type{});
    });
}

// LDS bytes of one row of the slab form with class block kb
static size_t slab_row_bytes(int F, int kb)
{
    const size_t P = (size_t)F * (size_t)(F > 0 ? F - 1 : 0) / 2;
    return ((size_t)F + 4 * (size_t)kb * P) * sizeof(float);
}

tahoe_status vector_inter_build(const tahoe_forest *f, VectorShap *sh)
{
    const int F = f->p.num_cols, K = f->num_classes;
    // the form is the sparse handle's (build_tables, contribs.hip), by F alone: it enters the bits
    const size_t inter_row = ((size_t)F + 4 * (size_t)F * F) * sizeof(float);
    sh->inter_slabs = inter_row <= kVecInterLdsBudget && inter_row <= (size_t)f->lds_limit;
    const size_t budget = std::min(kVecInterLdsBudget, (size_t)f->lds_limit);
    // The class block: the largest of 8, 4, 2 -- not above K rounded up to one of them -- of which one row fits the budget (in
    // place: no LDS per class, so the largest), else 1; TAHOE_VECTOR_SHAP_KB forces one that leaves a row.  Then the rows of a
    // slab tile: the largest power of two <= 32 that fits.  Neither changes a bit of the result.
    const int kb = pick_class_block(f->knobs.vector_shap_kb, K,
                                    [&](int c, bool) { return !sh->inter_slabs || slab_row_bytes(F, c) <= budget; });
    sh->inter_class_block = kb;
    size_t R = 1;
    if (sh->inter_slabs)
        for (R = kVecInterMaxRows; R > 1 && R * slab_row_bytes(F, kb) > budget;) R /= 2;
    sh->inter_rows = (int)R;
    sh->inter_lds_bytes = sh->inter_slabs ? R * slab_row_bytes(F, kb) : kContribWaves * (size_t)F * sizeof(float);
    hipError_t e = hipSuccess;
    with_inter_shape(kb, sh->inter_slabs, [&](auto c, auto slabs) {
        e = allow_max_lds(reinterpret_cast<const void *>(&vector_interactions_kernel<decltype(c)::value, decltype(slabs)::value>),
                          f->lds_limit);
    });
    return hip_status(e, "hipFuncSetAttribute(vector_interactions)");
}

bool vector_serves_interactions(const tahoe_forest *f) { return f->vl && f->vl->shap && f->vl->shap->interactions; }

tahoe_status vector_predict_interactions(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows, hipStream_t stream,
                                         const char *fn)
{
    if (rows == 0) return TAHOE_OK;
    if (!out_dev || !data_dev) return fail(TAHOE_ERR_INVALID_ARG, "%s: null argument", fn);
    if (tahoe_status st = check_shap_out(f, rows, 2, fn)) return st;
    const VectorShap *sh = f->vl->shap;
    DeviceGuard on_device(f->device);
    if (tahoe_status st = vector_launch_contribs_spare(f, out_dev, data_dev, rows, stream)) return st;
    const int K = f->num_classes, kb = sh->inter_class_block;
    const size_t per_block = sh->inter_slabs ? (size_t)sh->inter_rows : (size_t)kContribWaves;
    const dim3 grid((unsigned)((rows + per_block - 1) / per_block), sh->grid_blocks ? (unsigned)((K + kb - 1) / kb) : 1u);
    with_inter_shape(kb, sh->inter_slabs, [&](auto c, auto slabs) {
        hipLaunchKernelGGL((vector_interactions_kernel<decltype(c)::value, decltype(slabs)::value>), grid, dim3(256),
                           sh->inter_lds_bytes, stream, out_dev, data_dev, rows, f->p.num_cols, K, sh->inter_rows, sh->elems,
                           sh->one_minus_z, sh->bin_info, sh->bins, f->vl->leaves, sh->bias, sh->div, f->p.missing);
    });
    TAHOE_HIP_TRY(hipGetLastError());
    return TAHOE_OK;
}

}  // namespace tahoe
