// The TreeSHAP path tables of a handle created with TAHOE_CREATE_CONTRIBS, shared by the translation units that read them
// (contribs.hip builds them and runs the path-dependent kernels, interventional.hip the interventional ones).  Internal: not
// part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "forest_internal.h"

struct tahoe_cstate {
    uint4 *elems = nullptr;         // [bins][64] path elements, class-major (bin ranges class_bins[c] .. class_bins[c + 1])
    float *one_minus_z = nullptr;   // [bins][64] 1 - zero fraction, from float64 (1 - (float)z loses it when z is near 1)
    uint32_t *bin_info = nullptr;   // [bins] longest path of the bin (elements, root included) | rounds of ordered adds << 8
    int *class_bins = nullptr;      // [num_classes + 1]
    float *bias = nullptr;          // [num_classes] the bias column, float64 on the host, rounded once
    float *class_div = nullptr;     // [num_classes] (float)Tc with TAHOE_OUT_AVG, else 1.0f
    size_t bins = 0;
    size_t paths = 0;
    size_t path_elems = 0;          // elements of all paths, root elements included
    int rows_per_tile = 0;          // rows of a workgroup's LDS tile (fixed per handle)
    size_t lds_bytes = 0;
    // tahoe_forest_predict_interactions: the form (LDS slabs or in place), its rows per workgroup (slabs) or per wave (in
    // place), and its LDS bytes per workgroup; fixed per handle by num_cols
    bool inter_slabs = false;
    int inter_rows = 0;
    size_t inter_lds_bytes = 0;
};

namespace tahoe {

// Element word (.w): fid (15 bits) | rank in its path << 15 | (path length - 1) << 20 | round << 25 | missing_ok << 30 |
// nan_ok << 31.  .x / .y / .z: the lower bound (x >= lower for every right edge), the upper bound (!(x >= upper) for every left
// edge; NaN = none), the zero fraction (product of the edges' cover ratios).  A path's rank-0 lane is its root element (z = o
// = 1) and carries the leaf value in .x.  Padding lanes are rank-0 paths of length 1.  Round: the earlier lanes of the bin on the
// same feature (their terms add first).
constexpr int kContribWaves = 4;      // waves per workgroup; bin b of a class goes to wave (b - first bin of the class) % 4
constexpr int kContribMaxCols = 32767;
constexpr uint32_t kElemFidMask = 0x7fffu;
constexpr int kElemRankShift = 15, kElemLenShift = 20, kElemRoundShift = 25;  // 5-bit fields
constexpr uint32_t kElemFieldMask = 31u;
constexpr uint32_t kElemRankLenMask = 0x3ffu << kElemRankShift;  // rank and length - 1 together
// Smallest nonzero zero fraction a path element stores: 32 x 2^-126, so that z / (ud + 1) >= 2^-126 (normal) for ud <= 31
constexpr double kContribMinZ = 0x1p-121;

// The element word of a path's element, for rank < 32, 1 <= len <= 32, round < 32
inline uint32_t elem_word(int fid, int rank, int len, int round, bool missing_ok, bool nan_ok)
{
    return (uint32_t)fid | (uint32_t)rank << kElemRankShift | (uint32_t)(len - 1) << kElemLenShift |
           (uint32_t)round << kElemRoundShift | (missing_ok ? 1u << 30 : 0u) | (nan_ok ? 1u << 31 : 0u);
}
__host__ __device__ __forceinline__ int elem_fid(uint32_t w) { return (int)(w & kElemFidMask); }
__host__ __device__ __forceinline__ int elem_rank(uint32_t w) { return (int)((w >> kElemRankShift) & kElemFieldMask); }
__host__ __device__ __forceinline__ int elem_ud(uint32_t w) { return (int)((w >> kElemLenShift) & kElemFieldMask); }  // length - 1
__host__ __device__ __forceinline__ int elem_round(uint32_t w) { return (int)((w >> kElemRoundShift) & kElemFieldMask); }
__host__ __device__ __forceinline__ bool elem_missing_ok(uint32_t w) { return (w >> 30) & 1u; }
__host__ __device__ __forceinline__ bool elem_nan_ok(uint32_t w) { return (w >> 31) != 0; }

// one-fraction: does x follow every edge of the element's feature on its path?  (go_right's rule, folded over the edges; the
// arguments are the element's fields)
__device__ __forceinline__ bool follows(float x, float lower, float upper, bool missing_ok, bool nan_ok, float missing)
{
    const bool is_missing = fabsf(x - missing) <= kMissingEps;
    return is_missing ? missing_ok : (x != x ? nan_ok : (x >= lower && !(x >= upper)));
}

// v of lane src_lane (ds_bpermute)
__device__ __forceinline__ float lane_read(float v, int src_lane)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}
__device__ __forceinline__ uint32_t lane_read_u(uint32_t v, int src_lane)
{
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}

}  // namespace tahoe
