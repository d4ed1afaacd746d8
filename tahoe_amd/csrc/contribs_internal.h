// The TreeSHAP path tables of a handle created with TAHOE_CREATE_CONTRIBS, shared by the translation units that read them
// (contribs.hip builds them and runs the path-dependent kernels, interventional.hip the interventional ones).  Internal: not
// part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

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
// = 1) and carries the leaf value in .x.  Padding lanes are rank-0 paths of length 1.
constexpr int kContribWaves = 4;      // waves per workgroup; bin b of a class goes to wave (b - first bin of the class) % 4
constexpr int kContribMaxCols = 32767;
constexpr uint32_t kElemFidMask = 0x7fffu;
// Smallest nonzero zero fraction a path element stores: 32 x 2^-126, so that z / (ud + 1) >= 2^-126 (normal) for ud <= 31
constexpr double kContribMinZ = 0x1p-121;

}  // namespace tahoe
