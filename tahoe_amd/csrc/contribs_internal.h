// The TreeSHAP path tables of a handle created with TAHOE_CREATE_CONTRIBS, shared by the translation units that read them
// (contribs.hip builds them and runs the path-dependent kernels, interventional.hip the interventional ones).  Internal: not
// part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

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
    // Category sets (TAHOE_CREATE_CAT_CONTRIBS; null / 0 on a handle whose paths cross no categorical split): set_pool holds,
    // per distinct set, a header outside_ok << 31 | nwords and its nwords bitset words (the split pool's layout); elem_set
    // [bins][64] names an element's header as offset + 1, 0 = the element has no set
    uint32_t *elem_set = nullptr;
    uint32_t *set_pool = nullptr;
    uint32_t set_words = 0;         // words of set_pool: bounds every word read
};

// The background of interventional TreeSHAP (tahoe_forest_set_background): interventional.hip builds it, its kernels and
// vector_iv.hip's read it
struct tahoe_istate {
    unsigned long long *masks = nullptr;  // [bins][B] ballot of the lanes whose element background row r follows (rank-0 lanes 0)
    float *consts = nullptr;              // [kIvTable] weight table, then [num_classes] the bias column
    size_t bg_rows = 0;
    size_t bytes = 0;                     // device bytes of the two buffers (counted in tahoe_forest::device_bytes)
};

namespace tahoe {

// W[p * 32 + q] = (p - 1)! q! / (p + q)! = 1 / (p C(p + q, q)) for p >= 1, p + q <= 31 (a path has at most 31 features), from
// float64 rounded once; 0 elsewhere.  A lane of A reads W[a][b], a lane of B W[b][a] (and subtracts).
constexpr int kIvTable = 32 * 32;
constexpr int kIvMaxTileRows = 8;               // rows of a workgroup's tile: small, so that a batch spreads over the CUs
constexpr size_t kIvLdsBudget = 80 * 1024;      // two workgroups per CU where the tile allows it, as contribs_kernel
constexpr int kIvUnroll = 8;                    // background rows whose mask and weight loads are issued together

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

// A lane's view of its element's category set: the pool index of its first word (0: no set), its header and its first word.
// An element without a set reads as "no member anywhere, everything outside allowed", which follows_set() passes.
struct ElemSet {
    uint32_t at, head, word0;
};
constexpr uint32_t kSetOutsideOk = 0x80000000u, kSetWordsMask = 0xfffffu;

// The set of lane `idx` of the bins (loop-invariant: once per bin, outside the row loop)
__device__ __forceinline__ ElemSet elem_set_load(const uint32_t *__restrict__ elem_set, const uint32_t *__restrict__ pool,
                                                 uint32_t pool_words, size_t idx)
{
    ElemSet s{elem_set[idx], kSetOutsideOk, 0u};
    if (s.at != 0u) {
        s.head = pool[s.at - 1u];
        s.word0 = ((s.head & kSetWordsMask) != 0u && s.at < pool_words) ? pool[s.at] : 0u;
    }
    return s;
}
// Does some lane of the wave hold a set of more than one word?  (Else no lane gathers: every lane holds its whole set.)
__device__ __forceinline__ bool elem_sets_gather(const ElemSet &s) { return __ballot((s.head & kSetWordsMask) > 1u) != 0ull; }

// one-fraction of an element that may carry a category set: follows() on the interval, and, for a non-missing x, bit trunc(x)
// of the set where go_right_cat's range test holds (0 <= x < 2^24 and trunc(x) < 32 nwords), else outside_ok.  gather
// (wave-uniform, elem_sets_gather): read the word trunc(x) selects from the pool, bounded by pool_words; without it the lane's
// held word serves (nwords <= 1).
__device__ __forceinline__ bool follows_set(float x, float lower, float upper, bool missing_ok, bool nan_ok, float missing,
                                            const ElemSet &s, const uint32_t *__restrict__ pool, uint32_t pool_words, bool gather)
{
    const bool is_missing = fabsf(x - missing) <= kMissingEps;
    const bool in = x >= 0.0f && x < 16777216.0f;
    const uint32_t c = in ? (uint32_t)x : 0u;
    const bool in_range = in && (c >> 5) < (s.head & kSetWordsMask);
    uint32_t word = s.word0;
    if (gather) {
        const uint32_t wi = s.at + (c >> 5);
        word = (in_range && wi < pool_words) ? pool[wi] : 0u;
    }
    const bool set_ok = in_range ? ((word >> (c & 31u)) & 1u) != 0u : (s.head & kSetOutsideOk) != 0u;
    const bool num_ok = x != x ? nan_ok : (x >= lower && !(x >= upper));
    return is_missing ? missing_ok : (num_ok && set_ok);
}

// 1 / k for k = 0 .. 33 (entry 0 unused), correctly rounded by constant folding: the uniform factors of the recursions
// (treeshap_lanes.h defines the __constant__ table of a unit from this list).
#define TAHOE_CONTRIB_INV_TABLE                                                                                                   \
    {0.0f,         1.0f,         1.0f / 2.0f,  1.0f / 3.0f,  1.0f / 4.0f,  1.0f / 5.0f,  1.0f / 6.0f,  1.0f / 7.0f,  1.0f / 8.0f,    \
     1.0f / 9.0f,  1.0f / 10.0f, 1.0f / 11.0f, 1.0f / 12.0f, 1.0f / 13.0f, 1.0f / 14.0f, 1.0f / 15.0f, 1.0f / 16.0f, 1.0f / 17.0f,   \
     1.0f / 18.0f, 1.0f / 19.0f, 1.0f / 20.0f, 1.0f / 21.0f, 1.0f / 22.0f, 1.0f / 23.0f, 1.0f / 24.0f, 1.0f / 25.0f, 1.0f / 26.0f,   \
     1.0f / 27.0f, 1.0f / 28.0f, 1.0f / 29.0f, 1.0f / 30.0f, 1.0f / 31.0f, 1.0f / 32.0f, 1.0f / 33.0f}

// The path tables of a vector-leaf handle (tahoe_vector_forest_create_ex with TAHOE_CREATE_CONTRIBS), on the host: one set of
// bins for the forest -- the bins tahoe_sparse_forest_create_ex builds for one class of the K-fold expansion -- whose root
// elements carry in .x the index of the leaf's vector instead of a leaf value; bias[k] and div[k] as class_bias computes them on
// the expansion.  contribs.hip builds them (tree_paths, pack_paths), vector_shap.hip uploads and reads them.  The forest has
// passed contribs_validate_sparse; f->p, num_classes = K and class_trees = num_trees are set.  TAHOE_ERR_UNSUPPORTED when
// num_cols is past the limit of 20 B of LDS per column.  covers == nullptr (TAHOE_CREATE_INTERVENTIONAL alone): the bins are built
// as if every cover were 1 -- features, bounds, flags, lengths, packing, ranks and rounds do not depend on the covers; an
// element's .z is then not to be read -- and one_minus_z, bias and div stay empty.
struct VectorPathTables {
    std::vector<uint4> elems;
    std::vector<float> one_minus_z;
    std::vector<uint32_t> bin_info;
    std::vector<float> bias, div;
    size_t paths = 0, path_elems = 0;
};
tahoe_status contribs_tables_vector(const tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes,
                                    const float *leaf_values, const float *covers, VectorPathTables &out);

}  // namespace tahoe
