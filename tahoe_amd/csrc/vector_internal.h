// The device state of a vector-leaf handle (tahoe_vector_forest_create), shared by vector.hip (create, the walk kernels),
// vector_shap.hip (TreeSHAP on such a handle), vector_iv.hip (interventional TreeSHAP), vector_inter.hip (interaction values) and
// vector_approx.hip (Saabas contributions).
// Internal: not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "forest_internal.h"

namespace tahoe {

struct VNode {
    float val;         // threshold (leaf: unused)
    uint32_t bits;     // fid[0:29] | def_left << 30 | is_leaf << 31
    uint32_t left_idx; // children left_idx, left_idx + 1 relative to the root; leaf: index of the leaf's vector
    uint32_t pad;
};
static_assert(sizeof(VNode) == 16, "VNode must be 16 bytes");
constexpr uint32_t kVFidMask = (1u << 30) - 1u;
constexpr uint32_t kVDefLeft = 1u << 30;
constexpr uint32_t kVIsLeaf = 1u << 31;

// The TreeSHAP path tables of a handle created with TAHOE_CREATE_CONTRIBS and / or TAHOE_CREATE_INTERVENTIONAL (DESIGN.md
// sections 26 and 27): one set of bins for the forest, laid out as tahoe_cstate's, except that a path's root element carries the
// index of the leaf's vector in .x.  They are kept off tahoe_forest::cs on purpose: the kernels that read tahoe_cstate take .x of
// a root element for a leaf value.  Without TAHOE_CREATE_CONTRIBS the bins are built from unit covers: .z is not to be read.
struct VectorShap {
    bool contribs = false;         // TAHOE_CREATE_CONTRIBS: one_minus_z, bias and the elements' .z are those of the caller's covers
    bool interventional = false;   // TAHOE_CREATE_INTERVENTIONAL: tahoe_forest_set_background and its predict are served
    uint4 *elems = nullptr;        // [bins][64]
    float *one_minus_z = nullptr;  // [bins][64]; null without contribs
    uint32_t *bin_info = nullptr;  // [bins]
    float *bias = nullptr;         // [K]; null without contribs
    float div = 1.0f;              // (float)num_trees with TAHOE_OUT_AVG, else 1.0f
    int bins = 0;
    size_t paths = 0, path_elems = 0;
    int class_block = 1;           // KB: classes that share one recursion (1, 2, 4 or 8), fixed per handle
    int rows_per_tile = 0;         // R
    size_t lds_bytes = 0;          // (1 + 4 KB) R num_cols floats
    bool grid_blocks = false;      // gridDim.y runs over the class blocks (else a workgroup loops over them)
    // vector_interventional_kernel<KB, WLDS> (vector_iv.hip): its class block, rows per tile, whether the weight table sits in LDS,
    // and its LDS bytes ((1 + 4 KB) R num_cols floats and the table); fixed per handle by num_cols and K
    int iv_class_block = 1;
    int iv_rows = 0;
    bool iv_wlds = true;
    size_t iv_lds_bytes = 0;
    // TAHOE_CREATE_VECTOR_INTERACTIONS (with contribs): tahoe_forest_predict_interactions is served by
    // vector_interactions_kernel<KB, SLABS> (vector_inter.hip) -- its form (triangle slabs in LDS, or in place in the output; by
    // num_cols alone, as the sparse handle's), class block, rows of a tile (slabs; in place a wave owns one row) and LDS bytes
    // (slabs: (num_cols + 4 KB num_cols (num_cols - 1) / 2) R floats; in place: 4 num_cols floats)
    bool interactions = false;
    bool inter_slabs = true;
    int inter_class_block = 1;
    int inter_rows = 1;
    size_t inter_lds_bytes = 0;
};

// The tables and the launch shape of a handle created with TAHOE_CREATE_VECTOR_APPROX: the child deltas of
// every output beside each other, the bias column, and what vector_approx_kernel<KB, SLAB> runs as -- fixed per handle by num_cols,
// K, the device's LDS and the knobs
struct VectorApprox {
    float *dd = nullptr;      // [num_nodes][kp]: row i = the K deltas of node i as a child (a root's row and the padding are 0)
    float *bias = nullptr;    // [K] the bias column of tahoe_forest_predict_contribs on this handle
    float div = 1.0f;         // (float)num_trees with TAHOE_OUT_AVG, else 1.0f
    int class_block = 1;      // KB: outputs that share one walk (1, 2, 4 or 8)
    int kp = 1;               // floats per row of dd: K rounded up to a multiple of KB, so that a block's deltas are one aligned load
    bool slab = false;        // accumulate in a lane-private LDS row (else in place in phi_dev)
    int waves = 1;            // waves (64 rows each) per workgroup
    int stride = 0;           // floats per slab row: KB (num_cols + 1) made odd
    size_t lds_bytes = 0;     // per workgroup
    bool grid_blocks = true;  // gridDim.y runs over the class blocks (else a workgroup loops over them)
};

// The class block KB of a vector-leaf TreeSHAP kernel, the classes that share one recursion: a forced value (TAHOE_VECTOR_SHAP_KB)
// of 1, 2, 4 or 8 if it fits, else 1; without one the largest of 8, 4, 2 -- not above K rounded up to one of them -- that fits,
// else 1.  fits(c, forced): does the kernel's shape hold a block of c?  No choice changes a bit of the result.
template <class Fits>
inline int pick_class_block(int forced, int K, Fits fits)
{
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) return fits(forced, true) ? forced : 1;
    for (int c = 8; c > 1; c /= 2)
        if (c < 2 * K && fits(c, false)) return c;
    return 1;
}

// fn(std::integral_constant<int, KB>) for the runtime class block
template <class Fn>
inline void with_class_block(int kb, Fn &&fn)
{
    if (kb == 8) fn(std::integral_constant<int, 8>{});
    else if (kb == 4) fn(std::integral_constant<int, 4>{});
    else if (kb == 2) fn(std::integral_constant<int, 2>{});
    else fn(std::integral_constant<int, 1>{});
}

}  // namespace tahoe

struct tahoe_vstate {
    tahoe::VNode *nodes = nullptr;
    int32_t *roots = nullptr;
    float *leaves = nullptr;
    tahoe::VectorShap *shap = nullptr;  // non-null: created with TAHOE_CREATE_CONTRIBS and / or TAHOE_CREATE_INTERVENTIONAL
    tahoe::VectorApprox *approx = nullptr;  // non-null: created with TAHOE_CREATE_VECTOR_APPROX
};

namespace tahoe {

// vector_shap.hip.  vector_shap_build: the tables of a forest that has passed contribs_validate_sparse, from the caller's arrays,
// for flags = TAHOE_CREATE_CONTRIBS and / or TAHOE_CREATE_INTERVENTIONAL (covers: null without the former);
// vector_predict_contribs: tahoe_forest_predict_contribs on a handle with tables, entry checks included (fn: the call's name)
tahoe_status vector_shap_build(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *leaf_values,
                               const float *covers, unsigned flags);
void vector_shap_destroy(tahoe_forest *f);
// vector_iv.hip: class block, tile rows and LDS form of vector_interventional_kernel on f (sh->iv_*), from num_cols, K and the knobs
void vector_iv_shape(const tahoe_forest *f, VectorShap *sh);
// vector_shap.hip: the first kernel of tahoe_forest_predict_interactions on a handle with sh->interactions -- phi, with
// vector_contribs_kernel's bits, into row num_cols of each (row, k) matrix of out_dev
tahoe_status vector_launch_contribs_spare(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows, hipStream_t stream);
// vector_inter.hip: form, class block, tile rows and LDS bytes of vector_interactions_kernel on f (sh->inter_*), from num_cols, K
// and the knobs, and the LDS limit of the instantiation the handle uses
tahoe_status vector_inter_build(const tahoe_forest *f, VectorShap *sh);
// vector_approx.hip: the tables of TAHOE_CREATE_VECTOR_APPROX from the caller's arrays, whose covers have passed
// contribs_validate_sparse, and the form and LDS limit of the kernel the handle uses
tahoe_status vector_approx_build(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *leaf_values,
                                 const float *covers);
void vector_approx_destroy(tahoe_forest *f);

}  // namespace tahoe
