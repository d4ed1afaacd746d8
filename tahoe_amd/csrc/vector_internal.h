// The device state of a vector-leaf handle (tahoe_vector_forest_create), shared by vector.hip (create, the walk kernels) and
// vector_shap.hip (TreeSHAP on such a handle).  Internal: not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>

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

// The TreeSHAP path tables of a handle created with TAHOE_CREATE_CONTRIBS: one set of bins for the
// forest, laid out as tahoe_cstate's, except that a path's root element carries the index of the leaf's vector in .x.  They are
// kept off tahoe_forest::cs on purpose: the kernels that read tahoe_cstate take .x of a root element for a leaf value.
struct VectorShap {
    uint4 *elems = nullptr;        // [bins][64]
    float *one_minus_z = nullptr;  // [bins][64]
    uint32_t *bin_info = nullptr;  // [bins]
    float *bias = nullptr;         // [K]
    float div = 1.0f;              // (float)num_trees with TAHOE_OUT_AVG, else 1.0f
    int bins = 0;
    size_t paths = 0, path_elems = 0;
    int class_block = 1;           // KB: classes that share one recursion (1, 2, 4 or 8), fixed per handle
    int rows_per_tile = 0;         // R
    size_t lds_bytes = 0;          // (1 + 4 KB) R num_cols floats
    bool grid_blocks = false;      // gridDim.y runs over the class blocks (else a workgroup loops over them)
};

}  // namespace tahoe

struct tahoe_vstate {
    tahoe::VNode *nodes = nullptr;
    int32_t *roots = nullptr;
    float *leaves = nullptr;
    tahoe::VectorShap *shap = nullptr;  // non-null: created with TAHOE_CREATE_CONTRIBS
};

namespace tahoe {

// vector_shap.hip.  vector_shap_build: the tables of a forest that has passed contribs_validate_sparse, from the caller's arrays;
// vector_predict_contribs: tahoe_forest_predict_contribs on a handle with tables, entry checks included (fn: the call's name)
tahoe_status vector_shap_build(tahoe_forest *f, const int32_t *trees, const tahoe_sparse_node *nodes, const float *leaf_values,
                               const float *covers);
void vector_shap_destroy(tahoe_forest *f);

}  // namespace tahoe
