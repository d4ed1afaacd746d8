// What the translation units of an oblivious handle share (oblivious.hip: create and the walk; oblivious_shap.hip: the TreeSHAP,
// Saabas and interaction tables and kernels; oblivious_shap_cat.hip: those kernels for handles with category sets).  Internal: not
// part of the ABI.
#pragma once
#include "forest_internal.h"

struct tahoe_oshap;  // explanation tables of a handle of tahoe_oblivious_forest_create_ex with flags, owned by oblivious_shap.hip

struct tahoe_ostate {
    tahoe::InnerNode *splits = nullptr;
    int32_t *split_off = nullptr;
    int64_t *leaf_off = nullptr;
    float *leaves = nullptr;
    // tahoe_oblivious_forest_create_cat with splits: cats says that some record is a category set (forest_internal.h: kObCat);
    // cat_pool holds the sets wider than one word (null when there is none), cat_words its length in words
    bool cats = false;
    uint32_t *cat_pool = nullptr;
    uint32_t cat_words = 0;
    tahoe_oshap *shap = nullptr;
};

namespace tahoe {

constexpr int kObMaxDepth = 16;

// The caller's forest as the creates have checked it, for the table builds: h_splits holds the device records ({thr, fid |
// def_left << 31}; a category set as forest_internal.h describes it)
struct ObliviousSource {
    const int32_t *depths;
    const std::vector<InnerNode> *h_splits;
    const std::vector<int32_t> *h_split_off;
    const std::vector<int64_t> *h_leaf_off;
    const float *leaf_values;
    const float *leaf_covers;
    size_t num_leaves;
};

// TAHOE_ERR_INVALID_FOREST unless every leaf cover is finite and >= 0 (no device touched)
tahoe_status oblivious_shap_validate(const int32_t *depths, int num_trees, const float *leaf_covers);
// The tables `flags` (TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_APPROX_CONTRIBS | TAHOE_CREATE_INTERACTIONS |
// TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL) ask for, on the handle's device; src.leaf_covers is read only with one of the first three
tahoe_status oblivious_shap_build(tahoe_forest *f, const ObliviousSource &src, unsigned flags);
void oblivious_shap_destroy(tahoe_forest *f);

}  // namespace tahoe
