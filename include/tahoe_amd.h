/*
 * tahoe_amd.h -- C ABI of libtahoe_amd.so: the MI355X (gfx950) implementation of Tahoe's batched
 * tree-ensemble traversal.  Plain pointers and sizes only; no HIP, torch or C++ types.
 *
 * This is the drop-in boundary for the reference's forest operator API (its layer L3):
 *   reference                                        -> entry point here
 *   init_dense / init_dense_adaptive                 -> tahoe_forest_create
 *     (BaseTahoeTest.h:519-525, :605-611; dense_forest::init Struct.h:815-833;
 *      dense_adaptive_forest::init Struct.h:1756-1986)
 *   predict_dense / predict_dense_adaptive           -> tahoe_forest_predict
 *     (BaseTahoeTest.h:544-547, :599-602; forest::predict Struct.h:245-269)
 *   global `selected_algorithm` (Struct.h:11)        -> tahoe_forest_set_strategy (per handle)
 *   delete forest (BaseTahoeTest.h:594,709; leaks)   -> tahoe_forest_destroy (frees device memory)
 *   generate_forest_from_file / generate_data_from_file (BaseTahoeTest.h:267-402)
 *                                                    -> tahoe_load_model / tahoe_load_data
 *   allocate/updateDevice/updateHost (cuda_base.h:28-50), compare_GPU (cuda_base.h:98-111)
 *                                                    -> tahoe_device_* / tahoe_compare_device
 * Every device pointer is a HIP device pointer on the handle's device; `stream` is a hipStream_t
 * passed as void* (NULL = the default stream).  All predict calls are asynchronous on `stream`
 * and allocate nothing, with one exception: two strategies keep a grow-only workspace on the handle --
 * QRING a 2-byte-per-value quantised copy of the batch (plus one float per (tree, row) for the small batches it
 * walks in tree slices), and the row-streaming form of TILERING (kernel form TAHOE_FORM_TILERING_WIDE_STREAM,
 * which the create-time shape rule may pick with no environment variable set) one float per (row, tree rounded
 * up to 32), capped at 1 GiB (TAHOE_WSTREAM_SLAB_MB, read at create; larger batches are walked in slabs of rows).
 * A batch larger than any before grows the workspace inside predict: hipDeviceSynchronize + hipFree + hipMalloc,
 * which is illegal during stream capture.  tahoe_forest_reserve(rows) sizes everything beforehand; after it no
 * batch of up to `rows` rows allocates, and predict may be captured into a HIP graph.
 *
 * Handles share no global state and different handles may be used from different threads and streams
 * at the same time.  One handle serves one predict at a time: its workspace is reused by the next call,
 * so calls on the same handle must be ordered on one stream (or separated by a synchronisation).  A
 * process that drives several GPUs keeps one handle per device; predict switches to the handle's
 * device for its launches and restores the caller's.
 *
 * There is no CPU fallback: every compute entry point fails with TAHOE_ERR_NO_DEVICE when no
 * gfx950 device is usable.
 */
#ifndef TAHOE_AMD_H
#define TAHOE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAHOE_AMD_ABI_VERSION 2

/* The library is built with -fvisibility=hidden and a linker version script: the declarations below are its only
 * exported symbols (tests/test_formats_capi.py checks `nm -D`). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- status codes (the reference prints and continues, cuda_base.h:19-25; we return codes) ---- */
typedef enum {
    TAHOE_OK = 0,
    TAHOE_ERR_INVALID_ARG = 1,   /* NULL pointer, negative size, bad enum (check_params, BaseTahoeTest.h:490-516) */
    TAHOE_ERR_IO = 2,            /* file cannot be opened (BaseTahoeTest.h:273-277, :360-364) */
    TAHOE_ERR_NO_MEMORY = 3,
    TAHOE_ERR_NO_DEVICE = 4,     /* no usable gfx950 device: there is no CPU path */
    TAHOE_ERR_HIP = 5,           /* a HIP runtime call failed; text in tahoe_last_error() */
    TAHOE_ERR_INVALID_FOREST = 6,/* a reachable bottom-level node is not a leaf / fid >= num_cols */
    TAHOE_ERR_UNSUPPORTED = 7    /* requested strategy cannot run this shape */
} tahoe_status;

/* Thread-local text of the last error returned on this thread ("" if none). */
const char *tahoe_last_error(void);
int tahoe_abi_version(void);

/* ---- node encoding: dense_node_t, Struct.h:44-48, masks Struct.h:57-59 ---- */
typedef struct {
    float weight; /* branch probability; unused at inference */
    float val;    /* threshold (internal node) or leaf value */
    int32_t bits; /* fid[0:29] | def_left<<30 | is_leaf<<31 */
} tahoe_dense_node;

/* encode_node Struct.h:103-108 / dense_node_decode Struct.h:110-117 */
void tahoe_encode_node(tahoe_dense_node *n, int fid, float value, int def_left, float weight, int is_leaf);
void tahoe_decode_node(const tahoe_dense_node *n, float *value, float *weight, int *fid, int *def_left,
                       int *is_leaf);
/* tree_num_nodes Struct.h:15-17 */
int tahoe_tree_num_nodes(int depth);

/* ---- enums: algo_t Struct.h:23-27, strategy_t :29-34, output_t :37-42 ---- */
enum { TAHOE_ALGO_NAIVE = 0, TAHOE_ALGO_TREE_REORG = 1, TAHOE_ALGO_BATCH_TREE_REORG = 2 };
enum { TAHOE_FIL_SHARED_DATA = 0, TAHOE_FIL_SHARED_FOREST = 1, TAHOE_FIL_SPLIT_FOREST = 2,
       TAHOE_FIL_SPLIT_FOREST_SHARED_DATA = 3 };
enum { TAHOE_OUT_RAW = 0x0, TAHOE_OUT_AVG = 0x1, TAHOE_OUT_SIGMOID = 0x10, TAHOE_OUT_THRESHOLD = 0x100 };
/* Row-wise softmax over the classes of a multi-class handle (tahoe_forest_create_multiclass); no counterpart in the
 * reference.  tahoe_forest_create / _create_ex reject it. */
#define TAHOE_OUT_SOFTMAX 0x1000

/* forest_params_t, Struct.h:166-189 (same fields, same order). */
typedef struct {
    int num_nodes;     /* ignored for dense forests */
    int depth;         /* ps.depth: levels - 1; a tree has 2^(depth+1)-1 nodes */
    int num_trees;
    int num_cols;
    int algo;          /* algo_t; accepted and ignored (the layout is ours) */
    int output;        /* output_t bit set */
    float threshold;
    float global_bias;
    int strategy;      /* strategy_t of the FIL baseline; accepted and ignored */
    float missing;     /* "missing" sentinel: |x - missing| <= 1e-6 takes the default branch */
} tahoe_forest_params;

/* Traversal strategies of this library (the analogue of selected_algorithm 0..4, Struct.h:2168-2179). */
enum {
    TAHOE_STRATEGY_AUTO = 0,     /* selector picks from shape and LDS capacity */
    TAHOE_STRATEGY_DIRECT = 1,   /* lane = row, nodes and features straight from global memory
                                    (analogue of infer_adaptive_reorg_*, Struct.h:1196-1240) */
    TAHOE_STRATEGY_ROWTILE = 2,  /* 64-row feature-major tile in LDS, waves split the trees, top 8
                                    levels of each tree staged in LDS, deeper levels gathered from
                                    global memory, ordered leaf-sum exchange; any num_cols whose
                                    tile fits LDS */
    TAHOE_STRATEGY_TILEBLOCK = 3,/* num_cols <= 512: 128- (or 64-) row tile in LDS, four trees in
                                    flight, top 10 levels SoA in LDS, last two levels + leaves from
                                    one 32-byte block per walk; two barriers per round of 4 trees */
    TAHOE_STRATEGY_TILERING = 4, /* TILEBLOCK's data path with decoupled waves: walker waves with
                                    private tops, no barrier in the tree loop, one consumer wave adds
                                    leaf values in tree order through an LDS ring.  num_cols > 512, two
                                    forms picked at create: (a) tiles -- 32- / 16- / 8-row float32 tiles
                                    staged as they lie in memory, 2 / 4 / 8 trees per wave, 48-byte bottom
                                    blocks; (b) row streaming on 16-bit keys (num_cols <= 3072 and a multiple
                                    of 4, at most a tree per three features and 1024 trees, LDS for every
                                    level above the last two of ALL trees): one persistent workgroup per CU,
                                    rows turned into monotone 16-bit keys on their way into a ring of LDS
                                    slots, lane = tree, equal keys decided on the float32 values, leaf values
                                    through a workspace (tahoe_forest_reserve) and added in tree order by a
                                    summer wave.  AUTO's choice for wide rows when 2 x trees x depth <
                                    13 x num_cols (10 x where QRING walks three trees per lane): no quantise
                                    pass */
    TAHOE_STRATEGY_QRING = 5     /* TILERING on rank-quantised data: features and thresholds become
                                    exact 16-bit ranks (a per-predict quantise pass), 4-byte nodes.
                                    num_cols <= 256: tiles of three (or two) 64-row regions = 192 (128)
                                    rows, 14 walker waves x 3 chains (15 x 2), a batch walked as whole
                                    waves of 192-row tiles + a remainder of 128-row tiles; small batches
                                    give every tile to several workgroups, each a slice of the trees, and
                                    an ordered-sum kernel adds the leaf values in tree order (SPLIT).
                                    Forests whose features each see <= 254 thresholds (histogram-trained
                                    models) are quantised to 8-bit ranks for batches of whole tiles: 384-row
                                    tiles of three 128-row regions, six chains per lane; forests of <= 128
                                    features walk 384-row tiles on 16-bit ranks too (regions at a 16-KiB stride).
                                    Wider rows: 128-row tiles, or 64- / 32- / 16-row tiles with several
                                    trees per wave.  Forests with more than 32767 distinct thresholds on a
                                    feature are walked in groups of consecutive trees with chained float32
                                    sums (still the one sequential sum); unavailable only if a single tree
                                    exceeds that */
};
/* On a sparse handle (tahoe_sparse_forest_create): DIRECT = nodes and features from global memory,
 * ROWTILE = 64-row float32 tile in LDS, TILEBLOCK = tile + the first 512 nodes of each tree (breadth-first)
 * in LDS, walker waves + ordered ring consumer (trees of <= 65535 nodes), QRING = the same on rank-quantised
 * data: 192- / 128-row u16 tiles, three / two chains per lane, the first 9 levels of each tree as a complete
 * heap in LDS, 32-byte two-level blocks below (num_cols <= 256; tree groups as for dense forests).  AUTO
 * takes QRING when 20 x trees >= 13 x num_cols (enough walking per feature value to pay the quantise pass)
 * and the batch has >= 64 rows per CU, else TILEBLOCK, else what fits. */

typedef struct tahoe_forest tahoe_forest; /* opaque */

/* Builds the device layout from host nodes in the reference encoding: num_trees trees, each
 * 2^(depth+1)-1 nodes in heap order (children of i are 2i+1, 2i+2), tree-major (what
 * generate_forest_from_file produces, BaseTahoeTest.h:319-328).  The forest lives on the current
 * HIP device.  Validates that every reachable path ends in a leaf inside the tree and that every
 * reachable fid < num_cols (the reference reads out of bounds instead). */
tahoe_status tahoe_forest_create(tahoe_forest **out, const tahoe_dense_node *nodes,
                                 const tahoe_forest_params *params);
/* The same with options.  TAHOE_CREATE_PROB_RELAYOUT: the reference's probability-guided re-layout
 * (dense_adaptive_forest::init, Struct.h:1775-1825; swap_child :1712-1750): bottom-up, wherever dense_node_t.weight of
 * a node's left child is smaller than that of its right child, the two subtrees change places and the node is marked
 * "exchange" (the walk inverts its condition there, Struct.h:1060-1063), so that the likelier child is always the left
 * one and hot paths sit next to each other in memory.  Results are unchanged: leaf indices are still reported in the
 * original heap numbering.  Served by the strategies whose node words have a spare bit (DIRECT, ROWTILE, and QRING
 * when num_cols <= 256); without the flag `weight` is ignored, as in round 1.  tahoe_forest_create honours the
 * environment variable TAHOE_RELAYOUT=1 (read once, at create) for experiments. */
#define TAHOE_CREATE_PROB_RELAYOUT 0x1u
tahoe_status tahoe_forest_create_ex(tahoe_forest **out, const tahoe_dense_node *nodes,
                                    const tahoe_forest_params *params, unsigned flags);
void tahoe_forest_destroy(tahoe_forest *f);

/* NaN as a missing value (XGBoost, LightGBM, scikit-learn's histogram boosters, CatBoost's AsIs: the default-direction bit says
 * where a NaN goes).  A create flag for tahoe_forest_create_ex, tahoe_forest_create_multiclass, tahoe_sparse_forest_create_ex and
 * tahoe_sparse_forest_create_cat (tahoe_dense_to_sparse_ex converts node arrays and takes no flags: a converted forest gets the
 * rule from the create it is passed to); it combines with TAHOE_CREATE_PROB_RELAYOUT.  On such a handle a feature value x is missing iff
 *     isnan(x) || fabsf(x - params.missing) <= 1e-6f        (float32 arithmetic)
 * and a missing value takes the node's default branch (right iff !def_left); at a categorical split the missing test, step 1 of
 * the rule of tahoe_sparse_forest_create_cat, is this one, so a NaN takes the default branch instead of being a non-member.
 * Nothing else in any rule changes.  The sentinel keeps working beside NaN (XGBoost's DMatrix(missing=m)); any NaN bit pattern
 * counts (quiet, signalling, either sign, any payload); params.missing = NaN means "NaN only"; params.missing = +-inf stays what
 * it is without the flag (inf - inf is NaN, the band never matches, and an infinite x is an ordinary value).  Without the flag
 * every handle behaves as ever: a NaN goes left, and a NaN sentinel switches the missing branch off.
 * Every call that walks rows to a leaf applies the rule: tahoe_forest_predict, _predict_raw, _predict_leaf_idx,
 * _predict_accumulate, _predict_host, _predict_csr (a stored NaN is missing, as a stored sentinel and an absent entry are),
 * _predict_columns / _predict_column_ptrs and _predict_staged.  Strategies served: AUTO, DIRECT, ROWTILE and QRING on a dense or
 * multi-class handle -- TILEBLOCK and TILERING are TAHOE_ERR_UNSUPPORTED there, and AUTO plans only the served ones -- and every
 * strategy of a sparse or categorical handle.  Refused with TAHOE_ERR_INVALID_ARG before a device is touched: the flag together
 * with TAHOE_CREATE_CONTRIBS, _APPROX_CONTRIBS, _CAT_CONTRIBS or _PARTIAL_DEPENDENCE, and on the oblivious and vector-leaf
 * creates.  tahoe_forest_create honours no environment variable for it. */
#define TAHOE_CREATE_NAN_MISSING 0x1000u

/* Multi-class forests (XGBoost multi:softprob / multi:softmax, LightGBM multiclass: one tree per class per boosting round);
 * sparse forests take the same contract through tahoe_sparse_forest_create_ex.
 * Tree t of the num_trees trees belongs to class t % num_classes; num_trees must be a multiple of num_classes, each class then
 * has Tc = num_trees / num_classes trees.  A predict writes rows x num_classes values, row-major: margin[row][c] = the float32
 * sum of class c's leaf values added from 0.0f in increasing tree order -- bit for bit what predict_on_cpu gives on the
 * sub-forest of trees c, c + C, c + 2C, ...  Output bits, applied per element in this order: AVG divides by (float)Tc,
 * global_bias is added to every class (XGBoost's base_score), SIGMOID per element (LightGBM multiclassova), then
 * TAHOE_OUT_SOFTMAX: m = max_c z_c, e_c = expf(z_c - m), p_c = e_c / sum_c e_c (sum in class order).  THRESHOLD with
 * num_classes > 1, SOFTMAX with SIGMOID and SOFTMAX with num_classes == 1 are TAHOE_ERR_INVALID_ARG.  num_classes must be in
 * [1, 1024]; every argument is checked before a device is touched.  `flags` as for tahoe_forest_create_ex.
 * num_classes == 1 gives a handle that behaves exactly like tahoe_forest_create_ex.
 * The trees are stored class-major (class c's trees contiguous, in their relative order), so one walk over all trees
 * serves every class and QRING's quantise pass runs once per predict.  On a multi-class handle:
 *   - tahoe_forest_predict, _predict_raw and the sums of _predict_leaf_idx write rows x num_classes values; leaf indices
 *     stay leaf_dev[row * num_trees + tree] in the caller's tree numbering and the original heap numbering;
 *   - reserve (and HIP graph capture after it), set/get_strategy, get_kernel_form, get_info, profiling and check work
 *     unchanged.  Strategies served: AUTO, DIRECT, ROWTILE, QRING; TILEBLOCK and TILERING are TAHOE_ERR_UNSUPPORTED;
 *   - tahoe_forest_predict_accumulate and tahoe_forest_predict_host return TAHOE_ERR_UNSUPPORTED and launch nothing.
 * (A multi-class sparse handle serves every strategy of a sparse handle -- AUTO, DIRECT, ROWTILE, TILEBLOCK, QRING -- with
 * the same outputs; see tahoe_sparse_forest_create_ex.) */
tahoe_status tahoe_forest_create_multiclass(tahoe_forest **out, const tahoe_dense_node *nodes,
                                            const tahoe_forest_params *params, int num_classes, unsigned flags);
/* Classes of the handle: num_classes of tahoe_forest_create_multiclass or tahoe_sparse_forest_create_ex, 1 for every other
 * handle (tahoe_sparse_forest_create included), 0 for NULL. */
int tahoe_forest_num_classes(const tahoe_forest *f);

/* Per-feature contributions (path-dependent TreeSHAP: XGBoost pred_contribs, LightGBM pred_contrib).  A create flag for
 * tahoe_forest_create_ex and tahoe_forest_create_multiclass; it combines with TAHOE_CREATE_PROB_RELAYOUT.  dense_node_t.weight
 * is the cover of a node (a reach probability, a hessian sum, any positive scale): at every reachable internal node the
 * children's weights wl, wr must be finite and >= 0 with wl + wr > 0, else create returns TAHOE_ERR_INVALID_FOREST naming the
 * tree and node (checked before a device is touched; weights below a leaf are ignored).  The handle then also holds one path per
 * reachable leaf (repeated features merged), built from the caller's nodes, in 64-lane bins.  A path element whose product of
 * cover ratios (float64) is below 2^-121 is stored with a zero fraction of 0 (its 1 - z is kept from float64), so the float32
 * recursions never take the reciprocal of a subnormal: results stay finite for any valid covers, and a path term moves by
 * less than 2^-121 |leaf| per element cut from the exact value.  num_cols must be <= the device's
 * LDS bytes / 20 (8192 on an MI355X), else TAHOE_ERR_UNSUPPORTED.  Without the flag `weight` is ignored and nothing is built. */
#define TAHOE_CREATE_CONTRIBS 0x4u
/* phi_dev[rows][num_classes][num_cols + 1] <- exact Shapley values of v(S) = E[f(x) | x_S], the path-dependent expectation: at a
 * node whose feature is in S the row's branch (the rule of tahoe_forest_predict: missing sentinel -> default branch, else right
 * iff x >= thr), at any other node the mix of the two children by their cover ratios wl / (wl + wr), wr / (wl + wr).  Class c
 * is explained by its trees c, c + C, ... .  Contributions explain the margin before SIGMOID / THRESHOLD / SOFTMAX; with
 * TAHOE_OUT_AVG every column is divided by (float)Tc (trees of the class).  Column num_cols (the bias) is
 * sum_t E_t / (AVG ? Tc : 1) + global_bias, computed on the host in float64 at create and rounded once; sum_i phi_i is the
 * margin up to rounding.  Deterministic: the same bits on every call, for a row in any batch, under every strategy (the
 * strategy is not used), with or without TAHOE_CREATE_PROB_RELAYOUT; class c of a multi-class handle gives the bits of a
 * handle created from class c's sub-forest.  Asynchronous on `stream`; allocates nothing (graph-capturable).  rows == 0:
 * TAHOE_OK, nothing launched; NULL phi_dev / data_dev with rows > 0: TAHOE_ERR_INVALID_ARG; a handle (dense or sparse) created
 * without TAHOE_CREATE_CONTRIBS: TAHOE_ERR_UNSUPPORTED, nothing launched.  A sparse handle created with the flag
 * (tahoe_sparse_forest_create_ex, covers given per node) is served the same way: its paths are walked pre-order, left child
 * first, so a forest converted with tahoe_dense_to_sparse_ex holds the dense handle's path bins and gives its bits.  On a handle
 * with categorical splits (tahoe_sparse_forest_create_cat with TAHOE_CREATE_CAT_CONTRIBS) the row's branch at a categorical node
 * is that function's rule; everything else, the determinism included, is as above. */
tahoe_status tahoe_forest_predict_contribs(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, void *stream);

/* SHAP interaction values (XGBoost pred_interactions, SHAP's TreeExplainer.shap_interaction_values) of the game that
 * tahoe_forest_predict_contribs explains: same v(S), branch rule, cover ratios and class trees c, c + C, ...; the margin before
 * SIGMOID / THRESHOLD / SOFTMAX.  out_dev[((row * C + c) * (F + 1) + i) * (F + 1) + j], F = num_cols, C = num_classes:
 *  - i != j, both < F: the Shapley interaction index sum_{S in N \ {i,j}} |S|! (M - |S| - 2)! / (2 (M - 1)!) (v(S + {i,j}) -
 *    v(S + {i}) - v(S + {j}) + v(S)) summed over trees; per path leaf (o_i - z_i)(o_j - z_j) U_j(P \ {i}) / 2, U_j(P \ {i}) the
 *    unwound-path sum of j on the path without i (XGBoost's conditioned TreeSHAP); with TAHOE_OUT_AVG divided by (float)Tc.
 *    out[i][j] and out[j][i] carry the same bits; a pair that shares no path is +0.0f.
 *  - i < F: out[i][i] = phi_i - S_i in float32, phi_i bit for bit the value of tahoe_forest_predict_contribs, S_i the sum of
 *    out[i][j] over j < F, j != i, added in increasing j from 0.0f: each row sums to phi_i up to that rounding.
 *  - out[F][F] is the bias column of tahoe_forest_predict_contribs, bit for bit; out[i][F] and out[F][i] (i < F) are +0.0f.
 * Deterministic as tahoe_forest_predict_contribs (any batch, strategy, re-layout; class c = class c's sub-forest).  The
 * off-diagonal sums run in LDS for num_cols <= 71 and in place in out_dev above that (no other limit than the create flag's).
 * Asynchronous on `stream`; allocates nothing (graph-capturable).  rows == 0: TAHOE_OK, nothing launched; NULL out_dev /
 * data_dev with rows > 0, or rows * C * (F + 1)^2 * 4 overflowing size_t: TAHOE_ERR_INVALID_ARG; a handle (dense or sparse)
 * created without TAHOE_CREATE_CONTRIBS: TAHOE_ERR_UNSUPPORTED; nothing launched on any refusal.  Sparse handles created with
 * the flag, those with categorical splits included, are served as by tahoe_forest_predict_contribs.  An oblivious handle is
 * served with TAHOE_CREATE_INTERACTIONS (tahoe_oblivious_forest_create_ex, which states the order of its sums), a vector-leaf
 * handle with TAHOE_CREATE_VECTOR_INTERACTIONS (tahoe_vector_forest_create_ex): C = K there, and out[row][k] carries the bits of
 * class k on the T x K-tree expansion on a sparse handle. */
tahoe_status tahoe_forest_predict_interactions(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows, void *stream);

/* Interventional TreeSHAP (SHAP's TreeExplainer(model, data=bg), feature_perturbation="interventional"; Lundberg et al. 2020):
 * the game v_r(S) = f(x_S, r_{N \ S}) against each row r of a background data set, averaged over the background.  Served on
 * dense, sparse and multi-class handles created with TAHOE_CREATE_CONTRIBS; it reads the path bins that flag builds.  The covers are
 * checked at create as for tahoe_forest_predict_contribs but this game does not use them.  A vector-leaf handle serves it with
 * TAHOE_CREATE_INTERVENTIONAL (tahoe_vector_forest_create_ex), which takes no covers; without that flag both calls below are
 * TAHOE_ERR_UNSUPPORTED on it, TAHOE_CREATE_CONTRIBS or not.  An oblivious handle serves it with
 * TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL (tahoe_oblivious_forest_create_ex), which takes no covers either; without that flag both
 * calls are TAHOE_ERR_UNSUPPORTED on it, whatever other flag it carries.
 *
 * tahoe_forest_set_background: bg_dev is row-major bg_rows x num_cols float32 on the handle's device; the handle keeps what it
 * needs (per path bin and background row, the 64-bit ballot of the bin's lanes whose element the row follows: bins x bg_rows x
 * 8 bytes, counted in tahoe_forest_info.device_bytes), so the caller may free bg_dev on return.  Synchronous on `stream`, and
 * it allocates: not graph-capturable.  A second call replaces the background; (NULL, 0) clears it.  It also computes the bias
 * column of each class c, bias_c = (float)((sum_r (double)raw_c(r)) / bg_rows / div_c + (double)global_bias): raw_c(r) the bits
 * of tahoe_forest_predict_raw for background row r, div_c = Tc with TAHOE_OUT_AVG, else 1, the sum in background order in
 * float64 on the host, rounded once.  The handle's strategy setting is left as it was.  Refusals: NULL handle, NULL bg_dev with
 * bg_rows > 0, bg_rows x num_cols x 4 overflowing size_t or bg_rows >= 2^31: TAHOE_ERR_INVALID_ARG; a handle (dense or sparse)
 * created without TAHOE_CREATE_CONTRIBS: TAHOE_ERR_UNSUPPORTED; an allocation that fails: TAHOE_ERR_NO_MEMORY.  On any refusal
 * the previous background is kept.  On a vector-leaf handle: the same contract with C = K and div = num_trees; the masks are
 * stored once for the forest (bins x bg_rows x 8 bytes, not K times as on the T x K-tree expansion), raw_k(r) are the bits of
 * tahoe_forest_predict_raw on that handle, and device_bytes grows by bins x bg_rows x 8 + (1024 + K) x 4.
 * On an oblivious handle created with TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL: the same contract with C = K and div = num_trees,
 * raw_k(r) the bits of tahoe_forest_predict_raw on that handle.  A background row enters a tree only through its leaf index there,
 * so the handle keeps no row: per tree it keeps the occupied leaves -- R(r, t) exactly what tahoe_forest_predict_leaf_idx reports --
 * in ascending order with their integer counts (the histogram is made on the host; the order of the background rows cannot
 * affect it).  device_bytes grows by 8 x (occupied (tree, leaf) pairs; at most min(bg_rows, 2^depth) per tree) + 4 x (num_trees
 * + 1) + 4 x K. */
tahoe_status tahoe_forest_set_background(tahoe_forest *f, const float *bg_dev, size_t bg_rows, void *stream);
/* phi_dev[rows][num_classes][num_cols + 1] <- phi_i(x) = (1 / B) sum_r phi_i(x, r), B = background rows, phi_i(x, r) the exact
 * Shapley value of v_r(S) = f(x_S, r_{N \ S}) summed over class c's trees c, c + C, ... and divided by (float)Tc with
 * TAHOE_OUT_AVG.  Every node applies the rule of tahoe_forest_predict to the value it gets, background values included
 * (missing sentinel -> default branch, NaN left, else right iff x >= thr).  Per leaf path, with A = the path's features that
 * only x follows and B' = those that only r follows (one that neither follows kills the path): i in A gets
 * +leaf (|A| - 1)! |B'|! / (|A| + |B'|)!, j in B' gets -leaf |A|! (|B'| - 1)! / (|A| + |B'|)!.  In float32: per (path element,
 * row) the weights are summed over the background rows in order, times +-leaf, the paths' terms summed in a fixed order, the sum
 * divided by (float)B, then by (float)Tc with AVG.  Column num_cols is the bias column of tahoe_forest_set_background, bit for
 * bit; sum_i phi_i + bias is the margin before SIGMOID / THRESHOLD / SOFTMAX up to rounding.  Deterministic: the same bits on
 * every call, for a row in any batch, under every strategy, with or without TAHOE_CREATE_PROB_RELAYOUT, and after the same
 * background is set again; class c of a multi-class handle gives the bits of a handle created from class c's sub-forest with
 * the same background.  No atomics.  Asynchronous on `stream`; allocates nothing (graph-capturable after set_background).
 * Refusals, nothing launched: a handle (dense or sparse) created without TAHOE_CREATE_CONTRIBS, or one with no background:
 * TAHOE_ERR_UNSUPPORTED (tahoe_last_error says which); then rows == 0: TAHOE_OK; NULL phi_dev / data_dev with rows > 0, or
 * rows x C x (num_cols + 1) x 4 overflowing size_t: TAHOE_ERR_INVALID_ARG.  On a handle with categorical splits
 * (TAHOE_CREATE_CAT_CONTRIBS) x and the background rows take tahoe_sparse_forest_create_cat's rule at a categorical node.
 * On a vector-leaf handle created with TAHOE_CREATE_INTERVENTIONAL: phi_dev[rows][K][num_cols + 1], bit for bit what
 * tahoe_sparse_forest_create_ex(num_classes = K, TAHOE_CREATE_CONTRIBS) gives on the T x K-tree expansion of
 * tahoe_vector_forest_create with the same background under any valid covers, bias column included (K == 1: the bits of the sparse
 * handle on the same trees).  The K outputs of a leaf share one pass over the background per (row, path bin); the result does not
 * depend on the batch, on how many outputs share a pass, on the strategy or on whether TAHOE_CREATE_CONTRIBS is also set.  The
 * same refusals in the same order, the missing flag first (text: "vector-leaf" and the call's name).
 * On an oblivious handle created with TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL: phi_dev[rows][K][num_cols + 1], bias last.  Per tree,
 * with X the row's leaf index, the elements e = the tree's distinct features in order of first appearance from level 0 and
 * mask_e their levels: per occupied background leaf {R, count}, diff = X ^ R, the players are U = {e : diff & mask_e != 0}, u =
 * |U| (u == 0: no term); the submasks S of U are taken in descending numeric order of their bit mask over the elements, from U
 * itself down to the empty set; the live leaf is j = R ^ (diff & OR_{e in S} mask_e), s = |S|, and each e in U, e ascending, takes
 * the term w x (float)count x leaf[j][k], w = +(s - 1)! (u - s)! / u! for e in S and -s! (u - s - 1)! / u! otherwise (float64
 * quotients rounded once to float32; the count enters as one multiplication).  Per (row, k, feature): one float32 sum from +0.0f
 * over the trees in order, within a tree over its occupied leaves in ascending order, within one over the submasks in that order;
 * then one division by (float)B, then by (float)num_trees with AVG.  A feature no tree uses gives +0.0f.  The bits do not depend
 * on the batch, on the kernel form, on how many outputs share a pass, on the strategy (not used) or on the handle's other flags,
 * and in the feature columns not on the order of the background rows.  No atomics; asynchronous, allocates nothing,
 * graph-capturable after set_background.  The same refusals in the same order: the missing flag first (text: "oblivious" and the
 * call's name), no background, then rows == 0: TAHOE_OK, NULL pointers, the size overflow. */
tahoe_status tahoe_forest_predict_contribs_interventional(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows,
                                                          void *stream);

/* Saabas contributions (XGBoost predict(..., pred_contribs=True, approx_contribs=True)): one root-to-leaf walk per (row, tree)
 * instead of exact TreeSHAP.  A create flag for tahoe_forest_create_ex, tahoe_forest_create_multiclass and
 * tahoe_sparse_forest_create_ex; it combines with TAHOE_CREATE_CONTRIBS and, on dense handles, with TAHOE_CREATE_PROB_RELAYOUT.
 * dense_node_t.weight (dense) or covers[] (sparse) are checked exactly as TAHOE_CREATE_CONTRIBS checks them, before a device is
 * touched, with the same codes and messages; on a sparse handle NULL covers with the flag is TAHOE_ERR_INVALID_ARG.  The flag
 * alone builds no path bins and brings neither the num_cols <= LDS / 20 limit nor the 31-distinct-features-per-path limit of
 * TAHOE_CREATE_CONTRIBS: any num_cols (below 2^29) and any depth.  It builds one 16-byte record per normalised heap node of a
 * dense tree, or one 8-byte pair of child deltas per sparse node, counted in tahoe_forest_info.device_bytes.
 *
 * Node means, on the host in float64 from the caller's trees: E(leaf) = (double)val; at an internal node
 * E(n) = (wl * E(l) + wr * E(r)) / (wl + wr), in that order, wl / wr the children's covers as double.  Each child of a reachable
 * internal node carries d(child) = (float)(E(child) - E(n)), rounded once.  Per row and tree the row follows the path of
 * tahoe_forest_predict (missing sentinel -> default branch, NaN left, else right iff x >= thr) and every internal node n on it
 * adds d(child taken) to phi[c][fid(n)]; the padding below a shallow leaf of a dense tree adds nothing, and a tree whose root
 * is a leaf adds nothing.  phi[row][c][i], i < F, is a float32 sum from +0.0f over class c's trees c, c + C, ... in increasing
 * order, root to leaf within a tree; with TAHOE_OUT_AVG the finished sum is divided by (float)Tc.  A feature the row never
 * splits on is +0.0f.  Column F is the bias column of tahoe_forest_predict_contribs, bit for bit.  sum_i phi_i + bias is the
 * margin before SIGMOID / THRESHOLD / SOFTMAX up to rounding (the deltas of a path telescope to leaf - E(root)). */
#define TAHOE_CREATE_APPROX_CONTRIBS 0x10u
/* phi_dev[rows][num_classes][num_cols + 1] <- the Saabas contributions above; the layout of tahoe_forest_predict_contribs.
 * Deterministic: the same bits on every call, for a row in any batch, under every strategy (the strategy is not used), with or
 * without TAHOE_CREATE_PROB_RELAYOUT; class c of a multi-class handle gives the bits of a handle created from class c's
 * sub-forest; a sparse handle converted with tahoe_dense_to_sparse_ex gives the dense handle's bits.  No atomics.  Asynchronous
 * on `stream`; allocates nothing (graph-capturable).  Refusals, nothing launched, in this order: NULL handle:
 * TAHOE_ERR_INVALID_ARG; a handle created without TAHOE_CREATE_APPROX_CONTRIBS: TAHOE_ERR_UNSUPPORTED; then rows == 0: TAHOE_OK;
 * NULL phi_dev / data_dev with rows > 0, or rows x C x (num_cols + 1) x 4 overflowing size_t: TAHOE_ERR_INVALID_ARG.  On a handle
 * with categorical splits (TAHOE_CREATE_CAT_CONTRIBS) the row follows tahoe_sparse_forest_create_cat's path; the deltas are per
 * child whatever the kind of the split.  A vector-leaf handle serves the call with TAHOE_CREATE_VECTOR_APPROX
 * (tahoe_vector_forest_create_ex, which states the definition per output): C = K there, and phi[row][k] carries the bits of class
 * k of the handle's K-fold expansion under TAHOE_CREATE_APPROX_CONTRIBS; without that flag: TAHOE_ERR_UNSUPPORTED. */
tahoe_status tahoe_forest_predict_contribs_approx(tahoe_forest *f, float *phi_dev, const float *data_dev, size_t rows, void *stream);

/* TreeSHAP and Saabas contributions on a handle with categorical splits.  A create flag for tahoe_sparse_forest_create_cat only
 * (every other create: TAHOE_ERR_INVALID_ARG); it goes with TAHOE_CREATE_CONTRIBS and / or TAHOE_CREATE_APPROX_CONTRIBS and says
 * that their tables may cross categorical splits; alone it is TAHOE_ERR_INVALID_ARG.  See tahoe_sparse_forest_create_cat. */
#define TAHOE_CREATE_CAT_CONTRIBS 0x20u

/* ---- sparse (irregular) forests: sparse_node_t Struct.h:50-54, sparse_storage Struct.h:343-354,
 * init_sparse / sparse_forest::init (BaseTahoeTest.h:766-772, Struct.h:2329-2343) ---- */
typedef struct {
    float val;        /* threshold, or the output of a leaf */
    int32_t bits;     /* fid[0:29] | def_left<<30 | is_leaf<<31 (sparse_node_init, BaseTahoeTest.h:719-724) */
    int32_t left_idx; /* left child, relative to the tree's root; the right child is left_idx + 1 */
} tahoe_sparse_node;

/* trees[t] = offset of tree t's root in nodes[] (ascending); params->num_nodes = total nodes; params->depth is
 * ignored.  The handle is used with the same tahoe_forest_predict* / destroy entry points; leaf indices are
 * relative to the tree's root.  The walk is infer_one_tree_sparse (Struct.h:2217-2250) with the branch rule of
 * the live dense path (BaseTahoeTest.h:452), so a forest converted with tahoe_dense_to_sparse predicts exactly
 * what the dense forest predicts.  Rejects (TAHOE_ERR_INVALID_FOREST) child links that leave the tree or point
 * backwards, and fid >= num_cols.  One output, no covers: tahoe_sparse_forest_create_ex adds classes and TreeSHAP. */
tahoe_status tahoe_sparse_forest_create(tahoe_forest **out, const int32_t *trees, const tahoe_sparse_node *nodes,
                                        const tahoe_forest_params *params);
/* The same with classes and covers.  Every check runs before a device is touched.
 *  - num_classes: the contract of tahoe_forest_create_multiclass (tree t belongs to class t % C, num_trees % C == 0, C in
 *    [1, 1024], SOFTMAX only with C > 1, THRESHOLD only with C == 1, not SOFTMAX with SIGMOID).  The trees are stored
 *    class-major; every strategy of a sparse handle (AUTO, DIRECT, ROWTILE, TILEBLOCK, QRING) adds each class's leaf values
 *    from 0.0f in increasing tree order, and predict / predict_raw / the sums of predict_leaf_idx write rows x C values, bit
 *    for bit the single-class sparse handle of trees c, c + C, ...; leaf indices stay in the caller's tree numbering.
 *    tahoe_forest_predict_accumulate and tahoe_forest_predict_host return TAHOE_ERR_UNSUPPORTED when C > 1.
 *  - flags: TAHOE_CREATE_CONTRIBS and / or TAHOE_CREATE_APPROX_CONTRIBS (any other bit, TAHOE_CREATE_PROB_RELAYOUT included:
 *    TAHOE_ERR_INVALID_ARG; the covers of TAHOE_CREATE_APPROX_CONTRIBS are checked as below, its path lengths are not).  With it,
 *    covers[i] is the cover of nodes[i] (params->num_nodes floats; NULL: TAHOE_ERR_INVALID_ARG); at every reachable internal
 *    node the covers of nodes left_idx and left_idx + 1 must be finite and >= 0 with a positive sum (TAHOE_ERR_INVALID_FOREST
 *    naming the tree and node), and no reachable leaf's path may have more than 31 distinct features (TAHOE_ERR_UNSUPPORTED
 *    naming the tree; a deep path that repeats features is fine).  The handle then serves the four TreeSHAP calls.  Without
 *    the flag covers is ignored and may be NULL.  TAHOE_CREATE_PARTIAL_DEPENDENCE (below) is accepted too, alone or beside them:
 *    it needs covers, checks them and the depth as stated there, and serves tahoe_forest_predict_partial_dependence.
 * num_classes == 1 with flags == 0 gives a handle that behaves exactly like tahoe_sparse_forest_create. */
tahoe_status tahoe_sparse_forest_create_ex(tahoe_forest **out, const int32_t *trees, const tahoe_sparse_node *nodes,
                                           const float *covers, const tahoe_forest_params *params, int num_classes,
                                           unsigned flags);

/* Categorical splits (XGBoost enable_categorical, LightGBM categorical_feature): internal nodes whose branch tests whether the
 * row's category is in a set.  The word layout is LightGBM's cat_boundaries / cat_threshold; XGBoost's categories_nodes /
 * categories_segments / categories lists convert to it directly. */
typedef struct {
    int32_t num_splits;            /* categorical internal nodes; 0 = none */
    const int32_t *node;           /* [num_splits] strictly ascending indices into nodes[] */
    const int32_t *offset;         /* [num_splits + 1] ascending word offsets into words[], offset[0] == 0 */
    const uint32_t *words;         /* category c is a member of split k iff c < 32 * (offset[k+1] - offset[k])
                                      and bit c % 32 of words[offset[k] + c / 32] is set */
    const uint8_t *members_left;   /* NULL: members go right at every split (XGBoost); else per split, 1 = members go left
                                      (LightGBM) */
} tahoe_categorical_splits;

/* tahoe_sparse_forest_create_ex with categorical splits.  At the node of split k (node[k]) `val` is ignored and fid / def_left
 * keep their meaning; with x = the row's value of feature fid:
 *   1. If fabsf(x - missing) <= 1e-6f, the row takes the default branch, as at any node: right iff !def_left.
 *   2. Otherwise member = (x >= 0.0f && x < 32 * nwords) && bit((uint32_t)x), nwords = offset[k+1] - offset[k].  The cast
 *      truncates, so 2.7 is category 2 and -0.0 is category 0.  NaN, negative values and values past the bitset are never
 *      members.
 *   3. right = member != members_left[k] (members_left NULL: right = member).
 * With members_left == NULL this is XGBoost's Decision rule: members go right, everything else goes left, and NaN goes left as at
 * every numeric node here.  LightGBM differs in two places: it maps NaN to category 0 unless its missing type is NaN, and it
 * truncates -0.5 to category 0.  A caller who needs those bits maps such values before the call.
 * Checks, all before a device is touched, in this order:
 *   - the checks of tahoe_sparse_forest_create_ex on out, params, num_classes, flags and covers;
 *   - cats (when not NULL): num_splits < 0 or > num_nodes, NULL node / offset / words with num_splits > 0, node indices not
 *     strictly ascending or outside [0, num_nodes), offset[0] != 0, offsets that decrease, or a split wider than 2^19 words
 *     (categories < 2^24, exact in float32): TAHOE_ERR_INVALID_ARG;
 *   - the forest's structure, as tahoe_sparse_forest_create_ex checks it (TAHOE_ERR_INVALID_FOREST);
 *   - a listed node that is a leaf, or lies in no tree: TAHOE_ERR_INVALID_FOREST naming the tree and the node (relative to its
 *     root);
 *   - num_splits > 0 with TAHOE_CREATE_CONTRIBS or TAHOE_CREATE_APPROX_CONTRIBS and without TAHOE_CREATE_CAT_CONTRIBS (plain
 *     path elements are intervals per feature and a category set is not one), or with num_cols > 2^29: TAHOE_ERR_UNSUPPORTED;
 *   - TAHOE_CREATE_CAT_CONTRIBS with neither TAHOE_CREATE_CONTRIBS nor TAHOE_CREATE_APPROX_CONTRIBS (cats NULL or not):
 *     TAHOE_ERR_INVALID_ARG naming the flag;
 *   - the covers and the path lengths, as tahoe_sparse_forest_create_ex checks them for the two flags.
 * flags: those of tahoe_sparse_forest_create_ex and TAHOE_CREATE_CAT_CONTRIBS, which this function alone accepts.  With it and
 * splits, TAHOE_CREATE_CONTRIBS serves tahoe_forest_predict_contribs, _predict_interactions, _set_background and
 * _predict_contribs_interventional, and TAHOE_CREATE_APPROX_CONTRIBS serves tahoe_forest_predict_contribs_approx, with the rule
 * above at the categorical nodes.  A path's categorical edges on one feature make one path element: at split k the path going
 * right needs member == !members_left[k], going left member == members_left[k]; the element allows category c < 32 W (W the
 * widest of those splits, narrower ones zero-extended) iff every edge's bit of c equals what the edge needs, and it allows
 * every other non-missing value (beyond the words, negative, >= 2^24, NaN) iff no edge needs a member.  Numeric edges on the same
 * feature keep their interval and a value must pass both; the missing sentinel follows iff every edge's default branch is the
 * path's.  Covers, zero fractions, the bias column, the 31-features limit, num_cols <= LDS / 20 and every determinism promise of
 * the four calls are unchanged.  The sets live on the device beside the path bins (identical sets once), counted in
 * tahoe_forest_info.device_bytes.  With the flag and no splits the handle is tahoe_sparse_forest_create_ex's with the remaining
 * flags.
 * cats == NULL or num_splits == 0 gives the handle of tahoe_sparse_forest_create_ex.  A handle with splits serves DIRECT, ROWTILE
 * and TILEBLOCK (AUTO: TILEBLOCK when available, else ROWTILE, else DIRECT) with the float32 sums added in tree order, classes,
 * output bits, tahoe_forest_predict_accumulate and tahoe_forest_predict_host as tahoe_sparse_forest_create_ex describes them;
 * QRING is TAHOE_ERR_UNSUPPORTED (its 4-byte node word and its quantiser hold no set test).  Leaf indices stay relative to the
 * tree's root in the caller's numbering.  The bitsets live on the device (one header word per split beside its words), counted
 * in tahoe_forest_info.device_bytes. */
tahoe_status tahoe_sparse_forest_create_cat(tahoe_forest **out, const int32_t *trees, const tahoe_sparse_node *nodes,
                                            const float *covers, const tahoe_forest_params *params, int num_classes,
                                            unsigned flags, const tahoe_categorical_splits *cats);

/* ---- partial dependence: the model as a function of a few target features, the others averaged out by the node covers.  What
 * scikit-learn's partial_dependence(method="recursion") computes for gradient boosting, random forests and single trees. ----
 * A create flag for tahoe_sparse_forest_create_ex and tahoe_sparse_forest_create_cat (every other create keeps its refusal of an
 * unknown flag), alone or with any flag they accept; a dense model takes it through tahoe_dense_to_sparse_ex, which keeps the
 * covers of dense_node_t.weight.  It needs covers (NULL: TAHOE_ERR_INVALID_ARG) and goes with categorical splits without
 * TAHOE_CREATE_CAT_CONTRIBS (nothing here is a path element).  Checked, before a device is touched, after the checks the other
 * flags make: at every reachable internal node the covers of both children finite and >= 0 with a positive sum, and their float32
 * sum finite (TAHOE_ERR_INVALID_FOREST naming the tree and node); no reachable leaf more than 32 edges below its root
 * (TAHOE_ERR_UNSUPPORTED naming the tree: the stack depth of the walk).  No limit on the features of a path or on num_cols.
 * The handle keeps, counted in tahoe_forest_info.device_bytes: 8 bytes per node (the fractions below; max(num_nodes, 1) nodes)
 * and a workspace of 4 x num_trees x chunk bytes, chunk = the grid points one pass takes: a multiple of 64, at least 64, by
 * default what keeps the workspace near 32 MiB; the environment variable TAHOE_PD_CHUNK_ROWS, read at create, sets it (rounded
 * up to a multiple of 64).  A handle created without the flag is byte for byte what it was. */
#define TAHOE_CREATE_PARTIAL_DEPENDENCE 0x800u
/* pd_dev[g * C + c] (grid_rows x C floats, C = the handle's classes) = the partial dependence of class c at grid point g.
 * targets: host memory, num_targets distinct column ids, num_targets in [0, 32]; grid_dev: device memory, row-major grid_rows x
 * num_targets float32, column j the value of feature targets[j] (num_targets == 0: ignored, may be NULL).
 * The bits.  At create, per internal node with child covers cl, cr: tot = cl + cr, fl = cl / tot, fr = cr / tot, three IEEE float32
 * operations.  For grid point g and tree t, start at the root with w = 1.0f and acc = +0.0f.  At an internal node whose feature is
 * a target take the branch tahoe_forest_predict takes for the grid value of that feature (the missing sentinel's default branch,
 * NaN left, x >= val right, the set rule of tahoe_sparse_forest_create_cat at a categorical node), w unchanged.  At any other
 * internal node visit the left subtree with w * fl, then the right subtree with w * fr (one float32 multiply each); a child whose
 * fraction is exactly 0.0f is not visited.  At a leaf acc = acc + (w * val), the product rounded to float32 before the add (no
 * fused multiply-add).  Leaves are added in depth-first order, left before right.  pd[g][c] is the float32 sum from +0.0f of acc
 * over the trees of class c (t % C == c) in increasing t.  So: where every feature a tree splits on is a target, pd equals
 * tahoe_forest_predict_raw of that row bit for bit; a grid point's value does not depend on grid_rows, on its position in the
 * grid, on the chunk or on the call; with no targets every row gets the forest's cover-weighted mean.
 * The values are raw sums as tahoe_forest_predict_raw gives them: no AVG division, no global_bias, no output transform
 * (tahoe_transform_preds applies those).  Asynchronous on `stream`; the call allocates nothing, the targets travel as kernel
 * arguments, and a grid larger than the chunk runs chunk after chunk on the stream.
 * Refusals, in this order, nothing launched: f NULL: TAHOE_ERR_INVALID_ARG; a dense, multi-class dense, oblivious or vector-leaf
 * handle: TAHOE_ERR_UNSUPPORTED naming the call and the handle kind; a sparse handle created without
 * TAHOE_CREATE_PARTIAL_DEPENDENCE: TAHOE_ERR_UNSUPPORTED naming the flag; num_targets outside [0, 32], targets NULL with
 * num_targets > 0, a target outside [0, num_cols) or a repeated one: TAHOE_ERR_INVALID_ARG naming the index; then grid_rows == 0:
 * TAHOE_OK; pd_dev NULL, or grid_dev NULL with num_targets > 0: TAHOE_ERR_INVALID_ARG; grid_rows x num_targets or grid_rows x C
 * floats past size_t: TAHOE_ERR_INVALID_ARG. */
tahoe_status tahoe_forest_predict_partial_dependence(tahoe_forest *f, float *pd_dev, const int32_t *targets, int num_targets,
                                                     const float *grid_dev, size_t grid_rows, void *stream);

/* ---- oblivious (symmetric) forests: CatBoost models.  Every node of a level shares one split, so a tree of depth D is D
 * (feature, border) records and a table of 2^D leaves; no counterpart in the reference. ---- */
typedef struct {
    float thr;
    int32_t bits; /* fid[0:29] | def_left<<30 */
} tahoe_oblivious_split;
/* depths[t] in [0, 16], one per tree (trees may differ; depth 0 is a single leaf).  splits holds sum_t depths[t] records,
 * tree-major, record l of tree t the split of level l (may be NULL when that sum is 0).  leaf_values holds sum_t 2^depths[t] *
 * leaf_dim floats in CatBoost's layout: tree-major, then leaf index, then the K = leaf_dim values of that leaf.  Of `params`,
 * num_trees, num_cols, output, threshold, global_bias and missing are used; depth, num_nodes, algo and strategy are ignored.
 * Level l applies the rule of tahoe_forest_predict to the row's value x of its feature: fabsf(x - missing) <= 1e-6f takes the
 * default branch (right iff !def_left), NaN goes left, else right iff x >= thr.  Leaf index = sum_l bit_l << l: level 0 is the
 * least significant bit (CatBoost's numbering); tahoe_forest_predict_leaf_idx reports it.  margin[row][k] is the float32 sum
 * from +0.0f over trees 0..T-1 in order of leaf_values[t][idx_t][k] -- bit for bit what the heap expansion of the forest gives on
 * a handle of tahoe_forest_create (K == 1) or, with tree t * K + k carrying class k's leaves, of tahoe_forest_create_multiclass.
 * Output bits: K == 1 as tahoe_forest_create; K > 1 the contract of tahoe_forest_create_multiclass with C = K, except that AVG
 * divides by (float)num_trees (every tree feeds every class).  tahoe_forest_num_classes returns K.
 * Checks, all before a device is touched, in this order: NULL out / depths / leaf_values / params, num_trees < 0, NULL splits with
 * a positive sum of depths, leaf_dim outside [1, 1024], num_cols < 0 or unknown output bits, the output combinations
 * tahoe_forest_create_multiclass refuses (SOFTMAX with K == 1 or with SIGMOID, THRESHOLD with K > 1): TAHOE_ERR_INVALID_ARG; a
 * depth outside [0, 16]: TAHOE_ERR_INVALID_ARG naming the tree; a fid >= num_cols: TAHOE_ERR_INVALID_FOREST naming the tree and
 * the level.
 * The handle keeps 8 bytes per split, 12 bytes per tree and the leaf table (tahoe_forest_info.device_bytes; depth = the largest
 * depth, is_sparse = 0).  Served: tahoe_forest_predict, _predict_raw, _predict_leaf_idx (leaf_dev[row * num_trees + tree], sums
 * rows x K), _predict_accumulate (K == 1; K > 1 TAHOE_ERR_UNSUPPORTED), _reserve (nothing to size: predict allocates nothing and
 * can be captured), set/get_strategy, get_kernel_form, get_info, check, profiling, destroy.  Strategies: DIRECT (kernel form
 * TAHOE_OBLIVIOUS_FORM_DIRECT: features from global memory, any num_cols), ROWTILE (TAHOE_OBLIVIOUS_FORM_TILE: one wave per
 * 64-row float32 tile in LDS; needs 256 x num_cols bytes of LDS), AUTO = ROWTILE when the tile fits, else DIRECT; TILEBLOCK,
 * TILERING and QRING are TAHOE_ERR_UNSUPPORTED.
 * Out of scope, TAHOE_ERR_UNSUPPORTED with nothing launched and a text that says "oblivious": tahoe_forest_predict_csr,
 * _reserve_csr (and _get_csr_plan: form TAHOE_FORM_NONE) unless the handle comes from tahoe_oblivious_forest_create_ex or
 * _create_cat with TAHOE_CREATE_CSR; _predict_host, _set_stages, _predict_staged (_get_staged_strategy: 0),
 * _predict_contribs, _predict_contribs_approx, _predict_interactions, and _set_background with
 * _predict_contribs_interventional, unless the handle comes from tahoe_oblivious_forest_create_ex with that call's flag
 * (TAHOE_CREATE_STAGED for the three staged calls).  CatBoost's one-hot splits are
 * category sets (tahoe_oblivious_forest_create_cat); a CTR split is a border on a column the caller computes. */
tahoe_status tahoe_oblivious_forest_create(tahoe_forest **out, const int32_t *depths, const tahoe_oblivious_split *splits,
                                           const float *leaf_values, const tahoe_forest_params *params, int leaf_dim);
/* SHAP interaction values on an oblivious handle: accepted by tahoe_oblivious_forest_create_ex alone (every other create:
 * TAHOE_ERR_INVALID_ARG), alone or with TAHOE_CREATE_CONTRIBS and / or TAHOE_CREATE_APPROX_CONTRIBS. */
#define TAHOE_CREATE_INTERACTIONS 0x40u
/* Interventional TreeSHAP on an oblivious handle (tahoe_forest_set_background, tahoe_forest_predict_contribs_interventional):
 * accepted by tahoe_oblivious_forest_create_ex alone (every other create refuses it as an unknown flag; it is not
 * TAHOE_CREATE_INTERVENTIONAL, 0x80, which stays an unknown flag on this create), alone -- it needs no covers -- or with any of the
 * three flags above. */
#define TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL 0x200u
/* Staged prediction on an oblivious or a vector-leaf handle (tahoe_forest_set_stages, tahoe_forest_predict_staged,
 * tahoe_forest_get_staged_strategy; CatBoost's staged_predict / ntree_end, XGBoost's iteration_range on multi_output_tree models, a
 * random forest's output against n_estimators): accepted by tahoe_oblivious_forest_create_ex, tahoe_oblivious_forest_create_cat
 * and tahoe_vector_forest_create_ex, alone -- it reads no cover: leaf_covers / covers may be NULL -- or beside any of their other
 * flags; every other create refuses it as an unknown flag.  It builds no table: device_bytes is that of the handle without it until
 * stages are set, and everything else the handle serves is bit for bit what the handle without the flag gives.  A handle created
 * without it keeps refusing the three calls, with the same codes and texts as before the flag existed. */
#define TAHOE_CREATE_STAGED 0x2000u
/* CSR rows on an oblivious or a vector-leaf handle (tahoe_forest_predict_csr, tahoe_forest_reserve_csr, tahoe_forest_get_csr_plan,
 * with the contract stated at tahoe_forest_predict_csr and nothing new): accepted by tahoe_oblivious_forest_create_ex,
 * tahoe_oblivious_forest_create_cat and tahoe_vector_forest_create_ex, alone -- it reads no cover: leaf_covers / covers may be
 * NULL, and it joins no cover check -- or beside any of their other flags; every other create refuses it as an unknown flag.  It
 * builds no table: device_bytes is that of the handle without it until the first chunked CSR call (or tahoe_forest_reserve_csr)
 * allocates the chunk buffer, and everything else the handle serves is bit for bit what the handle without the flag gives.  A
 * handle created without it keeps refusing the three calls, with the same codes and texts as before the flag existed.
 * ROWTILE, and AUTO where the 64-row tile fits (256 x num_cols bytes of LDS) and nnz x ceil(K / 8) <= 96 x rows, stage the tile
 * straight from the CSR arrays (kernel forms TAHOE_OBLIVIOUS_FORM_CSR_TILE / TAHOE_VECTOR_FORM_CSR_TILE; with K > 8 every block of
 * 8 classes stages it again); DIRECT, a tile that does not fit, AUTO on rows that store more than that, and AUTO under
 * TAHOE_CSR_FUSED=0 run the handle's own kernels on densified chunks (tahoe_forest_get_csr_plan tells).
 * Still refused on these handles, flag or not, because they take dense rows only: leaf indices from CSR, staged output from CSR,
 * predict_accumulate from CSR, every explanation call from CSR; and there is no DIRECT kernel that reads CSR without a dense
 * chunk. */
#define TAHOE_CREATE_CSR 0x4000u
/* The same handle with explanations.  flags: a subset of TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_APPROX_CONTRIBS |
 * TAHOE_CREATE_INTERACTIONS | TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL | TAHOE_CREATE_STAGED (staged prediction, stated at the flag
 * and at tahoe_forest_set_stages; Tc = num_trees, C = K) | TAHOE_CREATE_CSR (CSR rows, stated at the flag), each serving its own call(s) and no other; with flags == 0
 * leaf_covers is ignored and the call is tahoe_oblivious_forest_create (which is this call with NULL, 0).  leaf_covers holds
 * sum_t 2^depths[t] floats, one per leaf in the order of the leaves: the training weight that reached the leaf (CatBoost's
 * leaf_weights).  Checks, before a device is touched and after those of tahoe_oblivious_forest_create: another flag bit, or one of
 * the first three flags with leaf_covers == NULL: TAHOE_ERR_INVALID_ARG; with one of the first three flags a cover that is
 * negative, NaN or infinite: TAHOE_ERR_INVALID_FOREST naming the tree and the leaf.  TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL alone
 * reads no cover (leaf_covers may be NULL); a handle created without it is bit for bit and byte for byte what it was before that
 * flag existed.
 * Covers of the implicit nodes: the float64 sum of the leaf covers below.  A node of positive cover mixes its children by
 * w_child / (w_l + w_r); a node of cover 0 mixes them 1/2 and 1/2 (the limit of adding one epsilon to every leaf cover).  Leaves
 * and whole subtrees of cover 0 are therefore accepted -- CatBoost models have them -- where TAHOE_CREATE_CONTRIBS on a dense or
 * sparse handle refuses a node whose children both have cover 0.  Node means E(n) = (w_l E(l) + w_r E(r)) / (w_l + w_r), or
 * (E(l) + E(r)) / 2 at a node of cover 0, in float64.
 * TAHOE_CREATE_CONTRIBS: tahoe_forest_predict_contribs is served -- path-dependent TreeSHAP as defined there (predict's branch
 * rule, repeated features merged, contributions to the margin), phi_dev rows x K x (num_cols + 1), bias last; zero fractions below
 * 2^-121 count as 0.  With AVG every column is divided by (float)num_trees.  Bias column k = sum_t E_t[k] / (AVG ? T : 1) +
 * global_bias in float64, rounded once (E_t[k]: the sum over the tree's leaves of value x product of the path's mixing ratios).
 * Per (row, class, feature) the float32 sum runs from +0.0f over the trees in order and, within a tree, over the leaves in order
 * of their index (a leaf the row weighs 0 is skipped): results do not depend on the batch or the kernel form.
 * TAHOE_CREATE_APPROX_CONTRIBS: tahoe_forest_predict_contribs_approx is served -- Saabas contributions as defined there on the
 * implicit heap: each child carries d = (float)(E(child) - E(n)); per tree, level 0 first, the row adds the taken child's d to
 * phi[k][fid of the level], one float32 add per (tree, level) from +0.0f, then / (float)num_trees with AVG; the same bias column,
 * bit for bit.  On covers whose node sums are exact in float32 it gives the bits of the heap expansion on a dense handle.
 * TAHOE_CREATE_INTERACTIONS: tahoe_forest_predict_interactions is served -- the interaction values defined there of the game above,
 * out_dev rows x K x (num_cols + 1)^2.  Per tree the elements are its distinct features in order of first appearance from level
 * 0; per leaf the row weighs (the rule above) and per pair c < e of elements the term is w_e(P \ {c}) (o_c ? 1 - z_c : -z_c) / 2
 * leaf[k], w_e(P \ {c}) the TreeSHAP weight of e on the path without c.  Off-diagonal [i][j], i != j < num_cols: one float32 sum
 * per unordered pair from +0.0f, trees in order, within a tree the leaves in order, then / (float)num_trees with AVG, stored at
 * [i][j] and [j][i].  [i][i] = phi_i - S_i in float32: phi_i the bits of tahoe_forest_predict_contribs on a handle with
 * TAHOE_CREATE_CONTRIBS, S_i the sum from +0.0f of the final [i][j], j != i ascending.  [F][F] is the bias column above; the rest
 * of row and column F, and the rows and columns of features no tree uses, are +0.0f.  Results do not depend on the batch.
 * The calls allocate nothing and can be captured.  The tables count in device_bytes: 8 bytes per (leaf, distinct feature of its
 * tree) and 4 per leaf (TreeSHAP and the interaction values, which share them), 4 K bytes per implicit child (Saabas), 8 bytes per
 * split and per (tree, distinct feature) more for the interaction values.  A call whose flag the handle lacks stays
 * TAHOE_ERR_UNSUPPORTED as above.
 * TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL: tahoe_forest_set_background and tahoe_forest_predict_contribs_interventional are served as
 * defined there.  At create it adds to device_bytes 2312 bytes (two 17 x 17 float32 weight tables) beside TAHOE_CREATE_CONTRIBS or
 * TAHOE_CREATE_INTERACTIONS, whose splits and elements it shares; alone, on a forest with at least one split, 8 bytes per split
 * + 4 per feature the forest uses + 8 per (tree, distinct feature) + 12 num_trees + 4 K + 20 (offsets, a bias column and the
 * one-element placeholders of the tables it does not build) + 2312.  One kernel form (LDS or in place) serves all the handle's
 * explanation calls; with this flag the weight tables count in the LDS the LDS form needs.  What a background adds is stated at
 * tahoe_forest_set_background. */
tahoe_status tahoe_oblivious_forest_create_ex(tahoe_forest **out, const int32_t *depths, const tahoe_oblivious_split *splits,
                                              const float *leaf_values, const float *leaf_covers,
                                              const tahoe_forest_params *params, int leaf_dim, unsigned flags);
/* tahoe_oblivious_forest_create_ex with category-set splits (CatBoost's one-hot splits; a set of any size).  Everything but cats
 * is as there: the same four flags and TAHOE_CREATE_STAGED, each serving its own call(s); TAHOE_CREATE_CAT_CONTRIBS stays an unknown flag here, because
 * no explanation table of an oblivious handle holds a threshold or an interval -- every explanation follows the sets as it stands.
 * cats is the struct of tahoe_sparse_forest_create_cat in the same word layout; cats->node[k] is an index into splits[], the record
 * of one (tree, level), strictly ascending in [0, sum_t depths[t]).  At such a level thr is ignored, fid and def_left keep their
 * meaning, and the level's bit is steps 1-3 of tahoe_sparse_forest_create_cat, word for word: the missing sentinel takes the
 * default branch (right iff !def_left); otherwise member = (x >= 0.0f && x < 32 * nwords) && bit((uint32_t)x) -- the cast
 * truncates; NaN, negative values, values past the words and values >= 2^24 are never members -- and right = member !=
 * members_left[k].  Level l still sets bit l of the leaf index; the order of the sums and the output bits are those of
 * tahoe_oblivious_forest_create.  A CatBoost one-hot split "hash == value goes right" is the set {id of value} with members_left
 * NULL; a CTR split is an ordinary border on a column the caller computes.
 * cats == NULL or num_splits == 0 gives the handle of tahoe_oblivious_forest_create_ex, bit for bit and byte for byte (that call
 * is this one with NULL).
 * Checks, all before a device is touched, in this order: those of tahoe_oblivious_forest_create_ex, in its order; then the cats
 * checks of tahoe_sparse_forest_create_cat with its codes and texts (TAHOE_ERR_INVALID_ARG), the bound on num_splits and node[]
 * being sum_t depths[t], a split wider than 2^19 words refused; then, with num_splits > 0, num_cols > 2^28: TAHOE_ERR_UNSUPPORTED
 * (the split record keeps bits 28 to 30 of its fid word for the kind of split).
 * device_bytes: a set of at most one word (categories < 32; the one-hot case) rides in its 8-byte split record and adds nothing.
 * A set of nwords >= 2 words adds 4 * (1 + nwords) bytes, a header word and its words in one pool:
 *   device_bytes(cats) = device_bytes(NULL) + 4 * sum over the splits k with nwords_k >= 2 of (1 + nwords_k).
 * The explanation tables share that pool and grow by nothing.
 * Served, under the same flags and with the same kernel forms, strategies (DIRECT, ROWTILE, AUTO) and graph capture: everything
 * tahoe_oblivious_forest_create_ex serves -- tahoe_forest_predict, _predict_raw, _predict_leaf_idx, _predict_accumulate (K == 1),
 * _reserve, _predict_contribs, _predict_contribs_approx, _predict_interactions, _set_background,
 * _predict_contribs_interventional, and _set_stages / _predict_staged / _get_staged_strategy, their definitions unchanged except that "the row's bit at a level" is the rule above.  The
 * elements of a tree are still its distinct features in order of first appearance, whether a feature appears numeric,
 * categorical, or both.  What that handle refuses stays refused with the same texts. */
tahoe_status tahoe_oblivious_forest_create_cat(tahoe_forest **out, const int32_t *depths, const tahoe_oblivious_split *splits,
                                               const float *leaf_values, const float *leaf_covers,
                                               const tahoe_forest_params *params, int leaf_dim, unsigned flags,
                                               const tahoe_categorical_splits *cats);

/* ---- vector-leaf forests: irregular trees whose leaves hold K = leaf_dim values (scikit-learn's RandomForestClassifier,
 * ExtraTreesClassifier, DecisionTreeClassifier and multi-output regressors; XGBoost multi_strategy = "multi_output_tree"); no
 * counterpart in the reference. ----
 * trees and nodes are exactly what tahoe_sparse_forest_create takes: root offsets ascending, params->num_nodes the total, an
 * internal node carries val = threshold and bits = fid | def_left<<30, its children are left_idx and left_idx + 1 relative to
 * the root.  At a leaf (is_leaf<<31) val is ignored and left_idx is the index of the leaf's vector: leaf_values[left_idx * K ..
 * + K), in [0, num_leaf_vectors).  Leaves may share a vector, and the vectors may come in any order.  Of `params`, num_nodes,
 * num_trees, num_cols, output, threshold, global_bias and missing are used; depth, algo and strategy are ignored.
 * Every node applies the rule of tahoe_forest_predict to the row's value x of its feature: fabsf(x - missing) <= 1e-6f takes the
 * default branch (right iff !def_left), NaN goes left, else right iff x >= val.  margin[row][k] is the float32 sum from +0.0f
 * over trees 0..T-1 in order of the row's leaf vector element k -- bit for bit what tahoe_sparse_forest_create_ex(num_classes =
 * K) gives on the T x K-tree expansion whose tree t * K + k is tree t with val = leaf_values[left_idx * K + k] at its leaves,
 * and with K == 1 what tahoe_sparse_forest_create gives.
 * Output bits: K == 1 as tahoe_sparse_forest_create; K > 1 the contract of tahoe_forest_create_multiclass with C = K, AVG
 * dividing by (float)num_trees (every tree feeds every class; the expansion has num_trees / C = T, so the two agree).
 * tahoe_forest_num_classes returns K.
 * Checks, all before a device is touched: NULL out / params, NULL trees / nodes with num_trees > 0, NULL leaf_values with
 * num_leaf_vectors > 0, num_trees < 0, num_nodes < 0, num_leaf_vectors < 0, leaf_dim outside [1, 1024], num_cols < 0 or unknown
 * output bits, the output combinations tahoe_forest_create_multiclass refuses (SOFTMAX with K == 1 or with SIGMOID, THRESHOLD with
 * K > 1): TAHOE_ERR_INVALID_ARG; the structure checks of tahoe_sparse_forest_create (ascending roots, children after the node and
 * inside the tree, fid < num_cols): TAHOE_ERR_INVALID_FOREST; a leaf whose left_idx is outside [0, num_leaf_vectors):
 * TAHOE_ERR_INVALID_FOREST naming the tree and the node (relative to its root).
 * The handle keeps 16 bytes per node (the 12-byte node padded: one aligned gather per step), 4 bytes per tree and the leaf table
 * (tahoe_forest_info.device_bytes; depth = the deepest leaf, is_sparse = 0).  Served: tahoe_forest_predict, _predict_raw,
 * _predict_leaf_idx (leaf_dev[row * num_trees + tree] = the leaf node's index relative to its root, as on a sparse handle; sums
 * rows x K), _reserve (nothing to size: predict allocates nothing and can be captured), set/get_strategy, get_kernel_form,
 * get_info, check, profiling, destroy.  Strategies: DIRECT (kernel form TAHOE_VECTOR_FORM_DIRECT: features from global memory,
 * any num_cols), ROWTILE (TAHOE_VECTOR_FORM_TILE: one wave per 64-row float32 tile in LDS; needs 256 x num_cols bytes of LDS),
 * AUTO = ROWTILE when the tile fits, else DIRECT; TILEBLOCK, TILERING and QRING are TAHOE_ERR_UNSUPPORTED.
 * Out of scope, TAHOE_ERR_UNSUPPORTED with nothing launched and a text that names the call and says "vector-leaf":
 * tahoe_forest_predict_accumulate, _predict_host; _predict_csr, _reserve_csr (and _get_csr_plan: form TAHOE_FORM_NONE) unless the
 * handle comes from _create_ex with TAHOE_CREATE_CSR;
 * _set_stages, _predict_staged (_get_staged_strategy: 0) unless the handle comes from _create_ex with TAHOE_CREATE_STAGED;
 * _predict_contribs_approx unless the handle comes from _create_ex with
 * TAHOE_CREATE_VECTOR_APPROX; _predict_contribs unless the handle comes from tahoe_vector_forest_create_ex with
 * TAHOE_CREATE_CONTRIBS; _set_background and _predict_contribs_interventional unless it
 * comes from there with TAHOE_CREATE_INTERVENTIONAL; _predict_interactions unless it comes from there with
 * TAHOE_CREATE_VECTOR_INTERACTIONS.  Categorical splits are not represented. */
tahoe_status tahoe_vector_forest_create(tahoe_forest **out, const int32_t *trees, const tahoe_sparse_node *nodes,
                                        const float *leaf_values, int64_t num_leaf_vectors, const tahoe_forest_params *params,
                                        int leaf_dim);
/* Interventional TreeSHAP on a vector-leaf handle: a create flag that tahoe_vector_forest_create_ex alone accepts (every other
 * create: its "unknown create flags" refusal), alone or with TAHOE_CREATE_CONTRIBS. */
#define TAHOE_CREATE_INTERVENTIONAL 0x80u
/* SHAP interaction values on a vector-leaf handle: a create flag that tahoe_vector_forest_create_ex alone accepts (every other
 * create: its refusal of an unknown flag), and only together with TAHOE_CREATE_CONTRIBS; TAHOE_CREATE_INTERVENTIONAL may join. */
#define TAHOE_CREATE_VECTOR_INTERACTIONS 0x100u
/* Saabas contributions on a vector-leaf handle: a create flag that tahoe_vector_forest_create_ex alone accepts (every other
 * create: TAHOE_ERR_INVALID_ARG, its refusal of an unknown flag), alone or with any of the three flags above.  It is not
 * TAHOE_CREATE_APPROX_CONTRIBS (0x10), which stays an unknown flag on that create, as does 0x200. */
#define TAHOE_CREATE_VECTOR_APPROX 0x400u
/* The same handle with explanations.  flags: a subset of TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_INTERVENTIONAL |
 * TAHOE_CREATE_VECTOR_INTERACTIONS | TAHOE_CREATE_VECTOR_APPROX | TAHOE_CREATE_STAGED (staged prediction, stated at the flag and
 * at tahoe_forest_set_stages; Tc = num_trees, C = K; it reads no covers and joins none of the checks below) | TAHOE_CREATE_CSR
 * (CSR rows, stated at the flag; no covers and no checks either); with flags == 0 covers is ignored and the call is tahoe_vector_forest_create (which is this
 * call with NULL, 0), bit for bit; a handle created without TAHOE_CREATE_INTERVENTIONAL or without
 * TAHOE_CREATE_VECTOR_INTERACTIONS is bit for bit and byte for byte what it was before that flag existed.  With
 * TAHOE_CREATE_CONTRIBS covers[i] is the cover of nodes[i] (num_nodes floats; scikit-learn's tree_.weighted_n_node_samples).
 * TAHOE_CREATE_INTERVENTIONAL serves tahoe_forest_set_background and tahoe_forest_predict_contribs_interventional as defined there.
 * Alone it ignores covers (NULL is fine: that game does not use them) and runs, of the checks below, the flag check and the
 * 31-distinct-features check (same code and text) and the num_cols limit; the handle then keeps only what that game reads, 16
 * bytes per path element in 64-lane bins and 4 bytes per bin -- the bins are built as if every cover were 1, which changes no
 * feature, bound, missing / NaN flag, length, packing, rank or round, and an element's zero fraction is never read -- and
 * tahoe_forest_predict_contribs stays TAHOE_ERR_UNSUPPORTED.  With both flags covers are required and checked, one set of tables
 * serves both calls and device_bytes is that of the TAHOE_CREATE_CONTRIBS handle.
 * Checks, before a device is touched and after those of tahoe_vector_forest_create, with the codes and texts of
 * tahoe_sparse_forest_create_ex: another flag bit: TAHOE_ERR_INVALID_ARG naming the bit; TAHOE_CREATE_VECTOR_INTERACTIONS without
 * TAHOE_CREATE_CONTRIBS: TAHOE_ERR_INVALID_ARG naming both flags; TAHOE_CREATE_CONTRIBS with covers == NULL:
 * TAHOE_ERR_INVALID_ARG; a reachable internal node whose children's covers are not finite, negative or sum to 0:
 * TAHOE_ERR_INVALID_FOREST naming the tree and the node; a reachable leaf whose path has more than 31 distinct features:
 * TAHOE_ERR_UNSUPPORTED naming the tree.  With a device: num_cols above a fifth of the LDS in floats (20 B per column):
 * TAHOE_ERR_UNSUPPORTED.
 * Served with the flag: tahoe_forest_predict_contribs as defined there (predict's branch rule, repeated features merged,
 * contributions to the margin, zero fractions below 2^-121 count as 0), phi_dev rows x K x (num_cols + 1), bias last; with AVG every
 * column is divided by (float)num_trees.  phi[row][k] is bit for bit what tahoe_sparse_forest_create_ex(num_classes = K,
 * TAHOE_CREATE_CONTRIBS) gives for class k on the T x K-tree expansion above when every copy of tree t carries tree t's covers;
 * with K == 1 the bits of the sparse handle on the same trees, bias column included.  Bias column k = sum_t E_t[k] / (AVG ? T : 1)
 * + global_bias in float64, rounded once, E_t[k] the cover-weighted mean of element k over tree t's leaves.  The K outputs of a
 * leaf share one evaluation of its path; results do not depend on the batch, on how many outputs share an evaluation or on the
 * strategy (which the call does not use).  The call is asynchronous, allocates nothing and can be captured.
 * The tables count in device_bytes: 20 bytes per path element in 64-lane bins, once for the forest -- not once per output as on
 * the expansion -- and 4 K bytes of bias.
 * TAHOE_CREATE_VECTOR_INTERACTIONS (with TAHOE_CREATE_CONTRIBS: covers required and checked as above) adds no table -- device_bytes
 * is that of the handle without it -- and serves tahoe_forest_predict_interactions as defined there: out_dev rows x K x
 * (num_cols + 1) x (num_cols + 1), asynchronous, allocating nothing, capturable, two kernels in stream order; rows == 0 is
 * TAHOE_OK, then NULL pointers and an output that overflows size_t are TAHOE_ERR_INVALID_ARG.  out[row][k] is bit for bit what
 * tahoe_sparse_forest_create_ex(num_classes = K, TAHOE_CREATE_CONTRIBS) gives for class k on the expansion with tree t's covers on
 * every copy (K == 1: the sparse handle's bits on the same trees): the accumulation form is the sparse handle's, chosen by num_cols
 * alone (LDS partial sums of four waves to num_cols = 71, in place in the output above), the diagonal is phi_i minus the row's
 * off-diagonal sum ascending from 0.0f, row and column num_cols are +0.0f but the corner, which is the bias.  The conditioned
 * recursion of a (row, path, conditioning element) runs once for a block of up to 8 outputs; results do not depend on the block,
 * the batch or the strategy.
 * TAHOE_CREATE_VECTOR_APPROX serves tahoe_forest_predict_contribs_approx: Saabas contributions of every output, phi_dev rows x K x
 * (num_cols + 1), bias last.  It needs covers (NULL: TAHOE_ERR_INVALID_ARG, "TAHOE_CREATE_VECTOR_APPROX needs covers"), checked as
 * tahoe_sparse_forest_create_ex checks them for TAHOE_CREATE_APPROX_CONTRIBS, with its codes and texts: the sibling covers at
 * every reachable internal node finite, >= 0 and of positive sum.  Path lengths are not checked: alone, the flag knows neither the
 * 31-distinct-features limit nor the 20-B-per-column limit and builds no path bins; with other flags each flag keeps its own
 * checks.  Definition: node means per output k in float64, E_k(n) = (wl * E_k(l) + wr * E_k(r)) / (wl + wr) with wl, wr the
 * children's covers, and E_k = (double)leaf_values[left_idx * K + k] at a leaf; each child of a reachable internal node carries
 * d_k = (float)(E_k(child) - E_k(n)).  The row follows predict's path, and every internal node on it adds the taken child's d_k to
 * phi[k][fid]: per (row, k, feature) one float32 sum from +0.0f, trees 0..T-1 in order, root to leaf, then with AVG one division
 * by (float)num_trees.  Bias column k is bit for bit the bias of tahoe_forest_predict_contribs on a vector-leaf handle (above).
 * phi[row][k] is bit for bit what tahoe_sparse_forest_create_ex(num_classes = K, TAHOE_CREATE_APPROX_CONTRIBS) gives for class k on
 * the T x K-tree expansion with tree t's covers on every copy; with K == 1 the bits of the sparse handle on the same trees.  One
 * walk per (row, tree) feeds a block of up to 8 outputs; results do not depend on the batch, on the block, on where the sums are
 * accumulated (LDS or phi_dev) or on the strategy, which the call does not use.  rows == 0 is TAHOE_OK, then NULL pointers
 * ("null argument") and an output that overflows size_t are TAHOE_ERR_INVALID_ARG.  The call is asynchronous, allocates nothing
 * and can be captured.  device_bytes grows by exactly the new tables: 4 Kp max(num_nodes, 1) bytes of deltas, Kp = K rounded up
 * to a multiple of the handle's class block (1, 2, 4 or 8; DESIGN.md section 29 has the rule), and 4 K bytes of bias.  Every other
 * call on a handle with the flag gives the bits it gives without it.
 * On a handle created without TAHOE_CREATE_VECTOR_APPROX tahoe_forest_predict_contribs_approx stays TAHOE_ERR_UNSUPPORTED as
 * above, _predict_interactions on
 * one created without TAHOE_CREATE_VECTOR_INTERACTIONS, _set_background and _predict_contribs_interventional on one created
 * without TAHOE_CREATE_INTERVENTIONAL. */
tahoe_status tahoe_vector_forest_create_ex(tahoe_forest **out, const int32_t *trees, const tahoe_sparse_node *nodes,
                                           const float *leaf_values, int64_t num_leaf_vectors, const float *covers,
                                           const tahoe_forest_params *params, int leaf_dim, unsigned flags);

/* dense2sparse (BaseTahoeTest.h:728-764).  *nodes_out / *trees_out: tahoe_free_host. */
tahoe_status tahoe_dense_to_sparse(const tahoe_dense_node *dense, int num_trees, int depth,
                                   tahoe_sparse_node **nodes_out, int32_t **trees_out, size_t *num_nodes_out);
/* The same nodes and trees, and *covers_out[i] = the weight of the dense node that sparse node i came from (tahoe_free_host):
 * the covers tahoe_sparse_forest_create_ex takes. */
tahoe_status tahoe_dense_to_sparse_ex(const tahoe_dense_node *dense, int num_trees, int depth, tahoe_sparse_node **nodes_out,
                                      int32_t **trees_out, float **covers_out, size_t *num_nodes_out);
/* Deterministic irregular forest (BASELINE config 5): per tree a depth limit in [min_depth, max_depth]; nodes
 * below min_depth become leaves with probability leaf_prob; at most max_tree_nodes per tree.  With nodes == NULL
 * only *num_nodes is computed (call twice). */
tahoe_status tahoe_synth_sparse_forest(tahoe_sparse_node *nodes, int32_t *trees, size_t *num_nodes, int num_trees,
                                       int num_cols, int min_depth, int max_depth, float leaf_prob,
                                       int max_tree_nodes, uint64_t seed);

/* (Multi-class handles: rows x num_classes values, see tahoe_forest_create_multiclass.)
 * preds_dev[rows] <- per-row float32 sum of leaf values in tree order 0..T-1 (the order of
 * predict_on_cpu, BaseTahoeTest.h:462-466), then AVG / bias / sigmoid / threshold as
 * forest::predict + transform_k do (Struct.h:196-209, :263-268).  data_dev is row-major
 * rows x num_cols float32 (data_d of generate_data_from_file, BaseTahoeTest.h:378-392); a batch held as columns (one buffer per
 * column, or one buffer with a column stride) goes to tahoe_forest_predict_columns / tahoe_forest_predict_column_ptrs below, a
 * batch held as CSR to tahoe_forest_predict_csr. */
tahoe_status tahoe_forest_predict(tahoe_forest *f, float *preds_dev, const float *data_dev, size_t rows,
                                  void *stream);

/* tahoe_forest_predict on rows given as CSR, without a dense copy of the batch.  Row r has values_dev[k] in column
 * indices_dev[k] for k in [indptr_dev[r], indptr_dev[r + 1]) and the missing sentinel (params.missing) in every other column:
 * an entry that is not stored is missing and takes the node's default branch, as in XGBoost and LightGBM.  preds_dev gets, bit
 * for bit, what tahoe_forest_predict writes for that dense matrix -- rows values, or rows x num_classes on a multi-class
 * handle, output transform included -- under every strategy setting (every kernel adds a row's leaf values in tree order).
 *   - Stored values are ordinary values: a stored sentinel is missing, a stored NaN goes left (on a handle created with
 *     TAHOE_CREATE_NAN_MISSING it is missing, by the rule stated there), -0.0 stays -0.0.
 *   - Column ids within a row need not be sorted; rows may be empty.  A row must not name a column twice: if it does, one of the
 *     two values is used, which one is unspecified, and nothing else is affected.
 *   - The kernels never read outside [0, nnz) of indices_dev / values_dev nor outside [0, rows] of indptr_dev, whatever
 *     indptr_dev holds: entry ranges are clamped to nnz.  An entry whose column id is outside [0, num_cols) is skipped (its row
 *     reads the sentinel there) and raises a flag of its own in the handle: the next tahoe_forest_check returns
 *     TAHOE_ERR_INVALID_ARG with a text that says "column" and clears that flag, so a later clean call checks TAHOE_OK.
 *   - Served on dense, multi-class, sparse, multi-class sparse and categorical handles, and on oblivious and vector-leaf handles
 *     created with TAHOE_CREATE_CSR (without the flag: TAHOE_ERR_UNSUPPORTED, as stated at their creates; on a handle with
 *     category sets the level rule of tahoe_oblivious_forest_create_cat applies to the densified row).  rows == 0: TAHOE_OK, nothing launched;
 *     nnz == 0 with rows > 0 is valid (every value missing).  NULL preds_dev / indptr_dev with rows > 0, NULL indices_dev /
 *     values_dev with nnz > 0, or nnz > INT64_MAX: TAHOE_ERR_INVALID_ARG, checked before the handle or a device is touched.
 *   - Asynchronous on `stream`.  ROWTILE, and on sparse handles TILEBLOCK, stage their 64-row LDS tile straight from the CSR
 *     arrays (kernel forms TAHOE_FORM_CSR_*; ROWTILE on an oblivious or vector-leaf handle: TAHOE_OBLIVIOUS_FORM_CSR_TILE /
 *     TAHOE_VECTOR_FORM_CSR_TILE); every other kernel form gets the batch densified chunk by chunk into a buffer the
 *     handle owns -- at most TAHOE_CSR_CHUNK_MB MiB (read at create, default 64; at least one 64-row tile), counted in
 *     device_bytes -- and runs on each chunk in turn.  Under AUTO the path is picked from num_cols, the trees and nnz / rows
 *     (tahoe_forest_get_csr_plan tells).  The buffer and the kernels' workspace grow on demand, which allocates and
 *     synchronises; after tahoe_forest_reserve_csr(rows, nnz) a call with at most that many rows and entries allocates nothing
 *     and can be captured.
 * Leaf indices, predict_accumulate, predict_host and the SHAP entry points take dense rows only. */
tahoe_status tahoe_forest_predict_csr(tahoe_forest *f, float *preds_dev, const int64_t *indptr_dev, const int32_t *indices_dev,
                                      const float *values_dev, size_t rows, size_t nnz, void *stream);
tahoe_status tahoe_forest_reserve_csr(tahoe_forest *f, size_t rows, size_t nnz);
/* How tahoe_forest_predict_csr runs a batch of `rows` rows with nnz entries: *chunk_rows = 0 and *form = the fused kernel
 * (TAHOE_FORM_CSR_*), or *chunk_rows = rows per densified chunk and *form = the kernel form that runs on a chunk. */
tahoe_status tahoe_forest_get_csr_plan(const tahoe_forest *f, size_t rows, size_t nnz, int *form, size_t *chunk_rows);

/* tahoe_forest_predict on a column-major batch -- a cuDF / Arrow table (one device buffer per column: _column_ptrs) or a
 * Fortran-ordered array (one buffer with a column stride: _columns) -- without a row-major copy made by the caller.
 *   _columns:      column c of the batch is data_dev[c * col_stride + r], r in [0, rows); col_stride >= rows, in floats
 *   _column_ptrs:  column c of the batch is cols_dev[c][r]; cols_dev is a DEVICE array of num_cols device pointers
 * preds_dev gets, bit for bit, what tahoe_forest_predict writes for the row-major matrix with the same values -- rows values,
 * or rows x num_classes, output transform included -- under every strategy setting and on every handle kind: dense, multi-class,
 * sparse, categorical, oblivious, vector-leaf.  No create flag is needed.
 *   - Values are ordinary values: the sentinel is missing, NaN goes left, -0.0 stays -0.0.  On a handle created with
 *     TAHOE_CREATE_NAN_MISSING a NaN is missing, by the rule stated there.  Arrow validity bitmaps are not read: a column with
 *     nulls must be filled by the caller, with NaN on such a handle, else with the sentinel (NaN then goes left).  float32 only.
 *   - A column pointer needs float alignment only; col_stride is any value >= rows.  Columns may come from separate allocations
 *     in any order, and two entries of the table may name the same buffer.
 *   - No kernel reads outside [0, rows) of any column, nor outside [0, num_cols) of the table.
 *   - NULL handle; NULL preds_dev / data_dev / cols_dev with rows > 0; col_stride < rows: TAHOE_ERR_INVALID_ARG, checked before
 *     the handle or a device is touched.  rows == 0: TAHOE_OK, nothing launched.  A handle with num_cols == 0 or no trees
 *     behaves as tahoe_forest_predict does (no value of the batch is read).
 *   - Asynchronous on `stream`.  Where the handle's strategy for the batch is QRING, the quantise pass reads the columns and the
 *     walk runs as ever (its ordinary kernel form); where it is ROWTILE, or TILEBLOCK on a sparse handle, the kernel stages its
 *     64-row LDS tile from the columns (TAHOE_COLUMNS_FORM_*).  Every other kernel form, and every oblivious or vector-leaf
 *     handle, gets the batch transposed chunk by chunk into the buffer tahoe_forest_predict_csr's fallback also uses -- at most
 *     TAHOE_CSR_CHUNK_MB MiB, counted in device_bytes -- and runs on each chunk in turn.  TAHOE_COLUMNS_FUSED=0 (read at
 *     create) sends AUTO to chunks always.  tahoe_forest_get_columns_plan tells.  The buffer and the kernels' workspace grow on
 *     demand, which allocates and synchronises; after tahoe_forest_reserve_columns(rows) a call of at most that many rows
 *     allocates nothing, leaves device_bytes unchanged and can be captured.
 * Leaf indices, predict_accumulate, predict_host, staged output and the explanation calls keep taking row-major rows. */
tahoe_status tahoe_forest_predict_columns(tahoe_forest *f, float *preds_dev, const float *data_dev, size_t rows, size_t col_stride,
                                          void *stream);
tahoe_status tahoe_forest_predict_column_ptrs(tahoe_forest *f, float *preds_dev, const float *const *cols_dev, size_t rows,
                                              void *stream);
tahoe_status tahoe_forest_reserve_columns(tahoe_forest *f, size_t rows);
/* How the two calls above run a batch of `rows` rows: *chunk_rows = 0 when no row-major copy is made, and *form = the walk's
 * ordinary form (TAHOE_FORM_QRING_*, TAHOE_FORM_SPARSE_QRING: the quantise pass reads the columns) or a TAHOE_COLUMNS_FORM_* (a
 * tile kernel does); else *chunk_rows = rows per transposed chunk and *form = the kernel form that runs on a chunk. */
tahoe_status tahoe_forest_get_columns_plan(const tahoe_forest *f, size_t rows, int *form, size_t *chunk_rows);

/* tahoe_forest_predict on a table of typed, nullable columns -- a cuDF / Arrow table as it is: no float32 copy of an integer or
 * float64 column and no rewrite of a column with nulls is asked of the caller.
 * A column is described in the layout of the Arrow C data interface: a data buffer, an optional validity bitmap, an offset. */
enum {
    TAHOE_COL_FLOAT32 = 0,
    TAHOE_COL_FLOAT64 = 1,
    TAHOE_COL_FLOAT16 = 2,
    TAHOE_COL_INT8 = 3,
    TAHOE_COL_INT16 = 4,
    TAHOE_COL_INT32 = 5,
    TAHOE_COL_INT64 = 6,
    TAHOE_COL_UINT8 = 7,   /* cuDF's bool8 too; Arrow's bit-packed boolean is not served */
    TAHOE_COL_UINT16 = 8,
    TAHOE_COL_UINT32 = 9,
    TAHOE_COL_UINT64 = 10
};
typedef struct tahoe_column {
    const void    *data;      /* device; element i of the column is data[offset + i]; aligned to the element size */
    const uint8_t *validity;  /* device or NULL (no nulls); bit (offset + i), LSB first, 1 = valid: Arrow's and cuDF's bitmap */
    int64_t        offset;    /* >= 0, in elements; applies to data and to validity */
    int32_t        type;      /* TAHOE_COL_* */
    int32_t        reserved;  /* 0 */
} tahoe_column;
typedef struct tahoe_table tahoe_table;  /* opaque: num_cols descriptors on one device */

/* Validates cols_host[0 .. num_cols) on the host -- an unknown type, a NULL data with rows > 0, a negative offset, a data pointer
 * that is not aligned to its element size, a non-zero reserved field (each TAHOE_ERR_INVALID_ARG naming the column's index) and
 * num_cols < 0 are refused before a device is touched -- then copies them to the current device with a synchronous copy and
 * records that device.  The buffers the descriptors name stay the caller's: they must outlive the calls that read them and may be
 * rewritten in place between calls (a captured call replays on the new contents).  tahoe_table_destroy(NULL) is a no-op. */
tahoe_status tahoe_table_create(const tahoe_column *cols_host, int num_cols, size_t rows, tahoe_table **out);
void         tahoe_table_destroy(tahoe_table *t);
/* preds_dev gets, bit for bit, what tahoe_forest_predict writes for the row-major rows x num_cols matrix M, where
 * M[r][c] = params.missing where column c has a validity buffer and bit offset + r is 0, else (float)data[offset + r] with C's
 * conversion: round to nearest even for 64-bit integers and float64, float64 overflow to +-inf, NaN stays NaN, float32
 * subnormal results kept (no flush), float16 and the narrow integers exact, float32 passed through bit for bit.  On every handle
 * kind, under every strategy setting, without a create flag.  Everything else follows from the handle: with
 * TAHOE_CREATE_NAN_MISSING a float64 / float16 NaN is missing, without it a NaN goes left.
 *   - What lies under a null in data is never read.  No byte of validity outside [offset >> 3, (offset + rows - 1) >> 3] and no
 *     element of data outside [offset, offset + rows) is read: no padding is assumed.
 *   - NULL handle, table or preds_dev; a table whose num_cols differs from the handle's; a table on another device than the
 *     handle's: TAHOE_ERR_INVALID_ARG before a device is touched.  A table of 0 rows: TAHOE_OK, nothing launched.
 *   - Asynchronous on `stream`; uploads nothing.  Where the handle's strategy for the batch is QRING (dense, multi-class or
 *     sparse handle), the quantise pass converts and tests the bitmap as it loads and the walk runs as ever (its ordinary kernel
 *     form).  Every other kernel form, and every categorical, oblivious or vector-leaf handle, gets the batch converted chunk by
 *     chunk into the row-major buffer tahoe_forest_predict_csr's fallback also uses -- at most TAHOE_CSR_CHUNK_MB MiB, counted in
 *     device_bytes -- and runs on each chunk in turn.  TAHOE_TABLE_FUSED=0 (read at create) sends AUTO to chunks always.
 *     tahoe_forest_get_table_plan tells, as tahoe_forest_get_columns_plan does: *chunk_rows = 0 and the walk's ordinary form, or
 *     the rows per converted chunk and the form that runs on a chunk.  After tahoe_forest_reserve_table(rows) a call of at most
 *     that many rows allocates nothing, leaves device_bytes unchanged and can be captured.
 * Leaf indices, predict_accumulate, predict_host, staged output and the explanation calls keep taking row-major rows. */
tahoe_status tahoe_forest_predict_table(tahoe_forest *f, float *preds_dev, const tahoe_table *t, void *stream);
tahoe_status tahoe_forest_reserve_table(tahoe_forest *f, size_t rows);
tahoe_status tahoe_forest_get_table_plan(const tahoe_forest *f, size_t rows, int *form, size_t *chunk_rows);

/* Raw float32 per-row sums only (no output transform) -- the quantity tree shards exchange. */
tahoe_status tahoe_forest_predict_raw(tahoe_forest *f, float *sums_dev, const float *data_dev, size_t rows,
                                      void *stream);

/* Chained tree shards ("sum-order caveat"): sums_dev[rows] holds, on entry, the float32 sums of the trees
 * that come BEFORE this forest's trees in the whole ensemble; on return, those sums continued through this forest's
 * trees in tree order.  Shard k called on shard k-1's output therefore reproduces the single sequential float32 sum of
 * predict_on_cpu (BaseTahoeTest.h:462-466) bit for bit, which an all-reduce of per-shard totals cannot.  Every
 * strategy supports it (the kernels start their per-row accumulator from sums_dev[row] instead of 0.0f).
 * TAHOE_ERR_UNSUPPORTED on a multi-class handle. */
tahoe_status tahoe_forest_predict_accumulate(tahoe_forest *f, float *sums_dev, const float *data_dev, size_t rows,
                                             void *stream);

/* Staged prediction: the output after the first n boosting rounds, for many n, in one walk over the forest (XGBoost
 * iteration_range=(0, n), LightGBM num_iteration=n, scikit-learn staged_predict).  Every kernel adds a row's leaf values in tree
 * order from 0.0f, so the running sum after tree n - 1 is, bit for bit, the sum of the forest cut to its first n trees; the
 * staged kernels store it there and go on.
 *
 * tahoe_forest_set_stages: rounds[0 .. num_stages) in host memory, strictly ascending, every value in [1, Tc], Tc = num_trees /
 * C, C = tahoe_forest_num_classes(f) (so num_stages <= Tc).  Stage s is the forest of the caller's trees 0 .. rounds[s] * C - 1:
 * the first rounds[s] trees of every class.  The handle keeps a device copy (num_stages ints, counted in
 * tahoe_forest_info.device_bytes).  Synchronous, and it allocates: not graph-capturable.  A second call replaces the stages;
 * (NULL, 0) clears them.  Refusals, TAHOE_ERR_INVALID_ARG with a text that names the offending index, checked before a device is
 * touched: a NULL handle, num_stages < 0, NULL rounds with num_stages > 0, a value outside [1, Tc], a value not above its
 * predecessor.  On any refusal the previous stages stay.  Served on dense, multi-class, sparse, multi-class sparse and
 * categorical handles, and on oblivious and vector-leaf handles created with TAHOE_CREATE_STAGED (without the flag:
 * TAHOE_ERR_UNSUPPORTED, as stated at their creates).  There every tree feeds every class: Tc = num_trees, C = K = leaf_dim, and
 * stage s is the forest of trees 0 .. rounds[s] - 1; a forest without trees has no valid stage. */
tahoe_status tahoe_forest_set_stages(tahoe_forest *f, const int32_t *rounds, int num_stages);
/* out_dev[(row * S + s) * C + c], S = num_stages <- bit for bit what tahoe_forest_predict writes for that row and class on a
 * handle created with the same parameters from the trees of stage s, output bits included, applied as that handle applies
 * them: AVG divides by (float)rounds[s], global_bias is added, SIGMOID, THRESHOLD, then TAHOE_OUT_SOFTMAX over the C values of
 * one (row, stage).  Asynchronous on `stream`; allocates nothing (graph-capturable after set_stages); deterministic: the same
 * bits for a row in any batch, under every strategy that serves the call.
 * Strategies with a staged form: DIRECT and ROWTILE on dense and multi-class handles; DIRECT, ROWTILE and TILEBLOCK on sparse,
 * multi-class sparse and categorical handles.  A forced strategy of that set is honoured.  Under AUTO a dense handle takes
 * ROWTILE when its tile fits LDS, else DIRECT; a sparse handle TILEBLOCK when available, else ROWTILE, else DIRECT -- whatever
 * AUTO picks for tahoe_forest_predict.  QRING, TILERING and dense TILEBLOCK have no staged form.  An oblivious or vector-leaf
 * handle created with TAHOE_CREATE_STAGED runs DIRECT or ROWTILE, whichever tahoe_forest_predict resolves for its strategy
 * setting (AUTO: ROWTILE when the 256 x num_cols-byte tile fits LDS, else DIRECT); "the same parameters" then means the same create
 * call, parameters and category sets on trees 0 .. rounds[s] - 1, and AVG divides by (float)rounds[s] whatever K is.
 * Refusals, in this order, nothing launched: a NULL handle: TAHOE_ERR_INVALID_ARG; no stages set: TAHOE_ERR_UNSUPPORTED
 * (tahoe_last_error says so); a forced strategy without a staged form: TAHOE_ERR_UNSUPPORTED; then rows == 0: TAHOE_OK; NULL
 * out_dev / data_dev with rows > 0: TAHOE_ERR_INVALID_ARG; rows * S * C * 4 overflowing size_t: TAHOE_ERR_INVALID_ARG.
 * Out of scope, on every handle kind: CSR rows (densify, or use tahoe_forest_predict_csr per truncated handle), a staged
 * tahoe_forest_predict_accumulate, staged leaf indices, and a start round other than 0. */
tahoe_status tahoe_forest_predict_staged(tahoe_forest *f, float *out_dev, const float *data_dev, size_t rows, void *stream);
/* The strategy tahoe_forest_predict_staged runs for `rows` rows (TAHOE_STRATEGY_DIRECT, _ROWTILE or _TILEBLOCK); 0 when the call
 * would be refused (no stages set, or a forced strategy without a staged form); -1 for a NULL handle.  Served on the handles
 * tahoe_forest_set_stages serves; an oblivious or vector-leaf handle gives DIRECT or ROWTILE. */
int tahoe_forest_get_staged_strategy(const tahoe_forest *f, size_t rows);

/* leaf_dev[row * num_trees + tree] <- index of the leaf the row ends in, in the tree's original heap
 * numbering (final `curr` of infer_one_tree, BaseTahoeTest.h:441-455).  sums_dev may be NULL (else rows x num_classes
 * raw sums on a multi-class handle). */
tahoe_status tahoe_forest_predict_leaf_idx(tahoe_forest *f, uint32_t *leaf_dev, float *sums_dev,
                                           const float *data_dev, size_t rows, void *stream);

/* Finishes sums -> preds in place (AVG, bias, sigmoid, threshold); what the ranks of a tree-sharded
 * forest call after the all-reduce.  num_trees_total = trees of the whole forest. */
tahoe_status tahoe_transform_preds(float *preds_dev, size_t rows, int output, int num_trees_total,
                                   float threshold, float global_bias, void *stream);

tahoe_status tahoe_forest_set_strategy(tahoe_forest *f, int strategy);
/* Waits for `stream` and reports TAHOE_ERR_HIP if a kernel flagged an internal error (a bounded
 * LDS wait of TILERING timing out); else TAHOE_ERR_INVALID_ARG, once, if a tahoe_forest_predict_csr since the last check
 * skipped an entry with a column id outside [0, num_cols); TAHOE_OK otherwise. */
tahoe_status tahoe_forest_check(tahoe_forest *f, void *stream);
/* Sizes the handle's device workspace for batches of up to `rows` rows: QRING's 2-byte-per-value quantised copy of
 * the batch and, for the batches small enough to be walked in tree slices (up to 64 rows per CU), one float per
 * (tree of the largest group, row); the row-streaming form of TILERING's leaf-value workspace, 4 bytes x rows x
 * (trees rounded up to 32), at most 1 GiB (TAHOE_WSTREAM_SLAB_MB at create).  Optional: predict grows the
 * workspace on demand, which is the only case in which a predict call allocates (and synchronises the device,
 * so it cannot be captured); after reserve(rows) no batch of up to `rows` rows does. */
tahoe_status tahoe_forest_reserve(tahoe_forest *f, size_t rows);

/* Host-resident batch (the reference uploads the data file once, BaseTahoeTest.h:378-389, and
 * has no per-batch host path; TAHOE_ERR_UNSUPPORTED on a multi-class handle).  Rows are uploaded in chunks of `chunk_rows` rows (0 = about 32 MiB of rows)
 * through two device buffers; the upload of chunk i+1 overlaps the traversal of chunk i and the download of
 * chunk i-1's predictions.  A pinned source (hipHostMalloc / hipHostRegister) is copied from directly,
 * pageable memory is staged through pinned buffers by a few host threads.  Synchronous: preds_host is
 * complete on return.  Results are identical to tahoe_forest_predict on the whole batch (rows are
 * independent).  The buffers and three streams are created on first use and kept by the handle. */
tahoe_status tahoe_forest_predict_host(tahoe_forest *f, float *preds_host, const float *data_host, size_t rows,
                                       size_t chunk_rows);
/* Pinned host memory for the call above (hipHostMalloc / hipHostFree). */
tahoe_status tahoe_host_alloc(void **ptr, size_t bytes);
tahoe_status tahoe_host_free(void *ptr);
/* Strategy the next predict will run (after AUTO resolution for `rows`). */
int tahoe_forest_get_strategy(const tahoe_forest *f, size_t rows);

typedef struct {
    int num_trees, depth, num_cols;
    int bits_bytes;          /* b of the reference's adaptive format rule (Struct.h:1827-1852): 1, 2 or 4 */
    int lds_levels;          /* top levels staged in LDS by ROWTILE */
    size_t device_bytes;     /* device memory owned by the handle */
    int lds_bytes_per_block; /* dynamic LDS of the ROWTILE kernel (0 = does not fit) */
    int device_id;
    int num_cus;
    int top_levels;          /* top levels staged in LDS by TILEBLOCK */
    int tile_rows;           /* rows per TILEBLOCK tile: 128, 64, or 0 = strategy unavailable */
    int tileblock_lds_bytes; /* dynamic LDS of the TILEBLOCK kernel */
    int qring_walkers;       /* walker waves of the QRING kernel; 0 = strategy unavailable */
    int qring_lds_bytes;     /* dynamic LDS of the QRING kernel */
    int qring_groups;        /* tree groups quantised separately (forests with > 32767 thresholds per feature) */
    int is_sparse;           /* 1: handle made by tahoe_sparse_forest_create(_ex) (only the generic fields are set) */
    int ring_rows;           /* rows per TILERING tile: 64 or 128; 32 / 16 / 8 for the wide-row float32 form (num_cols > 512);
                              * 0 = strategy unavailable */
    int tilering_lds_bytes;  /* dynamic LDS of the TILERING kernel the launch takes (of the wide-row form where that runs) */
    int qring_tile_rows;     /* rows per quantised tile in LDS: 384 (8-bit ranks, or <= 128 features), 192 (region form), 128, or
                              * 64 / 32 / 16 for wide rows (several trees per wave); 0 = features read from the quantised tile in
                              * L2, or QRING unavailable.  The large tile of the form: a batch may end in 128-row tiles. */
    int relayout;            /* 1: created with TAHOE_CREATE_PROB_RELAYOUT */
    size_t relayout_swaps;   /* internal nodes whose subtrees changed places */
    int stream_slots;        /* > 0: TILERING runs as the row-streaming kernel on 16-bit keys (picked at create by the shape
                              * rule -- num_cols <= 3072 and a multiple of 4, every level above the last two of all trees
                              * resident, at most a tree per three features, key map fine enough -- or forced with
                              * TAHOE_WSTREAM=1): LDS row slots of the ring the rows stream through */
    int stream_levels;       /* ... and the top levels of ALL trees it keeps resident in LDS */
    float stream_key_ties;   /* create-time estimate of the share of that form's 16-bit key compares that tie and fall back
                              * to the float32 values (one affine key map for all features: small-scale features beside
                              * large-scale ones tie often); the shape rule takes the form only below 1e-4 */
} tahoe_forest_info;
tahoe_status tahoe_forest_get_info(const tahoe_forest *f, tahoe_forest_info *info);

/* Which kernel a predict of `rows` rows launches (one strategy number can stand for several kernels: TILERING is
 * tilering_kernel, widef_kernel or wkey_kernel; QRING has several tile forms).  -1 for a NULL handle.
 * REGION8 / REGION6 name the code layout: whole waves of the batch go through 384-row tiles, a remainder (or a batch too small
 * for one wave of them) through 128-row tiles of the same codes in a second launch, as REGION_MIXED does for 192 + 128. */
enum {
    TAHOE_FORM_NONE = 0,                  /* strategy unavailable for this shape */
    TAHOE_FORM_DIRECT = 1,                /* direct_kernel */
    TAHOE_FORM_ROWTILE = 2,               /* rowtile_kernel */
    TAHOE_FORM_TILEBLOCK = 3,             /* tileblock_kernel */
    TAHOE_FORM_TILERING_TILE = 4,         /* tilering_kernel: 64- / 128-row float32 tile, num_cols <= 512 */
    TAHOE_FORM_TILERING_WIDE_TILE = 5,    /* widef_kernel: 32- / 16- / 8-row float32 tiles of wide rows */
    TAHOE_FORM_TILERING_WIDE_STREAM = 6,  /* wkey_kernel: rows streamed through LDS as 16-bit keys, lane = tree */
    TAHOE_FORM_QRING_REGION3 = 7,         /* qring_kernel, 192-row tiles of three 64-row regions (K3) */
    TAHOE_FORM_QRING_REGION2 = 8,         /* qring_kernel, 128-row tiles of two regions */
    TAHOE_FORM_QRING_REGION_MIXED = 9,    /* whole waves of 192-row tiles + a remainder of 128-row tiles (two launches) */
    TAHOE_FORM_QRING_SPLIT = 10,          /* small batches: tree slices per tile + ordered_sum_kernel */
    TAHOE_FORM_QRING_COLUMNS = 11,        /* qring_kernel on 128-slot columns (general node word, or the exchange-bit layout) */
    TAHOE_FORM_QRING_WIDE = 12,           /* qwide_kernel: 64- / 32- / 16-row tiles, several trees per wave */
    TAHOE_FORM_QRING_GX = 13,             /* qring_kernel reading codes from L2 (rows too wide for any LDS tile) */
    TAHOE_FORM_SPARSE_DIRECT = 14,        /* sparse handle: sparse_kernel without a tile */
    TAHOE_FORM_SPARSE_ROWTILE = 15,       /* sparse_kernel with the 64-row float32 tile */
    TAHOE_FORM_SPARSE_TOP = 16,           /* sparse_top_kernel */
    TAHOE_FORM_SPARSE_QRING = 17,         /* sparse_q_kernel */
    TAHOE_FORM_QRING_REGION8 = 18,        /* qring_kernel on 8-bit rank codes (<= 254 thresholds per feature): 384-row tiles of three
                                             128-row regions, six chains per lane (<= 128 features: 15 walkers, ring of 24) */
    TAHOE_FORM_QRING_REGION6 = 19,        /* qring_kernel on u16 codes, num_cols <= 128: 384-row tiles of six 64-row regions at a
                                             16-KiB stride, six chains per lane */
    TAHOE_FORM_CSR_ROWTILE = 20,          /* tahoe_forest_predict_csr only: rowtile_kernel staging its tile from the CSR arrays */
    TAHOE_FORM_CSR_SPARSE_ROWTILE = 21,   /* ... sparse_kernel with the tile */
    TAHOE_FORM_CSR_SPARSE_TOP = 22        /* ... sparse_top_kernel */
};
/* The kernel forms of an oblivious handle (tahoe_oblivious_forest_create).  They continue the numbering at 24: 23 stays
 * unassigned, because tahoe_kernel_form_name(23) == "?" is behaviour callers of the CSR entry points were promised (the first
 * value past TAHOE_FORM_CSR_SPARSE_TOP has no name). */
enum {
    TAHOE_OBLIVIOUS_FORM_DIRECT = 24,     /* oblivious_direct_kernel: features from global memory */
    TAHOE_OBLIVIOUS_FORM_TILE = 25        /* oblivious_tile_kernel: one wave per 64-row float32 tile */
};
/* The kernel forms of a vector-leaf handle (tahoe_vector_forest_create).  26 stays unassigned for the same reason: the first
 * value past TAHOE_OBLIVIOUS_FORM_TILE has no name (tahoe_kernel_form_name(26) == "?"). */
enum {
    TAHOE_VECTOR_FORM_DIRECT = 27,        /* vector_direct_kernel: features from global memory */
    TAHOE_VECTOR_FORM_TILE = 28           /* vector_tile_kernel: one wave per 64-row float32 tile */
};
/* The fused CSR forms of those two handle kinds (TAHOE_CREATE_CSR).  29 stays unassigned for the same reason: the first value past
 * TAHOE_VECTOR_FORM_TILE has no name (tahoe_kernel_form_name(29) == "?"). */
enum {
    TAHOE_OBLIVIOUS_FORM_CSR_TILE = 30,   /* tahoe_forest_predict_csr only: oblivious_tile_kernel staging its tile from the CSR arrays */
    TAHOE_VECTOR_FORM_CSR_TILE = 31       /* ... vector_tile_kernel */
};
/* The tile kernels fed from column-major batches (tahoe_forest_get_columns_plan only).  32 stays unassigned for the same reason:
 * the first value past TAHOE_VECTOR_FORM_CSR_TILE has no name (tahoe_kernel_form_name(32) == "?"). */
enum {
    TAHOE_COLUMNS_FORM_ROWTILE = 33,         /* rowtile_kernel staging its tile from the columns */
    TAHOE_COLUMNS_FORM_SPARSE_ROWTILE = 34,  /* ... sparse_kernel with the tile */
    TAHOE_COLUMNS_FORM_SPARSE_TOP = 35       /* ... sparse_top_kernel */
};
int tahoe_forest_get_kernel_form(const tahoe_forest *f, size_t rows);
const char *tahoe_kernel_form_name(int form);

/* Kernel timing with hipEvents on the stream the kernel runs on.  set_profiling(f, n) arms up to n
 * launches (0 disarms): each following predict brackets its traversal kernel with an event pair (a pre-pass kernel, if
 * the strategy has one, is timed apart: tahoe_forest_prepass_times).
 * kernel_times waits for the recorded launches and returns their durations in milliseconds. */
tahoe_status tahoe_forest_set_profiling(tahoe_forest *f, int max_launches);
tahoe_status tahoe_forest_kernel_times(tahoe_forest *f, float *ms_out, int capacity, int *count);
/* Durations of the pre-pass kernel of the same launches (QRING's quantise kernel; 0 for the others). */
tahoe_status tahoe_forest_prepass_times(tahoe_forest *f, float *ms_out, int capacity, int *count);

/* ---- file formats (BaseTahoeTest.h:267-402): one value per line ---- */
/* model: num_trees, levels(=depth+1), then per tree, per node in heap order: fid, value,
 * default_left, weight, is_leaf.  *num_trees / *depth are in/out (kept when a header line is
 * missing, as the reference keeps its constructor defaults).  nodes_out: tahoe_free_host. */
tahoe_status tahoe_load_model(const char *path, int *num_trees, int *depth, tahoe_dense_node **nodes_out);
/* data: num_rows, num_cols, missing, then rows*cols values row-major. */
tahoe_status tahoe_load_data(const char *path, int *num_rows, int *num_cols, float *missing, float **data_out);
tahoe_status tahoe_write_model(const char *path, int num_trees, int depth, const tahoe_dense_node *nodes);
tahoe_status tahoe_write_data(const char *path, int num_rows, int num_cols, float missing, const float *data);

/* ---- binary files (no counterpart in the reference, whose text formats cost ~2.5 s for the K3
 * model and ~25 s for the K3 data on one core).  64-byte header + the payload as it sits in memory
 * (dense_node_t AoS / row-major float32) + a checksum; TAHOE_ERR_IO on a foreign, truncated or corrupt file. */
tahoe_status tahoe_save_model_bin(const char *path, int num_trees, int depth, const tahoe_dense_node *nodes);
tahoe_status tahoe_load_model_bin(const char *path, int *num_trees, int *depth, tahoe_dense_node **nodes_out);
tahoe_status tahoe_save_data_bin(const char *path, int num_rows, int num_cols, float missing, const float *data);
tahoe_status tahoe_load_data_bin(const char *path, int *num_rows, int *num_cols, float *missing, float **data_out);
/* Text file with a cache beside it ("<path>.tbin"): used when it records the text file's current size and
 * mtime, else the text is parsed as by tahoe_load_model / tahoe_load_data and the cache rewritten (best
 * effort).  *from_cache (may be NULL) tells which happened.  The BaseTahoeTest mirror uses these when the
 * environment variable TAHOE_BIN_CACHE is set. */
tahoe_status tahoe_load_model_cached(const char *path, int *num_trees, int *depth, tahoe_dense_node **nodes_out,
                                     int *from_cache);
tahoe_status tahoe_load_data_cached(const char *path, int *num_rows, int *num_cols, float *missing, float **data_out,
                                    int *from_cache);
void tahoe_free_host(void *p);

/* ---- deterministic synthetic inputs: SplitMix64, counter-based ---- */
/* Complete trees: levels < depth internal (fid = x mod num_cols, threshold 2u-1, def_left = x&1),
 * bottom level leaves (val 2u-1); internal nodes above the bottom turn into leaves with
 * probability leaf_prob. */
void tahoe_synth_forest(tahoe_dense_node *nodes, int num_trees, int depth, int num_cols, uint64_t seed,
                        float leaf_prob);
/* rows x cols float32 in [-1,1); each value replaced by `missing` with probability missing_prob and
 * by NaN with probability nan_prob.  first_row lets ranks generate disjoint row ranges. */
void tahoe_synth_data(float *out, size_t first_row, size_t rows, int num_cols, uint64_t seed,
                      float missing_prob, float missing, float nan_prob);

/* A second generator, in the style of histogram-trained gradient-boosted models (XGBoost / LightGBM with max_bin <= 255:
 * the model families the reference is run on, run_all_15_examples.sh:51-65): at most max_bins distinct thresholds per
 * feature (bin edges = quantiles of a 4096-value sample of the feature), Zipf-skewed feature usage (exponent zipf_s), every
 * node splits what its ancestors left of the feature's range at a skewed position (unbalanced branches; `weight` = reach
 * probability), early leaves where hardly any row arrives (+ leaf_prob), features on different scales (scale_decades decades
 * of spread) and of four shapes (uniform, exponential, bell, small integer counts with half-integer thresholds).
 * tahoe_synth_data_hist draws rows from the same per-feature distributions (same feature_seed and scale_decades). */
tahoe_status tahoe_synth_forest_hist(tahoe_dense_node *nodes, int num_trees, int depth, int num_cols, uint64_t seed,
                                     uint64_t feature_seed, int max_bins, float zipf_s, float leaf_prob, float scale_decades);
tahoe_status tahoe_synth_data_hist(float *out, size_t first_row, size_t rows, int num_cols, uint64_t seed, uint64_t feature_seed,
                                   float scale_decades, float missing_prob, float missing);

/* ---- thin device helpers so that host code above this ABI needs no HIP headers ---- */
tahoe_status tahoe_device_count(int *count);
tahoe_status tahoe_device_set(int device);
tahoe_status tahoe_device_alloc(void **ptr, size_t bytes, int set_zero);   /* allocate(), cuda_base.h:28-32 */
tahoe_status tahoe_device_free(void *ptr);
tahoe_status tahoe_device_memset(void *ptr_dev, int value, size_t bytes, void *stream);
/* float32 <-> float64 on the device: tree shards that exchange their per-row partial sums by an all-reduce do it
 * on float64 copies (8 bytes per row), so that combining the partials adds no float32 rounding of its own. */
tahoe_status tahoe_widen_f32_to_f64(double *dst_dev, const float *src_dev, size_t n, void *stream);
tahoe_status tahoe_narrow_f64_to_f32(float *dst_dev, const double *src_dev, size_t n, void *stream);
tahoe_status tahoe_copy_to_device(void *dst_dev, const void *src_host, size_t bytes, void *stream);
tahoe_status tahoe_copy_to_host(void *dst_host, const void *src_dev, size_t bytes, void *stream);
tahoe_status tahoe_stream_create(void **stream);
tahoe_status tahoe_stream_destroy(void *stream);
tahoe_status tahoe_stream_synchronize(void *stream);
/* Events and device-to-device copies between GPUs of one process: what a host that chains tree shards over several
 * devices needs (device g waits for device g-1's chunk, copies its running sums over xGMI, continues them). */
tahoe_status tahoe_event_create(void **event);
tahoe_status tahoe_event_destroy(void *event);
tahoe_status tahoe_event_record(void *event, void *stream);
tahoe_status tahoe_stream_wait_event(void *stream, void *event);
tahoe_status tahoe_copy_peer(void *dst_dev, int dst_device, const void *src_dev, int src_device, size_t bytes, void *stream);
tahoe_status tahoe_device_synchronize(void);
tahoe_status tahoe_device_lds_bytes(int *bytes);  /* sharedMemPerBlock analogue, Struct.h:215-220 */
/* compare_GPU, cuda_base.h:98-111: counts i with |a[i]-b[i]| > tol (on the device). */
tahoe_status tahoe_compare_device(const float *a_dev, const float *b_dev, size_t n, float tol,
                                  size_t *num_bad, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* TAHOE_AMD_H */
