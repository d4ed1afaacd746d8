// What the lane-per-path-element TreeSHAP kernels share: the scalar-leaf kernels (contribs.hip, interventional.hip) and their
// vector-leaf twins (vector_shap.hip, vector_inter.hip, vector_iv.hip).  The association order of every floating-point statement
// is pinned bit for bit by the tests; the units are built with -ffp-contract=off and nothing here fuses.
//
// Who depends on what:
//   c_inv, from_left_lane, lane_read(_u),        contribs_tile, interaction_bins (contribs.hip), vector_contribs_tile,
//   unwind_split, vm_drain                       vector_interaction_bins; lane_read also the interventional kernels
//   background_weight_sum                        interventional_kernel, vector_interventional_kernel
//   load_leaf_block, add_leaf_block              vector_interaction_bins, vector_interventional_kernel
//
// Not shared, on measurement (MI355X; parent and branch builds in turn, five runs each, medians of 3 calls; a line fails where
// the branch's median exceeds the parent's by more than the spread of the parent's five medians): these bodies stay written out
// where they were, and a fix to one copy has to be made in the other.
//   - The extend recursion and two-ended unwound sum of contribs_tile / vector_contribs_tile.  As one function it changed only
//     compare, select and move instructions (862 -> 861 in contribs_kernel<false>, one VGPR fewer), yet contribs_kernel<false>
//     took 1035.3 against 1032.0 ms on K1 (spread 1.7) and vector_contribs_kernel<1> 419.4 against 417.7 ms (spread 0.3).
//   - The pair key and rounds of interaction_bins / vector_interaction_bins.  As one function: interactions_kernel in place
//     1016.2 against 992.4 ms (30 x 12 trees on 256 columns, spread 0.8) and 11455 against 10901 ms with category sets (spread
//     15), vector_interactions_kernel<1, true> 580.7 against 556.7 ms (spread 1.5).
//   - The extend recursion and one-sided unwound sum on the path without the conditioning element, same two functions.  As one
//     function it cost every interactions_kernel a VGPR (48 -> 49, 57 -> 58) and moved the unwound loop's counter and exit test
//     from the scalar to the vector unit; one pair of runs with it and the rounds shared: 1032.4 against 991.9 ms and 11378
//     against 10867 ms on the two workloads above, 679.7 against 662.4 ms for vector_interactions_kernel<1, false>.
//   - The leaf-block load and add of vector_contribs_tile, which the other two vector-leaf kernels take from here.  With the two
//     helpers vector_contribs_kernel<8> and <4> were faster (75.4 against 81.9 ms), but <1> took 419.6 against 417.8 ms (spread
//     0.5): vector_shap.hip keeps its own statements and its kernels are the parent's instruction for instruction.
// Internal: not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "contribs_internal.h"

namespace tahoe {

// 1 / k (TAHOE_CONTRIB_INV_TABLE), one table per including unit
[[maybe_unused]] static __constant__ float c_inv[34] = TAHOE_CONTRIB_INV_TABLE;

// value of lane - 1 (0 in lane 0): DPP wave_shr:1
__device__ __forceinline__ float from_left_lane(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
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

// the wave's stores have landed: between dependent read-modify-writes of one wave on the output (the in-place forms)
__device__ __forceinline__ void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Where the unwound sum of a followed element (one fraction 1, zero fraction z) of a path of ud + 1 elements changes direction.
// The weights q_i of the path without the element satisfy pw_i = q_i z (ud - i) / (ud + 1) + q_(i-1) i / (ud + 1).  Solved from
// the top (q_(ud-1) first) an error grows by z (ud - i) / (i + 1) per step, from the bottom (q_0 first) by i / (z (ud - i)):
// either alone loses 5 to 6 digits on a 32-element path whose z is near 1.  Both factors stay <= 1 when the top-down recurrence
// runs for i >= split and the bottom-up one for i < split, split = floor((z ud - 1) / (1 + z)) + 1 clamped to [0, ud].  z < 1 / ud
// (a cut z = 0 among them) gives 0: all from the top, and no division by a small z.
__device__ __forceinline__ int unwind_split(float z, int ud)
{
    const float s = floorf((z * (float)ud - 1.0f) / (1.0f + z)) + 1.0f;
    return (int)fminf(fmaxf(s, 0.0f), (float)ud);
}

// Interventional TreeSHAP: the sum, in background order, of this lane's weights over the B background rows of its bin (mb: the
// bin's stored ballots), for a row whose one-fraction on this lane is o (0 on a rank-0 lane).  pm = the lanes of the lane's path
// but its root, w = the 32 x 32 weight table.
__device__ __forceinline__ float background_weight_sum(bool o, unsigned long long pm, const unsigned long long *mb, int B,
                                                       const float *w, int lane)
{
    const unsigned long long mx = __ballot(o);
    const unsigned long long pa = pm & mx, pb = pm & ~mx;
    const int nb = __popcll(pb);
    // A lane that x follows is in A when r does not (weight W[a][b]), one that x does not follow is in B when r
    // does (W[b][a]): the sign is fixed for the row and applied after the sum
    const int sha = o ? 7 : 2, shb = o ? 2 : 7;  // byte offset of W[p][q]: (p << 7) + (q << 2)
    const char *wb = reinterpret_cast<const char *>(w);
    // this lane's weight for background row k, 0 where its element is in neither A nor B or the path is dead
    auto weight = [&](int k) {
        const unsigned long long d = mx ^ mb[k];
        const int na = __popcll(d & pa), nd = __popcll(d & pb);
        const bool active = nd == nb && ((d >> lane) & 1ull) != 0;
        const float wv = *reinterpret_cast<const float *>(wb + ((na << sha) + (nd << shb)));
        return active ? wv : 0.0f;
    };
    float acc = 0.0f;
    int k = 0;
    for (; k + kIvUnroll <= B; k += kIvUnroll) {  // the loads of kIvUnroll rows in flight together; adds in order
        float wk[kIvUnroll];
#pragma unroll
        for (int u = 0; u < kIvUnroll; ++u) wk[u] = weight(k + u);
#pragma unroll
        for (int u = 0; u < kIvUnroll; ++u) acc += wk[u];
    }
    for (; k < B; ++k) acc += weight(k);
    return acc;
}

// The leaf values of classes k0 .. k0 + nk - 1 of this lane's path (vector-leaf handles): a root lane reads them (vec = its .x,
// the index of the leaf's vector; a padding lane names vector 0, which exists where a bin does), the other lanes of the path take
// them from it
template <int KB>
__device__ __forceinline__ void load_leaf_block(float (&leaf)[KB], const float *__restrict__ leaves, uint32_t vec, int K, int k0,
                                                int nk, int rank, int gs)
{
#pragma unroll
    for (int j = 0; j < KB; ++j) {
        float own = 0.0f;
        if (rank == 0 && j < nk) own = leaves[(size_t)vec * (size_t)K + (size_t)(k0 + j)];
        leaf[j] = lane_read(own, gs);
    }
}

// cell[j stride] += term(j) for the nk classes of a block, every read before the first write.  term(j) spells the class's term
// at the call, so its association is visible there: tw * leaf[j], or tw * leaf[j] * h left to right (the interaction term)
template <int KB, class Term>
__device__ __forceinline__ void add_leaf_block(float *cell, size_t stride, int nk, Term term)
{
    float v[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j)
        if (j < nk) v[j] = cell[j * stride];
#pragma unroll
    for (int j = 0; j < KB; ++j)
        if (j < nk) cell[j * stride] = v[j] + term(j);
}

}  // namespace tahoe
