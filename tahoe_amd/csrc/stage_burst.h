// Global memory -> LDS staging of a workgroup's prologue (a walk tile, a quantiser's tables) as ONE burst of loads: every
// lane issues all of its 16-byte loads back to back and only then commits them to LDS, so the prologue costs one memory
// round trip plus the transfer instead of one round trip per piece (profiles/stage_burst/prologue_waits.txt).
//
// How it has to be written for hipcc to keep the burst.  "All loads into registers, then stores guarded by `if (e < n16)`"
// compiles back to load -> s_waitcnt vmcnt(0) -> store per piece: each load is sunk into the branch of its only user.  So
// nothing here stands under a per-lane branch.  A lane whose piece index lies past the end takes another piece instead
// (its index wrapped into the largest power of two that fits, so that the lanes of a wave still hit different addresses:
// no LDS write conflicts, coalesced loads) and rewrites it with that piece's own bytes.  The global side is never read
// past the end; LDS is never written past the end either.
//
// Two levels: stage_issue / stage_commit on a set of registers, for callers that put several copies (the regions of a walk
// tile) and loads of their own (a walker's first top) into one burst; stage_copy for a whole image.
#ifndef TAHOE_AMD_STAGE_BURST_H
#define TAHOE_AMD_STAGE_BURST_H

#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

namespace tahoe {

template <int V>
using StageCount = std::integral_constant<int, V>;

// mask that wraps a piece index into [0, 2^floor(log2 n16)) (n16 >= 1; uniform: scalar instructions)
__device__ __forceinline__ uint32_t stage_wrap(uint32_t n16) { return (1u << (31 - __builtin_clz(n16))) - 1u; }

// the p-th piece of thread tid among n16 pieces dealt round-robin to NT threads
template <int NT>
__device__ __forceinline__ uint32_t stage_piece(int p, int tid, uint32_t n16, uint32_t wrap)
{
    const uint32_t e = (uint32_t)(tid + p * NT);
    return e < n16 ? e : e & wrap;  // a select, not a branch
}

// A 16-byte piece as a native vector: assigning HIP's uint4 (a struct) through pointers is a memcpy to the optimiser, and a
// memcpy global -> register variable -> LDS leaves the variable in scratch.
typedef uint32_t stage_v4 __attribute__((ext_vector_type(4)));

// N pieces in registers: a recursive struct with compile-time access only (an indexed array may go to scratch)
template <int N>
struct StageRegs {
    stage_v4 r;
    StageRegs<N - 1> rest;
};
template <>
struct StageRegs<0> {};

// Loads this thread's P pieces of each of C copies, src[c * src_stride + (0 .. n16)), into v.  Requires 1 <= n16 <= P * NT.
template <int NT, int P, int C = 1, int I = 0>
__device__ __forceinline__ void stage_issue(StageRegs<C * P - I> &v, const uint4 *__restrict__ src, size_t src_stride, int tid, uint32_t n16,
                                            uint32_t wrap)
{
    if constexpr (I < C * P) {
        v.r = reinterpret_cast<const stage_v4 *>(src)[(size_t)(I / P) * src_stride + stage_piece<NT>(I % P, tid, n16, wrap)];
        stage_issue<NT, P, C, I + 1>(v.rest, src, src_stride, tid, n16, wrap);
    }
}

// ... and writes them to the same pieces of dst[c * dst_stride + (0 .. n16)) (LDS).
template <int NT, int P, int C = 1, int I = 0>
__device__ __forceinline__ void stage_commit(const StageRegs<C * P - I> &v, uint4 *dst, size_t dst_stride, int tid, uint32_t n16, uint32_t wrap)
{
    if constexpr (I < C * P) {
        reinterpret_cast<stage_v4 *>(dst)[(size_t)(I / P) * dst_stride + stage_piece<NT>(I % P, tid, n16, wrap)] = v.r;
        stage_commit<NT, P, C, I + 1>(v.rest, dst, dst_stride, tid, n16, wrap);
    }
}

// Calls fn(StageCount<P>) with the pieces per thread as a compile-time count: P = 1, about PMAX / 3, or PMAX, the smallest that
// covers np (np is uniform, so this is a scalar branch around whole bursts -- loads and their stores stay in one block; a
// burst with more pieces than needed re-stages some, see above).  Three steps, not one per count: each is a copy of the caller's
// whole prologue.
template <int PMAX, class Fn>
__device__ __forceinline__ void stage_dispatch(int np, Fn &&fn)
{
    constexpr int PMID = (PMAX + 2) / 3;
    if (PMAX == 1 || np <= 1)
        fn(StageCount<1>{});
    else if (PMID > 1 && np <= PMID)
        fn(StageCount<(PMID > 1 ? PMID : 1)>{});
    else
        fn(StageCount<PMAX>{});
}

// Copies `bytes` (a multiple of 16, at most PMAX * NT * 16; src and dst 16-byte aligned) from global memory to LDS with the NT
// threads of the workgroup as ONE burst.  The caller synchronises (a barrier) before other threads read dst.
template <int NT, int PMAX>
__device__ __forceinline__ void stage_copy_once(const void *__restrict__ src, void *dst, size_t bytes, int tid)
{
    const uint4 *s = reinterpret_cast<const uint4 *>(src);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    const uint32_t n16 = (uint32_t)(bytes >> 4);
    if (n16 == 0) return;
    const uint32_t wrap = stage_wrap(n16);
    stage_dispatch<PMAX>((int)((n16 + NT - 1) / NT), [&](auto p_tag) __attribute__((always_inline)) {
        constexpr int P = decltype(p_tag)::value;
        StageRegs<P> v;
        stage_issue<NT, P>(v, s, 0, tid, n16, wrap);
        stage_commit<NT, P>(v, d, 0, tid, n16, wrap);
    });
}

// The same for any size: whole bursts of PMAX loads per lane, then the rest as one burst.
template <int NT, int PMAX>
__device__ __forceinline__ void stage_copy(const void *__restrict__ src, void *dst, size_t bytes, int tid)
{
    const unsigned char *s = reinterpret_cast<const unsigned char *>(src);
    unsigned char *d = reinterpret_cast<unsigned char *>(dst);
    constexpr size_t WHOLE = (size_t)PMAX * NT * 16;
    while (bytes > WHOLE) {  // every index is in range
        StageRegs<PMAX> v;
        stage_issue<NT, PMAX>(v, reinterpret_cast<const uint4 *>(s), 0, tid, (uint32_t)(PMAX * NT), 0u);
        stage_commit<NT, PMAX>(v, reinterpret_cast<uint4 *>(d), 0, tid, (uint32_t)(PMAX * NT), 0u);
        s += WHOLE;
        d += WHOLE;
        bytes -= WHOLE;
    }
    stage_copy_once<NT, PMAX>(s, d, bytes, tid);
}

}  // namespace tahoe

#endif  // TAHOE_AMD_STAGE_BURST_H
