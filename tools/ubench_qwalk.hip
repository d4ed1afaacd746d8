// Micro-benchmark of the LDS-resident part of the QRING walk on gfx950 (tahoe_amd/csrc/qring.hip): a u16 code tile
// [256 cols][64*K rows] and one 10-level quantised top (4 KiB, u32 nodes, child pairs by ds_read_b64) per walker wave
// in LDS; every wave repeats the 10-level walk with K independent 64-row chains.  No global-memory traffic in the
// loop: prices the walk proper as a function of walker waves, chains per lane and loop form, and separates the LDS
// and VALU ceilings (MODE 1: the LDS reads only, MODE 2: the VALU only).  --top-forms: the same loop by how the top is held
// (u32 nodes, two 3-KiB forms in LDS, a packed top expanded at the commit; profiles/top24/ubench_levels.txt).
// Build: hipcc --offload-arch=gfx950 -O3 -o tools/ubench_qwalk tools/ubench_qwalk.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define CHECK(x)                                                                         \
    do {                                                                                 \
        hipError_t e = (x);                                                              \
        if (e != hipSuccess) {                                                           \
            printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

constexpr int LEVELS = 10;
constexpr int COLS = 256;
typedef const uint16_t __attribute__((address_space(3))) *lds_u16_ptr;
typedef const uint64_t __attribute__((address_space(3))) *lds_u64_ptr;

__device__ __forceinline__ uint32_t descend(uint32_t i, uint64_t m)
{
    uint32_t r;
    uint64_t co;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=&s"(co) : "v"(i), "s"(m));
    return r;
}

// Column stride 256 B (128-row regions): node = code << 16 | fid << 8, address = bfi(0xFF00, node, pos).
// Column stride 128 B (64-row regions, one region per chain): node = code << 16 | fid << 7, address = bfi(0x7F80, node, pos)
// with the region's base folded into pos.  COLB = 0: general form, 2 VALU (bfe + mad) with 384-byte columns.
template <int COLB>
__device__ __forceinline__ uint32_t xaddr(uint32_t node, uint32_t posb)
{
    uint32_t a;
    if (COLB == 256) {
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(a) : "s"(0xFF00u), "v"(node), "v"(posb));
    } else if (COLB == 128) {
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(a) : "s"(0x7F80u), "v"(node), "v"(posb));
    } else {
        asm("v_bfe_u32 %0, %1, 8, 8\n\tv_mad_u32_u24 %0, %0, %3, %2" : "=&v"(a) : "v"(node), "v"(posb), "s"(384u));
    }
    return a;
}

// TOP (DEP, COLB = 128 only): how the top lies in its 4-KiB slot.
//   0  u32 nodes, code << 16 | fid << 7 (what the product stages): v_bfi, cmp (SDWA WORD_1), addc, lshl_add + 2 LDS.
//   1  byte-packed, 3 B per node: node i (1-based) = bytes 3i .. 3i+2 = fid | code_lo | code_hi, read with ONE dword read at byte
//      3i - 1 (code in bits 31:16 as in form 0, fid in bits 15:8, the low byte is the previous node's): bfe, lshl_add, cmp, addc,
//      mad_u24 + 2 LDS.  Three of four of those reads straddle two LDS dwords.
//   2  two arrays, code[1024] u16 at the slot's start and fid[1024] u8 at byte 2048: lshl_add, cmp, addc, lshl_add, add + 3 LDS
//      (aligned reads).
//   3  form 0 whose slot every iteration rewrites from 16 dwords the lane holds (4 ds_write_b128): the commit of a prefetched top
//      as the product does it once per tree; the base line of form 4.
//   4  form 3 with the top held PACKED in 12 dwords per lane (what three 16-byte loads of a 3-KiB top in global memory bring) and
//      expanded to u32 node words on the way to the slot: per four nodes A = code0 << 16 | code1, B = code2 << 16 | code3 and C =
//      the four fids, placed so that ONE v_perm_b32 per node puts a fid into bits 14:7 under its code (bits 15 and 6:0 of a node
//      word are then arbitrary; the level loop reads neither): 16 v_perm + 4 ds_write_b128 per iteration, the level loop is form 0's.
// Forms 1, 2 and 4 hold a 10-level top in 3 KiB.  All walk the same tops to the same leaves (the host compares the sums).
typedef uint32_t __attribute__((aligned(1))) u32_a1;

template <int NW, int K, int MODE, bool UNROLL, int COLB, bool DEP, int TOP = 0>
__global__ void __launch_bounds__(NW * 64) qwalk(const uint16_t *__restrict__ tile_src, const uint32_t *__restrict__ top_src, int iters,
                                                 uint32_t *__restrict__ out)
{
    constexpr int TILEB = COLS * 128 * K;  // tile bytes: 64 * K rows of u16 per column
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *tile = reinterpret_cast<uint16_t *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int e = tid; e < TILEB / 2; e += NW * 64) tile[e] = tile_src[e % (COLS * 128)];
    uint32_t *slot = reinterpret_cast<uint32_t *>(smem + TILEB + wave * 4096);
    const uint32_t *src = top_src + (size_t)((blockIdx.x * NW + wave) % 64) * 1024;
    static_assert(TOP == 0 || (DEP && COLB == 128), "packed tops: the chosen-child form on 64-row regions");
    static_assert(TOP >= 0 && TOP <= 4, "top form");
    for (int i = lane; i < 1024; i += 64) {
        const uint32_t n = src[i];
        if (TOP == 0 || TOP >= 3) {
            slot[i] = n;
        } else if (TOP == 1) {
            unsigned char *b = reinterpret_cast<unsigned char *>(slot) + 3 * i;
            b[0] = (unsigned char)(n >> 7);
            b[1] = (unsigned char)(n >> 16);
            b[2] = (unsigned char)(n >> 24);
        } else {
            reinterpret_cast<uint16_t *>(slot)[i] = (uint16_t)(n >> 16);
            reinterpret_cast<unsigned char *>(slot)[2048 + i] = (unsigned char)(n >> 7);
        }
    }
    __syncthreads();
    const uint32_t slot_a = (uint32_t)reinterpret_cast<uintptr_t>(slot);
    uint32_t pos[K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        pos[k] = COLB == 128 ? (uint32_t)(k * COLS * 128) + (uint32_t)(((lane & 31) << 2) | ((lane >> 5) << 1))
                         : 2u * (uint32_t)(k * 64 + lane);
    uint32_t acc = 0;
    if (TOP == 1 || TOP == 2) {  // (the same data-dependent start as form 0: bits 14:8 of its node word are bits 7:1 of the fid)
        typedef const u32_a1 __attribute__((address_space(3))) *lds_u32a1_ptr;
        typedef const unsigned char __attribute__((address_space(3))) *lds_u8_ptr;
        const uint32_t slot_m1 = slot_a - 1u;
        for (int it = 0; it < iters; ++it) {
            uint32_t i[K], node[K], fid[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                i[k] = 1;
                if (TOP == 1) {
                    node[k] = *reinterpret_cast<lds_u32a1_ptr>(slot_m1 + 3u) ^ ((acc & 0x7fu) << 9);
                } else {
                    node[k] = *reinterpret_cast<lds_u16_ptr>(slot_a + 2u);
                    fid[k] = *reinterpret_cast<lds_u8_ptr>(slot_a + 2048u + 1u) ^ ((acc & 0x7fu) << 1);
                }
            }
            auto xa = [&](int k) {
                uint32_t a;
                if (TOP == 1)
                    asm("v_bfe_u32 %0, %1, 8, 8\n\tv_lshl_add_u32 %0, %0, 7, %2" : "=&v"(a) : "v"(node[k]), "v"(pos[k]));
                else
                    asm("v_lshl_add_u32 %0, %1, 7, %2" : "=v"(a) : "v"(fid[k]), "v"(pos[k]));
                return a;
            };
            auto right = [&](int k, uint32_t xc) { return __builtin_amdgcn_uicmp(xc, TOP == 1 ? node[k] >> 16 : node[k], 35); };
            auto level = [&]() {
                uint32_t xc[K];
#pragma unroll
                for (int k = 0; k < K; ++k) xc[k] = *reinterpret_cast<lds_u16_ptr>(xa(k));
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    i[k] = descend(i[k], right(k, xc[k]));
                    if (TOP == 1) {
                        uint32_t a;
                        asm("v_mad_u32_u24 %0, %1, 3, %2" : "=v"(a) : "v"(i[k]), "v"(slot_m1));
                        node[k] = *reinterpret_cast<lds_u32a1_ptr>(a);
                    } else {
                        node[k] = *reinterpret_cast<lds_u16_ptr>(slot_a + 2u * i[k]);
                        fid[k] = *reinterpret_cast<lds_u8_ptr>(slot_a + 2048u + i[k]);
                    }
                }
            };
            if (UNROLL) {
#pragma unroll
                for (int l = 0; l < LEVELS - 1; ++l) level();
            } else {
#pragma unroll 1
                for (int l = 0; l < LEVELS - 1; ++l) level();
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                i[k] = descend(i[k], right(k, *reinterpret_cast<lds_u16_ptr>(xa(k))));
                acc += i[k];
            }
        }
        out[(size_t)blockIdx.x * NW * 64 + tid] = acc;
        return;
    }
    uint32_t held[16] = {};  // forms 3 and 4: this lane's 16 nodes (groups of four at slot words 4 * (64 c + lane)), form 4: packed into 12
    if (TOP >= 3) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t n[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) n[j] = slot[4 * (64 * c + lane) + j];
            if (TOP == 3) {
#pragma unroll
                for (int j = 0; j < 4; ++j) held[4 * c + j] = n[j];
            } else {
                const uint32_t f2 = (n[2] >> 7) & 0xffu, f3 = (n[3] >> 7) & 0xffu;
                held[3 * c + 0] = (n[0] & 0xffff0000u) | (n[1] >> 16);
                held[3 * c + 1] = (n[2] & 0xffff0000u) | (n[3] >> 16);
                held[3 * c + 2] = (n[0] & 0x7f80u) | ((n[1] & 0x7f80u) << 16) | (f2 >> 1) | ((f2 & 1u) << 15) | ((f3 >> 1) << 16) | ((f3 & 1u) << 31);
            }
        }
    }
    for (int it = 0; it < iters; ++it) {
        uint32_t i[K], node[K];
        if (TOP >= 3) {  // the commit (the registers are made opaque: the expansion is paid every iteration, as per tree)
#pragma unroll
            for (int q = 0; q < (TOP == 3 ? 16 : 12); ++q) asm volatile("" : "+v"(held[q]));
            uint4 *s4 = reinterpret_cast<uint4 *>(slot);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (TOP == 3) {
                    s4[64 * c + lane] = make_uint4(held[4 * c], held[4 * c + 1], held[4 * c + 2], held[4 * c + 3]);
                } else {
                    const uint32_t a = held[3 * c], b = held[3 * c + 1], f = held[3 * c + 2];
                    s4[64 * c + lane] = make_uint4(__builtin_amdgcn_perm(a, f, 0x07060100u), __builtin_amdgcn_perm(a, f, 0x05040302u),
                                                   __builtin_amdgcn_perm(b, f, 0x07060001u), __builtin_amdgcn_perm(b, f, 0x05040203u));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            i[k] = 1;
            node[k] = slot[1] ^ ((acc & 0xffu) << 8);  // data-dependent start: the iterations stay ordered
        }
        auto level_dep = [&]() {  // read only the chosen child, after the compare: 4 VALU + 2 LDS, two round trips
            uint32_t xc[K];
#pragma unroll
            for (int k = 0; k < K; ++k) xc[k] = *reinterpret_cast<lds_u16_ptr>(xaddr<COLB>(node[k], pos[k]));
#pragma unroll
            for (int k = 0; k < K; ++k) {
                i[k] = descend(i[k], __builtin_amdgcn_uicmp(xc[k], node[k] >> 16, 35));
                node[k] = *reinterpret_cast<const uint32_t __attribute__((address_space(3))) *>(slot_a + 4u * i[k]);
            }
        };
        auto level = [&]() {
            if (DEP) {
                level_dep();
                return;
            }
            uint32_t xc[K];
            uint2 pr[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t xa = xaddr<COLB>(node[k], pos[k]);
                const uint32_t pa = slot_a + 8u * i[k];
                if (MODE != 2) {
                    xc[k] = *reinterpret_cast<lds_u16_ptr>(xa);
                    {
                        const uint64_t w = *reinterpret_cast<lds_u64_ptr>(pa);
                        pr[k] = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
                    }
                } else {
                    xc[k] = xa >> 3;
                    pr[k] = make_uint2(pa * 0x9E3779B1u, xa * 0x85EBCA6Bu);
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (MODE == 1) {  // LDS only: the next addresses do not depend on a compare
                    i[k] = ((i[k] * 2u) | (xc[k] & 1u)) & 511u;
                    node[k] = pr[k].x;
                } else {
                    const uint64_t cm = __builtin_amdgcn_uicmp(xc[k], node[k] >> 16, 35);
                    i[k] = descend(i[k], cm);
                    node[k] = __builtin_amdgcn_inverse_ballot_w64(cm) ? pr[k].y : pr[k].x;
                }
            }
        };
        if (UNROLL) {
#pragma unroll
            for (int l = 0; l < LEVELS - 1; ++l) level();
        } else {
#pragma unroll 1
            for (int l = 0; l < LEVELS - 1; ++l) level();
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t xcl = (MODE != 2) ? (uint32_t)*reinterpret_cast<lds_u16_ptr>(xaddr<COLB>(node[k], pos[k])) : node[k] >> 5;
            i[k] = descend(i[k], __builtin_amdgcn_uicmp(xcl, node[k] >> 16, 35));
            acc += i[k];
        }
    }
    out[(size_t)blockIdx.x * NW * 64 + tid] = acc;
}

template <int NW, int K, int MODE, bool UNROLL, int COLB = (K == 2 ? 256 : 0), bool DEP = false>
static void run(const uint16_t *tile, const uint32_t *tops, uint32_t *out)
{
    const int lds = COLS * 128 * K + NW * 4096;
    if (lds > 160 * 1024) {
        printf("NW %2d K %d: %d B of LDS do not fit\n", NW, K, lds);
        return;
    }
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&qwalk<NW, K, MODE, UNROLL, COLB, DEP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const int iters = 600 / K;
    float ms = 0;
    for (int rep = 0; rep < 2; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL((qwalk<NW, K, MODE, UNROLL, COLB, DEP>), dim3(256), dim3(NW * 64), lds, 0, tile, tops, iters, out);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
    }
    const double wave_levels_per_cu = (double)NW * iters * K * LEVELS;
    const double clk = ms * 1e-3 * 2.4e9 / wave_levels_per_cu;
    printf("NW %2d K %d colb %3d %s mode %s %s : %7.3f ms  %5.2f clk per wave-level per CU  (K3 walk of 12 levels at this rate: %.2f ms)\n", NW, K, COLB,
           DEP ? "dep " : "pair", MODE == 0 ? "full" : MODE == 1 ? "lds " : "valu", UNROLL ? "unrolled" : "loop    ", ms, clk, clk * 1.875e8 / 256 / 2.4e9 * 1e3);
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
}

// --kernel-shape: only the shape the product's K3 walk runs (14 walker waves x 3 chains on 64-row regions, child pairs,
// unrolled), best of 5 launches, as one JSON line: bench.py runs this as a child process for roofline.physical.walk.lds_walk_ceiling.
template <int NW, int K, bool DEP, bool UNROLL = true, int TOP = 0>
static float best_ms(const uint16_t *tile, const uint32_t *tops, uint32_t *out, int cus, int iters)
{
    const int lds = COLS * 128 * K + NW * 4096;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&qwalk<NW, K, 0, UNROLL, 128, DEP, TOP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    float best = 1e30f;
    for (int rep = 0; rep < 6; ++rep) {
        float ms = 0;
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL((qwalk<NW, K, 0, UNROLL, 128, DEP, TOP>), dim3(cus), dim3(NW * 64), lds, 0, tile, tops, iters, out);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0 && ms < best) best = ms;
    }
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    return best;
}
// Both forms of the level (both children beside the feature read: 5 VALU + 2 LDS; only the chosen child after the compare: 4 + 2);
// the ceiling is the faster one.
template <int NW, int K>
static void run_json(const uint16_t *tile, const uint32_t *tops, uint32_t *out)
{
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount < 256 ? prop.multiProcessorCount : 256;  // (the output buffer holds 256 workgroups)
    const int iters = 2400 / K;
    const float pair = best_ms<NW, K, false>(tile, tops, out, cus, iters), dep = best_ms<NW, K, true>(tile, tops, out, cus, iters);
    const float best = pair < dep ? pair : dep;
    const double wave_levels_per_cu = (double)NW * iters * K * LEVELS;  // one workgroup per CU
    printf("{\"nw\": %d, \"k\": %d, \"cus\": %d, \"ms\": %.4f, \"ms_pair_reads\": %.4f, \"ms_chosen_child\": %.4f, \"wave_levels_per_cu\": %.0f, "
           "\"ns_per_wave_level_per_cu\": %.5f, \"clock_mhz\": %d}\n", NW, K, cus, best, pair, dep, wave_levels_per_cu,
           best * 1e6 / wave_levels_per_cu, prop.clockRate / 1000);
}

// --top-forms: the level loop in the product's K3 shape (14 walker waves x 3 chains, 64-row regions) for the four ways to hold and
// read a top -- child pairs and the chosen child on u32 nodes, the byte-packed and the two-array 3-KiB tops -- as the loop the
// kernel runs (levels not unrolled: top_levels is a run-time value) and unrolled.  Best of 5 launches; `sum` is the sum of all
// lanes' leaf positions, equal for forms that walked the same paths (the pair form perturbs its start differently: not compared).
template <int NW, int K, bool DEP, bool UNROLL, int TOP>
static void run_top(const char *name, const uint16_t *tile, const uint32_t *tops, uint32_t *out, int cus)
{
    const int iters = 2400 / K;
    const float ms = best_ms<NW, K, DEP, UNROLL, TOP>(tile, tops, out, cus, iters);
    std::vector<uint32_t> h((size_t)cus * NW * 64);
    CHECK(hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost));
    uint64_t sum = 0;
    for (uint32_t v : h) sum += v;
    const double wave_levels_per_cu = (double)NW * iters * K * LEVELS;
    printf("NW %2d K %d %-34s %s : %7.3f ms  %6.3f clk per wave-level per CU at 2.4 GHz  sum %016llx\n", NW, K, name,
           UNROLL ? "unrolled" : "loop    ", ms, ms * 1e-3 * 2.4e9 / wave_levels_per_cu, (unsigned long long)sum);
}
template <int NW, int K>
static void run_top_forms(const uint16_t *tile, const uint32_t *tops, uint32_t *out)
{
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount < 256 ? prop.multiProcessorCount : 256;
    printf("%d CUs, clock %d MHz\n", cus, prop.clockRate / 1000);
    run_top<NW, K, false, false, 0>("u32 nodes, child pairs (5+2)", tile, tops, out, cus);
    run_top<NW, K, true, false, 0>("u32 nodes, chosen child (4+2)", tile, tops, out, cus);
    run_top<NW, K, true, false, 1>("3-B nodes, straddling dword (5+2)", tile, tops, out, cus);
    run_top<NW, K, true, false, 2>("u16 code + u8 fid arrays (5+3)", tile, tops, out, cus);
    run_top<NW, K, true, false, 3>("u32 nodes, commit per iteration", tile, tops, out, cus);
    run_top<NW, K, true, false, 4>("... from 12 packed dwords, 16 perm", tile, tops, out, cus);
    run_top<NW, K, false, true, 0>("u32 nodes, child pairs (5+2)", tile, tops, out, cus);
    run_top<NW, K, true, true, 0>("u32 nodes, chosen child (4+2)", tile, tops, out, cus);
    run_top<NW, K, true, true, 1>("3-B nodes, straddling dword (5+2)", tile, tops, out, cus);
    run_top<NW, K, true, true, 2>("u16 code + u8 fid arrays (5+3)", tile, tops, out, cus);
    run_top<NW, K, true, true, 3>("u32 nodes, commit per iteration", tile, tops, out, cus);
    run_top<NW, K, true, true, 4>("... from 12 packed dwords, 16 perm", tile, tops, out, cus);
}

int main(int argc, char **argv)
{
    uint64_t s = 99;
    auto rnd = [&]() {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (uint32_t)(s >> 33);
    };
    std::vector<uint16_t> h_tile(COLS * 128);
    for (auto &v : h_tile) v = (uint16_t)(rnd() % 16000);
    std::vector<uint32_t> h_tops(64 * 1024);
    for (auto &n : h_tops) n = ((rnd() % 16000 + 1) << 16) | ((rnd() & 0xffu) << 8) | (rnd() & 1u);
    uint16_t *d_tile;
    uint32_t *d_tops, *d_out;
    CHECK(hipMalloc(&d_tile, h_tile.size() * 2));
    CHECK(hipMalloc(&d_tops, h_tops.size() * 4));
    CHECK(hipMalloc(&d_out, 256 * 16 * 64 * 4));
    CHECK(hipMemcpy(d_tile, h_tile.data(), h_tile.size() * 2, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_tops, h_tops.data(), h_tops.size() * 4, hipMemcpyHostToDevice));
    if (argc > 1 && std::string(argv[1]) == "--kernel-shape") {
        run_json<14, 3>(d_tile, d_tops, d_out);
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "--top-forms") {
        run_top_forms<14, 3>(d_tile, d_tops, d_out);
        return 0;
    }

    run<15, 2, 0, false>(d_tile, d_tops, d_out);
    run<15, 2, 0, true>(d_tile, d_tops, d_out);
    run<15, 2, 0, false, 256, true>(d_tile, d_tops, d_out);
    run<15, 2, 0, true, 256, true>(d_tile, d_tops, d_out);
    run<15, 2, 0, true, 128, false>(d_tile, d_tops, d_out);
    run<13, 3, 0, false, 128, false>(d_tile, d_tops, d_out);
    run<13, 3, 0, true, 128, false>(d_tile, d_tops, d_out);
    run<13, 3, 0, false, 128, true>(d_tile, d_tops, d_out);
    run<13, 3, 0, true, 128, true>(d_tile, d_tops, d_out);
    run<14, 3, 0, true, 128, false>(d_tile, d_tops, d_out);
    run<7, 4, 0, true, 128, false>(d_tile, d_tops, d_out);
    run<7, 4, 0, true, 128, true>(d_tile, d_tops, d_out);
    run<15, 2, 1, false>(d_tile, d_tops, d_out);
    run<15, 2, 2, false>(d_tile, d_tops, d_out);
    run<15, 1, 0, false>(d_tile, d_tops, d_out);
    run<16, 2, 0, false>(d_tile, d_tops, d_out);
    run<12, 2, 0, false>(d_tile, d_tops, d_out);
    run<8, 2, 0, false>(d_tile, d_tops, d_out);
    run<8, 2, 0, true>(d_tile, d_tops, d_out);
    run<4, 2, 0, true>(d_tile, d_tops, d_out);
    run<13, 3, 0, false>(d_tile, d_tops, d_out);
    run<13, 3, 0, true>(d_tile, d_tops, d_out);
    run<13, 3, 1, false>(d_tile, d_tops, d_out);
    run<13, 3, 2, false>(d_tile, d_tops, d_out);
    run<8, 3, 0, true>(d_tile, d_tops, d_out);
    run<7, 4, 0, false>(d_tile, d_tops, d_out);
    run<7, 4, 0, true>(d_tile, d_tops, d_out);
    run<4, 4, 0, true>(d_tile, d_tops, d_out);
    return 0;
}
