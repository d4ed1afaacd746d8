// Prices the prologue staging patterns alone (no walk, no search): global memory -> LDS for the two shapes of K3,
//   walk      1 workgroup per CU, 960 threads, 160 KiB dynamic LDS, 96-KiB tiles (three 32-KiB regions) of a 512-MB buffer, each tile read once
//   quantise  1024 threads, a 144-KiB image out of an 18-MB set, each image read by 16 workgroups (L2 hits after the first)
// in three variants each:
//   loops     the loops the kernels had: one 16-byte (walk) / 4-byte (quantise) load per lane and trip, waited for before its store
//   burst     tahoe_amd/csrc/stage_burst.h: every load of the copy issued before the first wait, committed with ds_write_b128
//   lds-dma   __builtin_amdgcn_global_load_lds, 16 bytes per lane, 1 KiB per wave-instruction, no registers
// After the barrier every thread reads 16 bytes of what another wave staged and the sum goes to global memory, so nothing is dead.
//   hipcc --offload-arch=gfx950 -O3 -I tahoe_amd/csrc -o tools/ubench_stage tools/ubench_stage.hip && tools/ubench_stage
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stage_burst.h"

#define CK(x)                                                                                      \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));      \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

constexpr int kRegion = 32768, kTile = 3 * kRegion, kImage = 144 * 1024;

__device__ __forceinline__ void dma16(const unsigned char *src, unsigned char *lds_dst)
{
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)src, (__attribute__((address_space(3))) void *)lds_dst, 16, 0, 0);
}

// whole 1-KiB wave-pieces of `bytes` (a multiple of 1 KiB), dealt round-robin to the NT / 64 waves: the trip count is wave-uniform
template <int NT>
__device__ __forceinline__ void dma_copy(const unsigned char *src, unsigned char *dst, int bytes, int tid)
{
    const int wave = tid >> 6, lane = tid & 63;
    for (int wp = wave; wp < bytes / 1024; wp += NT / 64) dma16(src + (size_t)wp * 1024 + lane * 16, dst + (size_t)wp * 1024);
}

template <int NT, int VARIANT, bool WALK>
__global__ void __launch_bounds__(NT) stage_kernel(const unsigned char *__restrict__ buf, float *__restrict__ out, int iters, int share, int nbytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    float acc = 0.0f;
    for (int it = 0; it < iters; ++it) {
        // walk: tile = blockIdx.x + it * gridDim.x (each once); quantise: image = blockIdx.x / share
        const size_t unit = WALK ? (size_t)blockIdx.x + (size_t)it * gridDim.x : (size_t)(blockIdx.x / share);
        const unsigned char *src = buf + unit * (WALK ? kTile : kImage);
        constexpr int BYTES = WALK ? kTile : kImage;
        if (VARIANT == 0) {
            if (WALK) {
                for (int k = 0; k < 3; ++k) {
                    const uint4 *s = reinterpret_cast<const uint4 *>(src + k * kRegion);
                    uint4 *d = reinterpret_cast<uint4 *>(smem + k * kRegion);
                    for (int e = tid; e < nbytes / 16; e += NT) d[e] = s[e];  // (nbytes = kRegion: a run-time bound, as in the kernels)
                }
            } else {
                const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
                uint32_t *d = reinterpret_cast<uint32_t *>(smem);
                for (int e = tid; e < nbytes / 4; e += NT) d[e] = s[e];  // (nbytes = kImage)
            }
        } else if (VARIANT == 1) {
            if (WALK) {
                constexpr int P = (kRegion / 16 + NT - 1) / NT;
                const uint32_t n16 = kRegion / 16, wrap = tahoe::stage_wrap(n16);
                tahoe::StageRegs<3 * P> v;
                tahoe::stage_issue<NT, P, 3>(v, reinterpret_cast<const uint4 *>(src), n16, tid, n16, wrap);
                tahoe::stage_commit<NT, P, 3>(v, reinterpret_cast<uint4 *>(smem), n16, tid, n16, wrap);
            } else {
                tahoe::stage_copy_once<NT, 10>(src, smem, BYTES, tid);
            }
        } else {
            dma_copy<NT>(src, smem, BYTES, tid);
        }
        __syncthreads();  // (waits for the LDS-DMA too: vmcnt(0) is part of its fence)
        const uint4 r = reinterpret_cast<const uint4 *>(smem)[(tid * 37 + 64) % (BYTES / 16)];
        acc += __uint_as_float((r.x ^ r.y ^ r.z ^ r.w) & 0x3f800000u);
        __syncthreads();  // everyone has read before the next copy overwrites
    }
    out[(size_t)blockIdx.x * NT + tid] = acc;
}

template <int NT, int VARIANT, bool WALK>
static void run(const char *name, const unsigned char *buf, float *out, int grid, int iters, int share, double bytes)
{
    const size_t lds = WALK ? 160 * 1024 : kImage;
    CK(hipFuncSetAttribute((const void *)&stage_kernel<NT, VARIANT, WALK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    float best = 1e30f, sum = 0.0f;
    const int reps = 10;
    for (int r = -3; r < reps; ++r) {
        CK(hipEventRecord(a));
        hipLaunchKernelGGL((stage_kernel<NT, VARIANT, WALK>), dim3(grid), dim3(NT), lds, 0, buf, out, iters, share, WALK ? kRegion : kImage);
        CK(hipGetLastError());
        CK(hipEventRecord(b));
        CK(hipEventSynchronize(b));
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        if (r >= 0) {
            best = ms < best ? ms : best;
            sum += ms;
        }
    }
    printf("%-9s %-8s %5d workgroups x %2d copies: avg %8.1f us, min %8.1f us, %6.2f TB/s at min, %7.0f cycles per copy at 2.4 GHz\n", WALK ? "walk" : "quantise",
           name, grid, iters, sum / reps * 1e3, best * 1e3, bytes / (best * 1e-3) / 1e12, best * 1e-3 * 2.4e9 / iters / (WALK ? 1.0 : (double)grid / 256.0));
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(b));
}

int main()
{
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const size_t walk_bytes = (size_t)512 << 20;
    const int tiles = (int)(walk_bytes / kTile);
    const int iters = tiles / cus;  // every tile read once: cus * iters <= tiles
    const int images = 128, share = 16;  // 128 x 144 KiB = 18 MB
    unsigned char *buf = nullptr;
    float *out = nullptr;
    CK(hipMalloc((void **)&buf, walk_bytes));
    CK(hipMemset(buf, 0x3f, walk_bytes));
    CK(hipMalloc((void **)&out, (size_t)images * share * 1024 * sizeof(float)));
    if (cus > images * share || (size_t)images * kImage > walk_bytes || iters < 1) {
        fprintf(stderr, "unexpected device shape\n");
        return 1;
    }
    printf("%s, %d CUs; walk shape: %d tiles of 96 KiB per workgroup; quantise shape: %d images of 144 KiB x %d workgroups each\n", prop.name, cus, iters,
           images, share);
    for (int round = 0; round < 2; ++round) {
        run<960, 0, true>("loops", buf, out, cus, iters, 1, (double)cus * iters * kTile);
        run<960, 1, true>("burst", buf, out, cus, iters, 1, (double)cus * iters * kTile);
        run<960, 2, true>("lds-dma", buf, out, cus, iters, 1, (double)cus * iters * kTile);
        run<1024, 0, false>("loops", buf, out, images * share, 1, share, (double)images * share * kImage);
        run<1024, 1, false>("burst", buf, out, images * share, 1, share, (double)images * share * kImage);
        run<1024, 2, false>("lds-dma", buf, out, images * share, 1, share, (double)images * share * kImage);
    }
    CK(hipFree(buf));
    CK(hipFree(out));
    return 0;
}
