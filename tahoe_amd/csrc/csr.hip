// Predictions from CSR rows (tahoe_forest_predict_csr): an entry that is not stored is the missing value.
//
// Two paths, chosen per call by csr_fused_strategy (forest.hip; DESIGN.md, "CSR rows"):
//   fused     the 64-row float32 tile kernels (rowtile_kernel, sparse_kernel<TILE>, sparse_top_kernel; oblivious_tile_kernel and
//             vector_tile_kernel on a handle of TAHOE_CREATE_CSR) stage their LDS tile straight from the CSR arrays
//             (csr_stage_tile, csr_stage_tile_wave; forest_internal.h): no dense copy exists anywhere
//   fallback  csr_densify_kernel writes a chunk of rows as dense float32 into a buffer the handle owns (capped by
//             TAHOE_CSR_CHUNK_MB, counted in device_bytes), the handle's own predict path runs on the chunk, and so on chunk
//             after chunk on the caller's stream: every other kernel form is served, with extra memory independent of `rows`
// Rows are independent and every form adds a row's leaf values in tree order, so both paths write the bits that
// tahoe_forest_predict writes for the densified matrix.
#include <algorithm>

#include "forest_internal.h"

namespace tahoe {

constexpr int kDensifyRows = kBlock / kCsrLanes;  // rows per workgroup: 32

// out[r][c] (rows x cols, row-major) = missing, then the stored entries of rows row_begin + r over it.  A workgroup owns 32
// whole rows: it fills its slab (16-byte stores: the slab starts at a multiple of 128 bytes), and after the barrier kCsrLanes
// lanes stride over each row's entries.  Entry ranges are clamped to [0, nnz]; an entry whose column is outside [0, cols) is
// skipped and raises csr.bad_column.
__global__ void __launch_bounds__(kBlock) csr_densify_kernel(float *__restrict__ out, CsrView csr, size_t row_begin, size_t rows,
                                                             size_t total_rows, int cols, float missing)
{
    const size_t r0 = (size_t)blockIdx.x * kDensifyRows;
    const int nr = rows - r0 < (size_t)kDensifyRows ? (int)(rows - r0) : kDensifyRows;
    float *slab = out + r0 * (size_t)cols;
    const size_t n = (size_t)nr * cols;
    float4 *slab4 = reinterpret_cast<float4 *>(slab);
    const float4 m4 = make_float4(missing, missing, missing, missing);
    for (size_t i = threadIdx.x; i < n / 4; i += kBlock) slab4[i] = m4;
    if (threadIdx.x < n % 4) slab[n - 1 - threadIdx.x] = missing;
    __syncthreads();  // the fill is complete (s_waitcnt vmcnt(0) + s_barrier) before the same workgroup's scatter
    const int r = threadIdx.x / kCsrLanes, sub = threadIdx.x % kCsrLanes;
    if (r >= nr) return;
    const size_t row = row_begin + r0 + r;
    const int64_t end = csr_row_begin(csr, row + 1, total_rows);
    bool bad = false;
    for (int64_t k = csr_row_begin(csr, row, total_rows) + sub; k < end; k += kCsrLanes) {
        const int32_t c = csr.indices[k];
        const float v = csr.values[k];
        if ((uint32_t)c < (uint32_t)cols) slab[(size_t)r * cols + c] = v;
        else bad = true;
    }
    if (bad) atomicOr(csr.bad_column, 1);
}

// Rows per densify chunk: what TAHOE_CSR_CHUNK_MB holds, in whole tiles of every kernel form (384 = lcm of the 64-, 128-, 192-
// and 384-row tiles) where that many fit, else in 64-row tiles; at least one of those
size_t csr_chunk_cap(const tahoe_forest *f)
{
    const size_t row_bytes = std::max<size_t>((size_t)f->p.num_cols, 1) * sizeof(float);
    const size_t fit = ((size_t)std::max(f->knobs.csr_chunk_mb, 1) << 20) / row_bytes;
    return fit >= 384 ? fit / 384 * 384 : std::max<size_t>(fit / 64 * 64, 64);
}

// The chunk buffer holds min(rows, cap) rows after this; grows only
tahoe_status csr_reserve_chunk(tahoe_forest *f, size_t rows, const char *fn)
{
    const size_t want = std::min(rows, csr_chunk_cap(f));
    if (want <= f->csr_chunk_rows) return TAHOE_OK;
    const size_t row_bytes = std::max<size_t>((size_t)f->p.num_cols, 1) * sizeof(float);
    DeviceGuard on_device(f->device);
    if (f->csr_chunk) {
        TAHOE_HIP_TRY(hipDeviceSynchronize());  // a previous launch may still read the old buffer
        TAHOE_HIP_TRY(hipFree(f->csr_chunk));
        f->device_bytes -= f->csr_chunk_rows * row_bytes;
        f->csr_chunk = nullptr;
        f->csr_chunk_rows = 0;
    }
    if (hipMalloc(reinterpret_cast<void **>(&f->csr_chunk), want * row_bytes) != hipSuccess) {
        f->csr_chunk = nullptr;
        return fail(TAHOE_ERR_NO_MEMORY, "%s: no room for a %zu-row chunk of %d columns", fn, want, f->p.num_cols);
    }
    f->csr_chunk_rows = want;
    f->device_bytes += want * row_bytes;
    return TAHOE_OK;
}

void csr_destroy(tahoe_forest *f)
{
    if (f->csr_chunk) (void)hipFree(f->csr_chunk);
    f->csr_chunk = nullptr;
}

static int csr_fused_form(const tahoe_forest *f, int strategy)
{
    if (f->ob) return TAHOE_OBLIVIOUS_FORM_CSR_TILE;
    if (f->vl) return TAHOE_VECTOR_FORM_CSR_TILE;
    if (!f->sp) return TAHOE_FORM_CSR_ROWTILE;
    return strategy == TAHOE_STRATEGY_TILEBLOCK ? TAHOE_FORM_CSR_SPARSE_TOP : TAHOE_FORM_CSR_SPARSE_ROWTILE;
}

}  // namespace tahoe

using namespace tahoe;

extern "C" {

tahoe_status tahoe_forest_predict_csr(tahoe_forest *f, float *preds_dev, const int64_t *indptr_dev, const int32_t *indices_dev,
                                      const float *values_dev, size_t rows, size_t nnz, void *stream_)
{
    // (none of the argument checks reads the handle)
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_csr: null forest");
    if (rows && (!preds_dev || !indptr_dev)) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_csr: null preds_dev / indptr_dev");
    if (nnz && (!indices_dev || !values_dev)) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_csr: null indices_dev / values_dev");
    if (nnz > (size_t)INT64_MAX) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_csr: nnz %zu does not fit indptr's int64", nnz);
    if (const tahoe_status st = refuse_no_csr(f, "tahoe_forest_predict_csr")) return st;
    if (rows == 0) return TAHOE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard on_device(f->device);
    const CsrView csr{indptr_dev, indices_dev, values_dev, nnz, f->error_flag + 1};
    const bool timed = f->profiling && f->prof_count < f->ev_start.size();
    if (timed) {  // kernel_times reads the whole call, prepass_times 0
        TAHOE_HIP_TRY(hipEventRecord(f->ev_start[f->prof_count], stream));
        TAHOE_HIP_TRY(hipEventRecord(f->ev_mid[f->prof_count], stream));
    }
    {
        ProfilingPause pause(f);
        const int fused = csr_fused_strategy(f, rows, nnz);
        if (fused >= 0) {
            if (const tahoe_status s = predict_rows(f, preds_dev, nullptr, rows, stream, &csr, fused)) return s;
        } else {
            if (const tahoe_status s = csr_reserve_chunk(f, rows, "tahoe_forest_predict_csr")) return s;  // no-op unless this batch needs a larger chunk
            const size_t chunk = f->csr_chunk_rows, out_cols = (size_t)f->num_classes;
            for (size_t r0 = 0; r0 < rows; r0 += chunk) {
                const size_t n = std::min(chunk, rows - r0);
                const size_t grid = (n + kDensifyRows - 1) / kDensifyRows;
                if (grid > 0x7fffffffu) return fail(TAHOE_ERR_INVALID_ARG, "too many rows for one launch: %zu", n);
                hipLaunchKernelGGL(csr_densify_kernel, dim3((unsigned)grid), dim3(kBlock), 0, stream, f->csr_chunk, csr, r0, n, rows,
                                   f->p.num_cols, f->p.missing);
                TAHOE_HIP_TRY(hipGetLastError());
                if (const tahoe_status s = predict_rows(f, preds_dev + r0 * out_cols, f->csr_chunk, n, stream)) return s;
            }
        }
    }
    if (timed) {
        TAHOE_HIP_TRY(hipEventRecord(f->ev_stop[f->prof_count], stream));
        ++f->prof_count;
    }
    return TAHOE_OK;
}

tahoe_status tahoe_forest_reserve_csr(tahoe_forest *f, size_t rows, size_t nnz)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "null forest");
    if (const tahoe_status st = refuse_no_csr(f, "tahoe_forest_reserve_csr")) return st;
    // Which path a later call takes depends on its own rows and nnz, so the fallback's workspace is sized whatever `nnz` says: the
    // chunk buffer, and what the handle's kernels need for a batch of one chunk.  The fused kernels need no workspace.
    (void)nnz;
    if (rows == 0) return TAHOE_OK;
    if (const tahoe_status s = csr_reserve_chunk(f, rows, "tahoe_forest_reserve_csr")) return s;
    return tahoe_forest_reserve(f, f->csr_chunk_rows);
}

tahoe_status tahoe_forest_get_csr_plan(const tahoe_forest *f, size_t rows, size_t nnz, int *form, size_t *chunk_rows)
{
    if (!f || !form || !chunk_rows) return fail(TAHOE_ERR_INVALID_ARG, "null argument");
    if (const tahoe_status st = refuse_no_csr(f, "tahoe_forest_get_csr_plan")) {  // no CSR path: nothing would be launched
        *form = TAHOE_FORM_NONE;
        *chunk_rows = 0;
        return st;
    }
    const int fused = csr_fused_strategy(f, rows, nnz);
    *chunk_rows = fused >= 0 ? 0 : csr_chunk_cap(f);
    *form = fused >= 0 ? csr_fused_form(f, fused) : tahoe_forest_get_kernel_form(f, std::min(rows, *chunk_rows));
    return TAHOE_OK;
}

}  // extern "C"
