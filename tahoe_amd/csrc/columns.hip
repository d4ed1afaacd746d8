// Predictions from column-major batches (tahoe_forest_predict_columns, tahoe_forest_predict_column_ptrs): one buffer per column,
// or one buffer with a column stride.  No row-major copy of the batch is asked of the caller.
//
// Two paths, chosen per call by columns_fused_strategy (forest.hip):
//   fused     the kernel the handle would run on row-major rows reads the columns itself: QRING's quantise pass (quantize.hip,
//             the COLS instantiations; every QRING walk reads codes only) or the 64-row float32 tile loader (cols_stage_tile,
//             forest_internal.h) of rowtile_kernel, sparse_kernel<TILE> and sparse_top_kernel.  No row-major copy exists anywhere.
//   chunks    columns_to_rows_kernel transposes a chunk of rows into the buffer the CSR fallback also uses (capped by
//             TAHOE_CSR_CHUNK_MB, counted in device_bytes), the handle's own predict path runs on the chunk, and so on chunk after
//             chunk on the caller's stream: every other kernel form and every handle kind is served
// Both paths feed the same kernels the same float32 values, so both write the bits tahoe_forest_predict writes for the row-major
// matrix of those values.
#include <algorithm>

#include "forest_internal.h"

namespace tahoe {

constexpr int kTrTile = 64;            // the transpose moves 64 rows x 64 columns per workgroup
constexpr int kTrStride = kTrTile + 1; // LDS row stride, odd: neither side of the transpose bank-conflicts

// out[r][c] (rows x cols, row-major) = column c, row row_begin + r.  blockIdx.x runs over 64-row blocks, blockIdx.y over 64-column
// blocks.  In: wave w takes columns w, w + 4, ... of the block, lane = row -- 256 consecutive bytes of one column per wave-load,
// the column's address a scalar load -- and stores lds[c][r] (lane-linear, conflict-free).  Out: wave w takes rows w, w + 4, ...,
// lane = column -- 256 consecutive bytes of one output row per wave-store -- reading lds[lane][r]: stride 65 words, 32 distinct
// banks per half wave.  Both edges are masked: nothing outside [0, rows) of a column or [0, cols) of the table is read, nothing
// outside the chunk is written.
__global__ void __launch_bounds__(kBlock) columns_to_rows_kernel(float *__restrict__ out, ColsView cv, size_t row_begin, size_t rows,
                                                                 int cols)
{
    __shared__ float lds[kTrTile * kTrStride];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t r0 = (size_t)blockIdx.x * kTrTile;
    const int c0 = (int)blockIdx.y * kTrTile;
    const int nc = min(kTrTile, cols - c0);
    const int nr = rows - r0 < (size_t)kTrTile ? (int)(rows - r0) : kTrTile;
    if (lane < nr)
        for (int c = wave; c < nc; c += kWaves) lds[c * kTrStride + lane] = cv.col(c0 + c)[row_begin + r0 + lane];
    __syncthreads();
    if (lane < nc)
        for (int r = wave; r < nr; r += kWaves) out[(r0 + r) * (size_t)cols + c0 + lane] = lds[lane * kTrStride + r];
}

static int columns_fused_form(const tahoe_forest *f, int strategy, size_t rows)
{
    if (strategy == TAHOE_STRATEGY_QRING) return tahoe_forest_get_kernel_form(f, rows);  // the walk's ordinary form
    if (!f->sp) return TAHOE_COLUMNS_FORM_ROWTILE;
    return strategy == TAHOE_STRATEGY_TILEBLOCK ? TAHOE_COLUMNS_FORM_SPARSE_TOP : TAHOE_COLUMNS_FORM_SPARSE_ROWTILE;
}

// What both entry points do once their arguments are checked
static tahoe_status predict_columns(tahoe_forest *f, float *preds_dev, const ColsView &cv, size_t rows, hipStream_t stream,
                                    const char *fn)
{
    DeviceGuard on_device(f->device);
    const bool timed = f->profiling && f->prof_count < f->ev_start.size();
    const int fused = columns_fused_strategy(f, rows);
    if (fused == TAHOE_STRATEGY_QRING && !f->sp)  // launch_traversal times the quantise pass and the walk apart, as on rows
        return predict_rows(f, preds_dev, nullptr, rows, stream, nullptr, fused, &cv);
    if (timed) {  // kernel_times reads the whole call, prepass_times 0
        TAHOE_HIP_TRY(hipEventRecord(f->ev_start[f->prof_count], stream));
        TAHOE_HIP_TRY(hipEventRecord(f->ev_mid[f->prof_count], stream));
    }
    {
        ProfilingPause pause(f);
        if (fused >= 0) {
            if (const tahoe_status s = predict_rows(f, preds_dev, nullptr, rows, stream, nullptr, fused, &cv)) return s;
        } else if (f->p.num_cols == 0 || f->p.num_trees == 0) {
            if (const tahoe_status s = predict_rows(f, preds_dev, nullptr, rows, stream)) return s;  // no value of the batch is read
        } else {
            if (const tahoe_status s = csr_reserve_chunk(f, rows, fn)) return s;  // no-op unless this batch needs a larger chunk
            const size_t chunk = f->csr_chunk_rows, out_cols = (size_t)f->num_classes;
            const unsigned col_blocks = (unsigned)((f->p.num_cols + kTrTile - 1) / kTrTile);
            for (size_t r0 = 0; r0 < rows; r0 += chunk) {
                const size_t n = std::min(chunk, rows - r0);
                const size_t grid = (n + kTrTile - 1) / kTrTile;
                if (grid > 0x7fffffffu || col_blocks > 65535u)
                    return fail(TAHOE_ERR_INVALID_ARG, "%s: too many rows or columns for one launch: %zu x %d", fn, n, f->p.num_cols);
                hipLaunchKernelGGL(columns_to_rows_kernel, dim3((unsigned)grid, col_blocks), dim3(kBlock), 0, stream, f->csr_chunk, cv,
                                   r0, n, f->p.num_cols);
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

}  // namespace tahoe

using namespace tahoe;

extern "C" {

tahoe_status tahoe_forest_predict_columns(tahoe_forest *f, float *preds_dev, const float *data_dev, size_t rows, size_t col_stride,
                                          void *stream)
{
    // (none of the argument checks reads the handle)
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_columns: null forest");
    if (rows && (!preds_dev || !data_dev)) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_columns: null preds_dev / data_dev");
    if (col_stride < rows)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_columns: col_stride %zu is less than rows %zu", col_stride, rows);
    if (rows == 0) return TAHOE_OK;
    return predict_columns(f, preds_dev, ColsView{nullptr, data_dev, col_stride}, rows, (hipStream_t)stream, "tahoe_forest_predict_columns");
}

tahoe_status tahoe_forest_predict_column_ptrs(tahoe_forest *f, float *preds_dev, const float *const *cols_dev, size_t rows,
                                              void *stream)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_column_ptrs: null forest");
    if (rows && (!preds_dev || !cols_dev)) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_column_ptrs: null preds_dev / cols_dev");
    if (rows == 0) return TAHOE_OK;
    return predict_columns(f, preds_dev, ColsView{cols_dev, nullptr, 0}, rows, (hipStream_t)stream, "tahoe_forest_predict_column_ptrs");
}

tahoe_status tahoe_forest_reserve_columns(tahoe_forest *f, size_t rows)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_reserve_columns: null forest");
    if (rows == 0) return TAHOE_OK;
    // A fused call needs what the same strategy needs on row-major rows (QRING's code workspace), a chunked one the chunk buffer
    // and the kernels' workspace for one chunk.  AUTO's pick moves with the batch size on a sparse handle only, between forms
    // that are all fused or all chunked; a one-row batch is asked as well so that this holds without relying on it.
    if ((columns_fused_strategy(f, rows) >= 0 && columns_fused_strategy(f, 1) >= 0) || f->p.num_cols == 0 || f->p.num_trees == 0)
        return tahoe_forest_reserve(f, rows);
    if (const tahoe_status s = csr_reserve_chunk(f, rows, "tahoe_forest_reserve_columns")) return s;
    return tahoe_forest_reserve(f, columns_fused_strategy(f, rows) >= 0 ? rows : f->csr_chunk_rows);
}

tahoe_status tahoe_forest_get_columns_plan(const tahoe_forest *f, size_t rows, int *form, size_t *chunk_rows)
{
    if (!f || !form || !chunk_rows) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_get_columns_plan: null argument");
    const int fused = columns_fused_strategy(f, rows);
    const bool unread = f->p.num_cols == 0 || f->p.num_trees == 0;  // no value of the batch is read: nothing is copied either
    *chunk_rows = fused >= 0 || unread ? 0 : csr_chunk_cap(f);
    *form = fused >= 0 ? columns_fused_form(f, fused, rows) : tahoe_forest_get_kernel_form(f, unread ? rows : std::min(rows, *chunk_rows));
    return TAHOE_OK;
}

}  // extern "C"
