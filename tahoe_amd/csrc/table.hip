// Predictions from a table of typed, nullable columns (tahoe_table_create, tahoe_forest_predict_table): a cuDF / Arrow table as it
// is -- float32 / float64 / float16 and 8- to 64-bit integer columns, each with an optional validity bitmap and an element offset.
// No float32 copy of a column and no rewrite of a column with nulls is asked of the caller.
//
// Every element goes through table_load (forest_internal.h): a null becomes params.missing, everything else (float)element.  Two
// paths, chosen per call by table_fused_strategy (forest.hip):
//   fused     QRING's quantise pass (quantize.hip, the TAB instantiations) converts as it loads; every QRING walk reads codes only
//   chunks    table_to_rows_kernel converts and transposes a chunk of rows into the buffer the CSR and column fallbacks also use
//             (capped by TAHOE_CSR_CHUNK_MB, counted in device_bytes), the handle's own predict path runs on the chunk, and so on
//             chunk after chunk on the caller's stream: every other kernel form and every handle kind is served
// Both paths feed the same kernels the same float32 values, so both write the bits tahoe_forest_predict writes for the row-major
// matrix of those values.
#include <algorithm>
#include <vector>

#include "forest_internal.h"

// The device copy of the caller's descriptors; the buffers they name stay the caller's
struct tahoe_table {
    tahoe_column *cols = nullptr;  // [num_cols] on `device`
    int num_cols = 0;
    size_t rows = 0;
    int device = 0;
};

namespace tahoe {

constexpr int kTabTile = 64;             // 64 rows x 64 columns per workgroup
constexpr int kTabStride = kTabTile + 1; // LDS row stride, odd: neither side of the transpose bank-conflicts

// out[r][c] (rows x cols, row-major) = table_load(column c, row row_begin + r).  The geometry of columns_to_rows_kernel: blockIdx.x
// runs over 64-row blocks, blockIdx.y over 64-column blocks.  In: wave w takes columns w, w + 4, ... of the block, lane = row --
// the descriptor a scalar load, the type switch a uniform branch, 64 consecutive elements of one column per wave-load, the row's
// validity byte read by its lane (eight lanes share a byte) -- and stores lds[c][r] (lane-linear, conflict-free).  Out: wave w takes
// rows w, w + 4, ..., lane = column -- 256 consecutive bytes of one output row per wave-store -- reading lds[lane][r]: stride 65
// words.  Both edges are masked: no row outside [0, rows) of a column and no descriptor outside [0, cols) is read, nothing outside
// the chunk is written.
__global__ void __launch_bounds__(kBlock) table_to_rows_kernel(float *__restrict__ out, TableView tv, size_t row_begin, size_t rows,
                                                               int cols, float missing)
{
    __shared__ float lds[kTabTile * kTabStride];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t r0 = (size_t)blockIdx.x * kTabTile;
    const int c0 = (int)blockIdx.y * kTabTile;
    const int nc = min(kTabTile, cols - c0);
    const int nr = rows - r0 < (size_t)kTabTile ? (int)(rows - r0) : kTabTile;
    if (lane < nr)
        for (int c = wave; c < nc; c += kWaves) lds[c * kTabStride + lane] = table_load(tv.cols[c0 + c], row_begin + r0 + lane, missing);
    __syncthreads();
    if (lane < nc)
        for (int r = wave; r < nr; r += kWaves) out[(r0 + r) * (size_t)cols + c0 + lane] = lds[lane * kTabStride + r];
}

static int col_elem_size(int type)
{
    switch (type) {
    case TAHOE_COL_FLOAT32: case TAHOE_COL_INT32: case TAHOE_COL_UINT32: return 4;
    case TAHOE_COL_FLOAT64: case TAHOE_COL_INT64: case TAHOE_COL_UINT64: return 8;
    case TAHOE_COL_FLOAT16: case TAHOE_COL_INT16: case TAHOE_COL_UINT16: return 2;
    case TAHOE_COL_INT8: case TAHOE_COL_UINT8: return 1;
    default: return 0;
    }
}

static tahoe_status predict_table(tahoe_forest *f, float *preds_dev, const tahoe_table *t, hipStream_t stream, const char *fn)
{
    DeviceGuard on_device(f->device);
    const size_t rows = t->rows;
    const TableView tv{t->cols};
    const bool timed = f->profiling && f->prof_count < f->ev_start.size();
    const int fused = table_fused_strategy(f, rows);
    if (fused == TAHOE_STRATEGY_QRING && !f->sp)  // launch_traversal times the quantise pass and the walk apart, as on rows
        return predict_rows(f, preds_dev, nullptr, rows, stream, nullptr, fused, nullptr, &tv);
    if (timed) {  // kernel_times reads the whole call, prepass_times 0
        TAHOE_HIP_TRY(hipEventRecord(f->ev_start[f->prof_count], stream));
        TAHOE_HIP_TRY(hipEventRecord(f->ev_mid[f->prof_count], stream));
    }
    {
        ProfilingPause pause(f);
        if (fused >= 0) {
            if (const tahoe_status s = predict_rows(f, preds_dev, nullptr, rows, stream, nullptr, fused, nullptr, &tv)) return s;
        } else if (f->p.num_cols == 0 || f->p.num_trees == 0) {
            if (const tahoe_status s = predict_rows(f, preds_dev, nullptr, rows, stream)) return s;  // no column is read
        } else {
            if (const tahoe_status s = csr_reserve_chunk(f, rows, fn)) return s;  // no-op unless this batch needs a larger chunk
            const size_t chunk = f->csr_chunk_rows, out_cols = (size_t)f->num_classes;
            const unsigned col_blocks = (unsigned)((f->p.num_cols + kTabTile - 1) / kTabTile);
            for (size_t r0 = 0; r0 < rows; r0 += chunk) {
                const size_t n = std::min(chunk, rows - r0);
                const size_t grid = (n + kTabTile - 1) / kTabTile;
                if (grid > 0x7fffffffu || col_blocks > 65535u)
                    return fail(TAHOE_ERR_INVALID_ARG, "%s: too many rows or columns for one launch: %zu x %d", fn, n, f->p.num_cols);
                hipLaunchKernelGGL(table_to_rows_kernel, dim3((unsigned)grid, col_blocks), dim3(kBlock), 0, stream, f->csr_chunk, tv, r0,
                                   n, f->p.num_cols, f->p.missing);
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

tahoe_status tahoe_table_create(const tahoe_column *cols_host, int num_cols, size_t rows, tahoe_table **out)
{
    // (every refusal comes before a device is touched)
    if (!out) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_table_create: null out");
    *out = nullptr;
    if (num_cols < 0) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_table_create: num_cols %d is negative", num_cols);
    if (num_cols > 0 && !cols_host) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_table_create: null cols_host");
    for (int c = 0; c < num_cols; ++c) {
        const tahoe_column &d = cols_host[c];
        const int size = col_elem_size(d.type);
        if (size == 0) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_table_create: column %d: unknown type %d", c, d.type);
        if (d.reserved != 0) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_table_create: column %d: reserved is %d, not 0", c, d.reserved);
        if (d.offset < 0) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_table_create: column %d: negative offset %lld", c, (long long)d.offset);
        if (rows > 0 && !d.data) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_table_create: column %d: null data", c);
        if (reinterpret_cast<uintptr_t>(d.data) % (uintptr_t)size != 0)
            return fail(TAHOE_ERR_INVALID_ARG, "tahoe_table_create: column %d: data is not aligned to its %d-byte elements", c, size);
    }
    std::unique_ptr<tahoe_table> t(new tahoe_table);
    t->num_cols = num_cols;
    t->rows = rows;
    TAHOE_HIP_TRY(hipGetDevice(&t->device));
    size_t unused = 0;
    const hipError_t e = upload(&t->cols, cols_host, (size_t)num_cols, &unused);  // (hipMemcpy: done when this returns)
    if (e != hipSuccess) {
        if (t->cols) (void)hipFree(t->cols);
        return hip_status(e, "tahoe_table_create: upload");
    }
    *out = t.release();
    return TAHOE_OK;
}

void tahoe_table_destroy(tahoe_table *t)
{
    if (!t) return;
    if (t->cols) {
        DeviceGuard on_device(t->device);
        (void)hipFree(t->cols);
    }
    delete t;
}

tahoe_status tahoe_forest_predict_table(tahoe_forest *f, float *preds_dev, const tahoe_table *t, void *stream)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_table: null forest");
    if (!t) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_table: null table");
    if (!preds_dev) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_table: null preds_dev");
    if (t->num_cols != f->p.num_cols)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_table: the table has %d columns (num_cols), the forest %d", t->num_cols,
                    f->p.num_cols);
    if (t->device != f->device)
        return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_predict_table: the table is on device %d, the forest on device %d", t->device,
                    f->device);
    if (t->rows == 0) return TAHOE_OK;
    return predict_table(f, preds_dev, t, (hipStream_t)stream, "tahoe_forest_predict_table");
}

tahoe_status tahoe_forest_reserve_table(tahoe_forest *f, size_t rows)
{
    if (!f) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_reserve_table: null forest");
    if (rows == 0) return TAHOE_OK;
    // As tahoe_forest_reserve_columns: a fused call needs QRING's code workspace, a chunked one the chunk buffer and the kernels'
    // workspace for one chunk; a one-row batch is asked as well, since AUTO's pick moves with the batch size on a sparse handle.
    if ((table_fused_strategy(f, rows) >= 0 && table_fused_strategy(f, 1) >= 0) || f->p.num_cols == 0 || f->p.num_trees == 0)
        return tahoe_forest_reserve(f, rows);
    if (const tahoe_status s = csr_reserve_chunk(f, rows, "tahoe_forest_reserve_table")) return s;
    return tahoe_forest_reserve(f, table_fused_strategy(f, rows) >= 0 ? rows : f->csr_chunk_rows);
}

tahoe_status tahoe_forest_get_table_plan(const tahoe_forest *f, size_t rows, int *form, size_t *chunk_rows)
{
    if (!f || !form || !chunk_rows) return fail(TAHOE_ERR_INVALID_ARG, "tahoe_forest_get_table_plan: null argument");
    const int fused = table_fused_strategy(f, rows);
    const bool unread = f->p.num_cols == 0 || f->p.num_trees == 0;  // no column is read: nothing is copied either
    *chunk_rows = fused >= 0 || unread ? 0 : csr_chunk_cap(f);
    *form = tahoe_forest_get_kernel_form(f, fused >= 0 || unread ? rows : std::min(rows, *chunk_rows));
    return TAHOE_OK;
}

}  // extern "C"
