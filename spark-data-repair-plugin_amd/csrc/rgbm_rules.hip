// rgbm_rules.hip -- a relational step on the HBM-resident code table (what the steps share is rgbm_prep.h):
// =============================================================================================
// Rule-based repairs (python/repair/model.py `_build_rule_model`, `FunctionalDepModel.predict`, `PoorModel.predict`,
// `_repair_by_nearest_values`; reference model.py:44-100, 928-953, 1279-1291).
//
//   fd_map          for every code of x the single y code it occurs with over the rows where both cells are non-NULL, else -1.  Per x a
//                   (lo, hi) pair of y codes kept with integer atomicMin / atomicMax: unique iff lo == hi.  Min and max do not depend on
//                   the order of the rows, so the map is a function of the table, whatever the launch geometry.  A workgroup keeps the
//                   pairs of its row range in LDS (FD_LDS_CODES codes: 2 x 4 B each, 64 KiB, two workgroups a CU) and flushes the codes it
//                   saw with global vector atomics; more codes than that update the HBM tables directly.  A lane reads lo[x] / hi[x] first and
//                   issues the atomic only when y falls outside: lo only falls and hi only rises, so a stale read costs an atomic, never
//                   a wrong skip, and after the first rows of a low-cardinality x the loop is LDS reads (same address: broadcast).
//                   Algorithmic bytes: 8 B per row (two int32 columns), no staging: consecutive lanes load consecutive rows.
//   rule_fill       pred = lut[x] (or the constant lut[0]); NULL y cells receive pred >= 0; out_label = pred for every row.
//   row_nearest     one wave per row of a cost matrix: the minimum over the entries that are not NaN, whether it occurs once, and
//                   where; the position when the minimum is unique and <= threshold, else -1.
// =============================================================================================
#include "rgbm_prep.h"

namespace {

using namespace rgh;

constexpr int FD_B = 512;                                   // threads per workgroup
constexpr int FD_UNROLL = 4;                                // rows a lane loads before it updates
constexpr int FD_LDS_CODES = 8192;                          // x codes whose (lo, hi) pairs a workgroup keeps in LDS
constexpr long long NV_MAX_CELLS = 1ll << 30;               // entries of one nearest-value cost matrix

__global__ void k_fd_init(int* __restrict__ lo, int* __restrict__ hi, int nx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nx) { lo[i] = 0x7FFFFFFF; hi[i] = -1; }
}

template <bool LDS>
__global__ __launch_bounds__(FD_B) void k_fd_map(const int32_t* __restrict__ x, const int32_t* __restrict__ y, long long n, int nx, int ny,
                                                 long long rows_per_wg, int* glo, int* ghi) {
    extern __shared__ int fd_smem[];                        // LDS: lo [nx], hi [nx]
    int* lo = LDS ? fd_smem : glo;
    int* hi = LDS ? fd_smem + nx : ghi;
    const int tid = threadIdx.x;
    if (LDS) {
        for (int i = tid; i < nx; i += FD_B) { lo[i] = 0x7FFFFFFF; hi[i] = -1; }
        __syncthreads();
    }
    const long long begin = (long long)blockIdx.x * rows_per_wg;
    const long long end = begin + rows_per_wg < n ? begin + rows_per_wg : n;
    for (long long base = begin; base < end; base += FD_B * FD_UNROLL) {
        int xs[FD_UNROLL], ys[FD_UNROLL];
#pragma unroll
        for (int k = 0; k < FD_UNROLL; ++k) {
            const long long r = base + (long long)k * FD_B + tid;
            xs[k] = r < end ? x[r] : -1;
            ys[k] = r < end ? y[r] : -1;
        }
#pragma unroll
        for (int k = 0; k < FD_UNROLL; ++k) {
            const int xv = xs[k], yv = ys[k];
            if (xv < 0 || xv >= nx || yv < 0 || yv >= ny) continue;        // a NULL side: the row does not take part
            if (yv < lo[xv]) atomicMin(&lo[xv], yv);
            if (yv > hi[xv]) atomicMax(&hi[xv], yv);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = tid; i < nx; i += FD_B)
            if (hi[i] >= 0) { atomicMin(&glo[i], lo[i]); atomicMax(&ghi[i], hi[i]); }
    }
}

__global__ void k_fd_finish(const int* __restrict__ lo, const int* __restrict__ hi, int nx, int32_t* __restrict__ map) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nx) map[i] = lo[i] == hi[i] ? lo[i] : -1;                      // never seen: lo = INT_MAX, hi = -1
}

__global__ void k_rule_fill(int32_t* __restrict__ codes, long long n, int y_col, int x_col, const int32_t* __restrict__ lut, int n_lut,
                            long long row_begin, long long n_rows, int32_t* __restrict__ out_label) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const long long r = row_begin + i;
    int pred;
    if (x_col < 0) pred = lut[0];
    else { const int xv = codes[(long long)x_col * n + r]; pred = (xv >= 0 && xv < n_lut) ? lut[xv] : -1; }
    if (out_label) out_label[i] = pred;
    int32_t* cell = codes + (long long)y_col * n + r;
    if (pred >= 0 && *cell < 0) *cell = pred;
}

template <typename T>
__global__ __launch_bounds__(256) void k_row_nearest(const T* __restrict__ mat, long long n_a, int n_b, double threshold,
                                                     int32_t* __restrict__ out) {
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n_a) return;
    const int lane = (int)(threadIdx.x & 63u);
    const T* m = mat + row * n_b;
    double bm = 0.0; int cnt = 0, bp = 0x7FFFFFFF;           // the least value, how often it occurs (2 = more than once), its first position
    for (int c = lane; c < n_b; c += 64) {
        const double v = (double)m[c];
        if (isnan(v)) continue;                              // NaN = None: the pair has no cost
        if (cnt == 0 || v < bm) { bm = v; cnt = 1; bp = c; }
        else if (v == bm) cnt = 2;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double om = __shfl_xor(bm, d); const int oc = __shfl_xor(cnt, d); const int op = __shfl_xor(bp, d);
        if (oc > 0) {
            if (cnt == 0 || om < bm) { bm = om; cnt = oc; bp = op; }
            else if (om == bm) { cnt = 2; bp = op < bp ? op : bp; }
        }
    }
    if (lane == 0) out[row] = (cnt == 1 && bm <= threshold) ? bp : -1;
}

}  // namespace

extern "C" {

// scratch slots held together: TABLE_A (lo) TABLE_B (hi) VALS (map)
RGBM_EXPORT int rgbm_table_fd_map(const rgbm_table* t, int32_t x_col, int32_t y_col, int32_t* map_out) {
    if (!t || !map_out || x_col < 0 || x_col >= t->c || y_col < 0 || y_col >= t->c || x_col == y_col)
        return fail(RGBM_ERR_ARG, "rgbm_table_fd_map: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const int nx = t->n_codes[x_col], ny = t->n_codes[y_col];
        if (nx <= 0) return RGBM_OK;
        const long long n = t->n;
        int* d_lo = scr<int>(*t, SCR_TABLE_A, (size_t)nx);
        int* d_hi = scr<int>(*t, SCR_TABLE_B, (size_t)nx);
        int32_t* d_map = scr<int32_t>(*t, SCR_VALS, (size_t)nx);
        hipLaunchKernelGGL(k_fd_init, dim3(nblocks(nx, 256)), dim3(256), 0, s, d_lo, d_hi, nx);
        if (n > 0) {
            // enough workgroups to fill the device a few times over, each on a whole number of load tiles
            const long long tile = (long long)FD_B * FD_UNROLL;
            const long long chunks = std::max<long long>(1, std::min<long long>((n + 4 * tile - 1) / (4 * tile), 2048));
            const long long rows_per_wg = ((n + chunks - 1) / chunks + tile - 1) / tile * tile;
            const unsigned grid = (unsigned)((n + rows_per_wg - 1) / rows_per_wg);
            const int32_t* x = t->codes.p + (size_t)x_col * n;
            const int32_t* y = t->codes.p + (size_t)y_col * n;
            if (nx <= FD_LDS_CODES)
                hipLaunchKernelGGL(k_fd_map<true>, dim3(grid), dim3(FD_B), (size_t)nx * 2 * sizeof(int), s, x, y, n, nx, ny, rows_per_wg, d_lo, d_hi);
            else
                hipLaunchKernelGGL(k_fd_map<false>, dim3(grid), dim3(FD_B), 0, s, x, y, n, nx, ny, rows_per_wg, d_lo, d_hi);
        }
        hipLaunchKernelGGL(k_fd_finish, dim3(nblocks(nx, 256)), dim3(256), 0, s, d_lo, d_hi, nx, d_map);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(map_out, d_map, (size_t)nx * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

// scratch slots held together: IN_COLS (lut) VALS (labels)
RGBM_EXPORT int rgbm_table_rule_fill(rgbm_table* t, int32_t y_col, int32_t x_col, const int32_t* lut, int32_t n_lut, int64_t row_begin,
                                     int64_t n_rows, int32_t* out_label) {
    if (!t || y_col < 0 || y_col >= t->c || x_col >= t->c || x_col == y_col || !lut || n_lut < 1 || row_begin < 0 || n_rows < 0 ||
        row_begin > t->n || n_rows > t->n - row_begin)
        return fail(RGBM_ERR_ARG, "rgbm_table_rule_fill: bad argument");
    return guarded([&]() {
        use_device(t->device);
        rgh::ViewWrite view_wr(t);
        if (n_rows == 0) return RGBM_OK;
        const int ny = t->n_codes[y_col];
        for (int i = 0; i < n_lut; ++i)
            if (lut[i] >= ny) throw std::invalid_argument("rgbm_table_rule_fill: code outside the target column's dictionary");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const int32_t* d_lut = scr_upload<int32_t>(*t, SCR_IN_COLS, lut, (size_t)n_lut, s);
        int32_t* d_out = out_label ? scr<int32_t>(*t, SCR_VALS, (size_t)n_rows) : nullptr;
        hipLaunchKernelGGL(k_rule_fill, dim3(nblocks(n_rows, 256)), dim3(256), 0, s, t->codes.p, (long long)t->n, (int)y_col, (int)(x_col < 0 ? -1 : x_col),
                           d_lut, (int)n_lut, (long long)row_begin, (long long)n_rows, d_out);
        HIPCHK(hipGetLastError());
        if (out_label) HIPCHK(hipMemcpyAsync(out_label, d_out, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_nearest_values(int32_t device_id, const int32_t* a_cp, const int64_t* a_off, int64_t n_a, const int32_t* b_cp,
                                    const int64_t* b_off, int64_t n_b, const double* cost, double threshold, int32_t* nearest_out) {
    if (n_a < 0 || n_b < 0 || (n_a > 0 && !nearest_out) || (!cost && ((n_a > 0 && !a_off) || (n_b > 0 && !b_off))))
        return fail(RGBM_ERR_ARG, "rgbm_nearest_values: bad argument");
    return guarded([&]() {
        if (!cost) {
            check_pool_offsets(a_off, n_a, a_cp, "rgbm_nearest_values", "a");
            check_pool_offsets(b_off, n_b, b_cp, "rgbm_nearest_values", "b");
        }
        if (n_a == 0) return RGBM_OK;
        if (n_b == 0) { for (int64_t i = 0; i < n_a; ++i) nearest_out[i] = -1; return RGBM_OK; }
        if (n_b > 0x7FFFFFFF || n_a > NV_MAX_CELLS / n_b) throw std::invalid_argument("rgbm_nearest_values: the cost matrix holds more than 2^30 entries");
        use_device(device_id);
        StreamGuard sg;
        DevBuf<int32_t> d_out((size_t)n_a);
        const unsigned grid = nblocks(n_a, 4);               // one wave per row, four rows a workgroup
        if (cost) {
            DevBuf<double> d_cost((size_t)n_a * n_b);
            d_cost.upload(cost, (size_t)n_a * n_b, sg.s);
            hipLaunchKernelGGL(k_row_nearest<double>, dim3(grid), dim3(256), 0, sg.s, d_cost.p, (long long)n_a, (int)n_b, threshold, d_out.p);
            HIPCHK(hipGetLastError());
            d_out.download(nearest_out, (size_t)n_a, sg.s);
            HIPCHK(hipStreamSynchronize(sg.s));
        } else {
            DevBuf<int32_t> d_dist((size_t)n_a * n_b);       // stays in HBM: only the positions leave the device
            edit_distance_on_device(a_cp, a_off, n_a, b_cp, b_off, n_b, d_dist.p, sg.s);
            hipLaunchKernelGGL(k_row_nearest<int32_t>, dim3(grid), dim3(256), 0, sg.s, d_dist.p, (long long)n_a, (int)n_b, threshold, d_out.p);
            HIPCHK(hipGetLastError());
            d_out.download(nearest_out, (size_t)n_a, sg.s);
            HIPCHK(hipStreamSynchronize(sg.s));
        }
        return RGBM_OK;
    });
}

}  // extern "C"
