// rgbm_cellset.hip -- the CELL SET of a resident table: the union of detector results, kept on the device between the detect calls
// (DESIGN.md 5n).  A detector leaves its cells in the table's cell list; the set ORs them into a bit matrix of its own and emits the
// union once, ordered like every other result (position in the column list, then ascending row), with the codes the cells hold.
//
//   layout   n_cols x W 64-bit words, W = 64 * ceil(n / PROWS): bit (j, r) is bit r & 63 of word j * W + (r >> 6).  With PROWS = 64 x 64 that
//            IS the compaction's ballot layout (flags_to_ballots: entry e = j * nblk + b holds 64 words, word q the rows [b * PROWS + 64 q, +64)),
//            so scan_emit emits the matrix as it lies; the words beyond row n stay zero (k_cs_or never sets a bit of a row outside the table).
//   k_cs_or      one lane per cell of the cell list: 64-bit atomicOr on the word, the lanes of a wave that hold the same word first ORed
//                together (detector results are sorted by column and row, so a wave mostly holds one or two words)
//   k_cs_count   bcount of every (block, column) entry: popcount over its 64 words, one wave per entry
//   k_cs_gather  codes[col * n + row] of every emitted cell, as it lies
//   k_cs_drop_weak  one lane per emitted cell of ONE column: the weak flag of rgbm_domain.h's cell_domain; a set flag clears the cell's bit (atomicAnd:
//                several weak cells share a word)
//   k_cs_null    one wave per (block, column) entry: NULL into codes at every set bit, the zero words skipped
//   k_cs_or_cols the columns of the set ORed word by word: the ballots of the rows that hold a cell
// The matrix, the column lists and the codes of the last emit are DevBufs of the table, not Scr slots: they outlive the detect calls in between.
#include "rgbm_domain.h"

namespace {

using namespace rgh;

static_assert(PROWS == 64 * PBAL && PBAL == 64, "the cell set's word index j * W + (r >> 6) is the ballot layout only while a block holds 64 ballots");

constexpr int CS_ROUNDS = 2;      // leader rounds of k_cs_or before the remaining lanes add on their own (a sorted result: one or two words per wave)

// ROUNDS > 0: the lanes of a wave that hold the same word are ORed together (6 xor-shuffle steps over the wave) and their leader issues one
// atomic; ROUNDS == 0: every lane issues its own (measured on a sorted 160M-cell result: 0.77 ms with the combine, 9.3 ms without).  pos [c]: position of a column in the set, -1 = not in it (such a cell is skipped, and so is
// a cell outside the table: join semantics).
template <int ROUNDS>
__global__ __launch_bounds__(256) void k_cs_or(const long long* __restrict__ rows, const int32_t* __restrict__ cols, long long m,
                                               const int32_t* __restrict__ pos, long long n, int c, long long W,
                                               unsigned long long* __restrict__ bits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool active = false; long long w = -1; unsigned long long bit = 0;
    if (i < m) {
        const long long r = rows[i]; const int cc = cols[i];
        if (r >= 0 && r < n && cc >= 0 && cc < c) {
            const int p = pos[cc];
            if (p >= 0) { active = true; w = (long long)p * W + (r >> 6); bit = 1ull << (r & 63); }
        }
    }
    if (ROUNDS == 0) { if (active) atomicOr(&bits[w], bit); return; }
    const int lane = lane_id();
    unsigned long long pend = __ballot(active);
    for (int round = 0; round < ROUNDS && pend; ++round) {
        const int leader = __ffsll((long long)pend) - 1;
        const long long s = __shfl(w, leader);
        const bool mine = active && w == s;
        const unsigned long long same = __ballot(mine);
        unsigned long long v = mine ? bit : 0ull;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) v |= __shfl_xor(v, d);
        if (lane == leader) atomicOr(&bits[s], v);
        pend &= ~same;
    }
    if ((pend >> lane) & 1ull) atomicOr(&bits[w], bit);
}

// bcount[e] = set bits of entry e's 64 words; one wave per entry, 4 entries per workgroup
__global__ __launch_bounds__(PB) void k_cs_count(const unsigned long long* __restrict__ bits, long long m, unsigned* __restrict__ bcount) {
    const long long e = (long long)blockIdx.x * (PB / 64) + (threadIdx.x >> 6);
    if (e >= m) return;                                   // (whole waves leave: e is uniform over a wave)
    unsigned cnt = (unsigned)__popcll(bits[e * PBAL + lane_id()]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) cnt += (unsigned)__shfl_xor((int)cnt, d);
    if (lane_id() == 0) bcount[e] = cnt;
}

// the emitted cells lie inside the table by construction (k_cs_or, the matrix's zero tail)
__global__ __launch_bounds__(256) void k_cs_gather(const int32_t* __restrict__ codes, long long n, const long long* __restrict__ rows,
                                                   const int32_t* __restrict__ cols, long long m, int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    out[i] = codes[(long long)cols[i] * n + rows[i]];
}

// cell i = (rows [i], target) is one of the set's column `target` (its words at `bits`): weak -> its bit leaves the set; *n_weak counts them
__global__ __launch_bounds__(256) void k_cs_drop_weak(const int32_t* __restrict__ codes, long long n, int target, int d_a,
                                                      const long long* __restrict__ rows, long long m, const unsigned long long* __restrict__ joint,
                                                      const DomAttr* __restrict__ attrs, int k, const int32_t* __restrict__ colinfo,
                                                      const long long* __restrict__ lut_off, const int32_t* __restrict__ luts,
                                                      const uint8_t* __restrict__ single_ok, double beta, double row_count,
                                                      unsigned long long* __restrict__ bits, unsigned long long* __restrict__ n_weak) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool weak = false;
    if (i < m) {
        const long long r = rows[i];                      // inside the table: an emitted row
        weak = cell_domain(codes, n, target, d_a, r, joint, attrs, k, colinfo, lut_off, luts, single_ok, beta, row_count, nullptr).weak;
        if (weak) atomicAnd(&bits[r >> 6], ~(1ull << (r & 63)));
    }
    const unsigned long long w = __ballot(weak);
    if (lane_id() == 0 && w) atomicAdd(n_weak, (unsigned long long)__popcll(w));
}

// entry e = p * nblk + b of the matrix (one wave each, 4 per workgroup): codes[cols[p]][row] = NULL for every set bit; *n_cells counts them
__global__ __launch_bounds__(PB) void k_cs_null(const unsigned long long* __restrict__ bits, long long m, long long nblk, const int32_t* __restrict__ cols,
                                                int32_t* __restrict__ codes, long long n, unsigned long long* __restrict__ n_cells) {
    const long long e = (long long)blockIdx.x * (PB / 64) + (threadIdx.x >> 6);
    if (e >= m) return;                                   // (whole waves leave: e is uniform over a wave)
    const int lane = lane_id();
    const unsigned long long word = bits[e * PBAL + lane];
    unsigned long long nz = __ballot(word != 0ull);
    if (!nz) return;
    const long long col = cols[e / nblk], row0 = (e % nblk) * PROWS;
    unsigned cnt = (unsigned)__popcll(word);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) cnt += (unsigned)__shfl_xor((int)cnt, d);
    if (lane == 0) atomicAdd(n_cells, (unsigned long long)cnt);
    while (nz) {
        const int q = __ffsll((long long)nz) - 1;
        const unsigned long long wq = __shfl(word, q);
        const long long r = row0 + (long long)q * 64 + lane;
        if (((wq >> lane) & 1ull) && r < n) codes[col * n + r] = -1;
        nz &= nz - 1ull;
    }
}

// out [W] = the OR of the set's n_cols columns, word by word
__global__ __launch_bounds__(256) void k_cs_or_cols(const unsigned long long* __restrict__ bits, long long W, int n_cols, unsigned long long* __restrict__ out) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    unsigned long long v = 0ull;
    for (int p = 0; p < n_cols; ++p) v |= bits[(long long)p * W + w];
    out[w] = v;
}

bool cs_combine() {                   // RGBM_CELLSET_COMBINE=0: every lane its own atomic (tools/detect_only_bench.py times both forms); read per call
    const char* e = getenv("RGBM_CELLSET_COMBINE");
    return !(e && e[0] == '0');
}

// k_cs_or over m cells (device arrays) into the open set, in the form cs_combine() chooses; left in flight on s
void launch_cs_or(rgbm_table& t, const long long* d_rows, const int32_t* d_cols, long long m, hipStream_t s) {
    const long long W = (long long)PBAL * ((t.n + PROWS - 1) / PROWS);
    if (cs_combine())
        hipLaunchKernelGGL(k_cs_or<CS_ROUNDS>, dim3(nblocks(m, 256)), dim3(256), 0, s, d_rows, d_cols, m, t.cs_d_pos.p, (long long)t.n, (int)t.c, W, t.cs_bits.p);
    else
        hipLaunchKernelGGL(k_cs_or<0>, dim3(nblocks(m, 256)), dim3(256), 0, s, d_rows, d_cols, m, t.cs_d_pos.p, (long long)t.n, (int)t.c, W, t.cs_bits.p);
    HIPCHK(hipGetLastError());
}

}  // namespace

extern "C" {

RGBM_EXPORT int rgbm_table_cellset_open(rgbm_table* t, const int32_t* cols, int32_t n_cols) {
    if (!t || !cols || n_cols < 1 || n_cols > t->c) return fail(RGBM_ERR_ARG, "rgbm_table_cellset_open: bad argument (1 <= n_cols <= columns)");
    if (const int rc = refuse_cols(*t, cols, n_cols, true, nullptr, "rgbm_table_cellset_open")) return rc;
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const long long W = (long long)PBAL * ((t->n + PROWS - 1) / PROWS);
        std::vector<int32_t> pos((size_t)t->c, -1);
        for (int j = 0; j < n_cols; ++j) pos[cols[j]] = j;
        DevBuf<unsigned long long> bits((size_t)n_cols * (size_t)W); DevBuf<int32_t> d_cols((size_t)n_cols), d_pos((size_t)t->c);
        bits.zero(s); d_cols.upload(cols, (size_t)n_cols, s); d_pos.upload(pos.data(), pos.size(), s);
        HIPCHK(hipStreamSynchronize(s));
        t->cs_bits.swap(bits); t->cs_d_cols.swap(d_cols); t->cs_d_pos.swap(d_pos);
        t->cs_cols.assign(cols, cols + n_cols);
        t->cs_n_cols = n_cols; t->cs_open = true; t->cs_emitted = false;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_cellset_add(rgbm_table* t) {
    if (!t) return fail(RGBM_ERR_ARG, "rgbm_table_cellset_add: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!t->cs_open) throw std::invalid_argument("rgbm_table_cellset_add: no open cell set");
        if (t->n_cells > 0 && !t->cell_cols.p) throw std::invalid_argument("rgbm_table_cellset_add: the last result is a row list (no columns)");
        if (t->n_cells == 0) return RGBM_OK;
        launch_cs_or(*t, t->cell_rows.p, t->cell_cols.p, t->n_cells, s);
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

// scratch slots held together: | BCOUNT BOFF (the compaction's; its ballots are the set itself)
RGBM_EXPORT int rgbm_table_cellset_emit(rgbm_table* t, int64_t* n_cells_out, int64_t* counts_out) {
    if (!t || !n_cells_out) return fail(RGBM_ERR_ARG, "rgbm_table_cellset_emit: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!t->cs_open) throw std::invalid_argument("rgbm_table_cellset_emit: no open cell set");
        const int ncols = t->cs_n_cols;
        const long long nblk = (t->n + PROWS - 1) / PROWS, m = nblk * ncols;
        const Ballots b{t->cs_bits.p, scr<unsigned>(*t, SCR_BCOUNT, (size_t)m), scr<long long>(*t, SCR_BOFF, (size_t)m + 1), nblk, ncols};
        hipLaunchKernelGGL(k_cs_count, dim3(nblocks(m, PB / 64)), dim3(PB), 0, s, b.ballots, m, b.bcount);
        HIPCHK(hipGetLastError());
        t->cs_emitted = false;
        const long long total = emit_to_table(*t, b, t->cs_d_cols.p, s);
        if (t->cs_codes.n < (size_t)std::max<long long>(total, 1)) t->cs_codes.alloc((size_t)std::max<long long>(total, 1) * 5 / 4);
        if (total > 0) hipLaunchKernelGGL(k_cs_gather, dim3(nblocks(total, 256)), dim3(256), 0, s, t->codes.p, (long long)t->n, t->cell_rows.p, t->cell_cols.p, total, t->cs_codes.p);
        HIPCHK(hipGetLastError());
        std::vector<long long> off;
        if (counts_out) { off.resize((size_t)m + 1); HIPCHK(hipMemcpyAsync(off.data(), b.off, off.size() * 8, hipMemcpyDeviceToHost, s)); }
        HIPCHK(hipStreamSynchronize(s));
        if (counts_out) for (int j = 0; j < ncols; ++j) counts_out[j] = (int64_t)(off[(size_t)(j + 1) * nblk] - off[(size_t)j * nblk]);
        t->cs_emitted = true; t->cs_emit_version = t->cell_version;
        *n_cells_out = total;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_cells_fetch_codes(const rgbm_table* t, int32_t* codes_out) {
    if (!t) return fail(RGBM_ERR_ARG, "rgbm_table_cells_fetch_codes: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        if (!t->cs_emitted || t->cs_emit_version != t->cell_version)
            throw std::invalid_argument("rgbm_table_cells_fetch_codes: the cell list is not the result of rgbm_table_cellset_emit");
        if (t->n_cells > 0) {
            if (!codes_out) throw std::invalid_argument("rgbm_table_cells_fetch_codes: codes_out missing");
            HIPCHK(hipMemcpy(codes_out, t->cs_codes.p, (size_t)t->n_cells * 4, hipMemcpyDeviceToHost));
        }
        return RGBM_OK;
    });
}

// scratch slots held together: IN_ROWS IN_COLS
RGBM_EXPORT int rgbm_table_cellset_add_cells(rgbm_table* t, const int64_t* rows, const int32_t* cols, int64_t n_cells) {
    if (!t || n_cells < 0 || (n_cells > 0 && (!rows || !cols))) return fail(RGBM_ERR_ARG, "rgbm_table_cellset_add_cells: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!t->cs_open) throw std::invalid_argument("rgbm_table_cellset_add_cells: no open cell set");
        if (n_cells == 0) return RGBM_OK;
        static_assert(sizeof(long long) == sizeof(int64_t), "row positions are 64-bit");
        const long long* d_rows = scr_upload<long long>(*t, SCR_IN_ROWS, reinterpret_cast<const long long*>(rows), (size_t)n_cells, s);
        const int32_t* d_cols = scr_upload<int32_t>(*t, SCR_IN_COLS, cols, (size_t)n_cells, s);
        launch_cs_or(*t, d_rows, d_cols, (long long)n_cells, s);
        HIPCHK(hipStreamSynchronize(s));      // the caller's arrays are read by the async copies
        return RGBM_OK;
    });
}

// scratch slots held together: TABLE_A (attributes) COLS (single_ok) VALS (the weak counter) | BCOUNT BOFF (the compaction's; its ballots are the column's words)
RGBM_EXPORT int rgbm_table_cellset_drop_weak(rgbm_table* t, int32_t target_col, const int32_t* pair_idx, int32_t k, const int64_t* min_cnt,
                                             const uint8_t* single_ok, double beta, int64_t row_count, int64_t* n_cells_out, int64_t* n_weak_out) {
    if (!t || target_col < 0 || target_col >= t->c || k < 0 || (k > 0 && (!pair_idx || !min_cnt)) || !single_ok || row_count <= 0 || !n_cells_out ||
        !n_weak_out)
        return fail(RGBM_ERR_ARG, "rgbm_table_cellset_drop_weak: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!t->cs_open) throw std::invalid_argument("rgbm_table_cellset_drop_weak: no open cell set");
        const std::vector<DomAttr> attrs = dom_attrs(*t, target_col, pair_idx, k, min_cnt, "rgbm_table_cellset_drop_weak");
        const int p = (int)(std::find(t->cs_cols.begin(), t->cs_cols.end(), target_col) - t->cs_cols.begin());
        if (p >= t->cs_n_cols) throw std::invalid_argument("rgbm_table_cellset_drop_weak: the target is not a column of the cell set");
        // everything that refuses is behind us: from here on the cell list is replaced
        const int d_a = t->pc_nbins[target_col];
        const long long nblk = (t->n + PROWS - 1) / PROWS, W = (long long)PBAL * nblk;
        unsigned long long* col_bits = t->cs_bits.p + (long long)p * W;          // a one-column Ballots as it lies
        const Ballots b{col_bits, scr<unsigned>(*t, SCR_BCOUNT, (size_t)nblk), scr<long long>(*t, SCR_BOFF, (size_t)nblk + 1), nblk, 1};
        hipLaunchKernelGGL(k_cs_count, dim3(nblocks(nblk, PB / 64)), dim3(PB), 0, s, b.ballots, nblk, b.bcount);
        HIPCHK(hipGetLastError());
        const long long total = emit_to_table(*t, b, t->cs_d_cols.p + p, s);
        unsigned long long weak = 0;
        if (total > 0) {
            const DomAttr* d_attrs = scr_upload<DomAttr>(*t, SCR_TABLE_A, attrs.data(), attrs.size(), s);
            const uint8_t* d_ok = scr_upload<uint8_t>(*t, SCR_COLS, single_ok, (size_t)d_a, s);
            unsigned long long* d_weak = scr<unsigned long long>(*t, SCR_VALS, 1);
            HIPCHK(hipMemsetAsync(d_weak, 0, 8, s));
            hipLaunchKernelGGL(k_cs_drop_weak, dim3(nblocks(total, 256)), dim3(256), 0, s, t->codes.p, (long long)t->n, (int)target_col, d_a, t->cell_rows.p,
                               total, t->pc_counts.p, d_attrs, (int)k, t->pc_bins.p, t->pc_lut_off.p, t->pc_luts.p, d_ok, beta, (double)row_count,
                               col_bits, d_weak);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&weak, d_weak, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        *n_cells_out = total; *n_weak_out = (int64_t)weak;
        return RGBM_OK;
    });
}

// scratch slots held together: VALS (the cell counter)
RGBM_EXPORT int rgbm_table_cellset_null(rgbm_table* t, int64_t* n_cells_out) {
    if (!t || !n_cells_out) return fail(RGBM_ERR_ARG, "rgbm_table_cellset_null: bad argument");
    return guarded([&]() {
        use_device(t->device);
        rgh::ViewWrite view_wr(t);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!t->cs_open) throw std::invalid_argument("rgbm_table_cellset_null: no open cell set");
        const long long nblk = (t->n + PROWS - 1) / PROWS, m = nblk * t->cs_n_cols;
        unsigned long long* d_cnt = scr<unsigned long long>(*t, SCR_VALS, 1);
        unsigned long long cnt = 0;
        HIPCHK(hipMemsetAsync(d_cnt, 0, 8, s));
        if (m > 0) hipLaunchKernelGGL(k_cs_null, dim3(nblocks(m, PB / 64)), dim3(PB), 0, s, t->cs_bits.p, m, nblk, t->cs_d_cols.p, t->codes.p, (long long)t->n, d_cnt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        *n_cells_out = (int64_t)cnt;
        return RGBM_OK;
    });
}

// scratch slots held together: | BALLOTS BCOUNT BOFF
RGBM_EXPORT int rgbm_table_cellset_rows(rgbm_table* t, int64_t* n_rows_out) {
    if (!t || !n_rows_out) return fail(RGBM_ERR_ARG, "rgbm_table_cellset_rows: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!t->cs_open) throw std::invalid_argument("rgbm_table_cellset_rows: no open cell set");
        const Ballots b = table_ballots(*t, 1);
        const long long W = (long long)PBAL * b.nblk;
        hipLaunchKernelGGL(k_cs_or_cols, dim3(nblocks(W, 256)), dim3(256), 0, s, t->cs_bits.p, W, (int)t->cs_n_cols, b.ballots);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_cs_count, dim3(nblocks(b.nblk, PB / 64)), dim3(PB), 0, s, b.ballots, b.nblk, b.bcount);
        HIPCHK(hipGetLastError());
        *n_rows_out = emit_to_table(*t, b, nullptr, s);
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_cellset_close(rgbm_table* t) {
    if (!t) return fail(RGBM_ERR_ARG, "rgbm_table_cellset_close: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        t->cs_bits.release(); t->cs_d_cols.release(); t->cs_d_pos.release();
        t->cs_cols.clear(); t->cs_n_cols = 0; t->cs_open = false;
        return RGBM_OK;
    });
}

}  // extern "C"
