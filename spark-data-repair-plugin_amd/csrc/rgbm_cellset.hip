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
// The matrix, the column lists and the codes of the last emit are DevBufs of the table, not Scr slots: they outlive the detect calls in between.
#include "rgbm_prep.h"

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

bool cs_combine() {                   // RGBM_CELLSET_COMBINE=0: every lane its own atomic (tools/detect_only_bench.py times both forms); read per call
    const char* e = getenv("RGBM_CELLSET_COMBINE");
    return !(e && e[0] == '0');
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
        const long long m = t->n_cells, W = (long long)PBAL * ((t->n + PROWS - 1) / PROWS);
        if (cs_combine())
            hipLaunchKernelGGL(k_cs_or<CS_ROUNDS>, dim3(nblocks(m, 256)), dim3(256), 0, s, t->cell_rows.p, t->cell_cols.p, m, t->cs_d_pos.p, (long long)t->n,
                               (int)t->c, W, t->cs_bits.p);
        else
            hipLaunchKernelGGL(k_cs_or<0>, dim3(nblocks(m, 256)), dim3(256), 0, s, t->cell_rows.p, t->cell_cols.p, m, t->cs_d_pos.p, (long long)t->n,
                               (int)t->c, W, t->cs_bits.p);
        HIPCHK(hipGetLastError());
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

RGBM_EXPORT int rgbm_table_cellset_close(rgbm_table* t) {
    if (!t) return fail(RGBM_ERR_ARG, "rgbm_table_cellset_close: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        t->cs_bits.release(); t->cs_d_cols.release(); t->cs_d_pos.release();
        t->cs_n_cols = 0; t->cs_open = false;
        return RGBM_OK;
    });
}

}  // extern "C"
