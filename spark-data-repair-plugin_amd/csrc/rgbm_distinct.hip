// rgbm_distinct.hip -- a relational step on the HBM-resident code table (what the steps share is rgbm_prep.h):
// ---------------------------------------------------------------------------------------------
// distinct rows (rgbm_table_distinct_rows; the host statement is repair.pipeline.distinct_rows): the rows of the table grouped by
// equality over ALL columns (NULL is a value of its own), the groups in order of FIRST OCCURRENCE, a group of cnt rows kept as
// ceil(cnt / 255) consecutive copies whose multiplicities are 255, .., 255, cnt - 255 * (copies - 1).  The result is a function of the
// table alone: the hash, the slot a group lands in and the launch geometry never show in it.
//   k_dr_keys     the mixed-radix uint64 key words of every row, [W][n] (digit = code + 1, a code outside [0, n_codes) is NULL = 0;
//                 a new word starts where the next radix would pass 2^63 -- the words pipeline.distinct_rows builds)
//   k_dr_insert   open addressing over >= 2n slots.  A slot holds a ROW INDEX of its group (claimed with atomicCAS) and, once the kernel
//                 is done, the group's SMALLEST row index (integer atomicMin: order-free); count[slot] takes the group's rows (integer
//                 atomicAdd: order-free).  An occupied slot is compared word for word with the probing row's key.  Probe reads are
//                 agent-scope atomic loads (L2, never a stale L1 line); the probe loop ends after `cap` slots at the latest and then
//                 raises the error flag.  The count goes through wave_add (a table of a few distinct rows with millions of copies each);
//                 the atomicMin is skipped by every row that already sees a smaller index in the slot.
//   k_dr_mark     row i is its group's representative iff slot[row_slot[i]] == i  -> mask for the ordered compaction (k_flag<1>,
//                 k_scan_counts, k_emit: ascending representatives = groups by first occurrence)
//   k_dr_copies   copies per group; k_scan_counts over them gives every group's first output row
//   k_dr_source   per output row: the table row it copies and its multiplicity; the group's first output row is left with the
//                 representative for k_dr_inverse.  k_gather_rows then writes the codes.
// Algorithmic bytes per row: 4 B per column (keys) + 8 W (insert) + ~12 B of slot traffic + 4 B slot id, then 4 B per column and
// output row for the gather and 8 B for `inverse`.
// ---------------------------------------------------------------------------------------------
#include "rgbm_prep.h"

#include <cstring>

namespace {

using namespace rgh;

constexpr int DR_EMPTY = 0x7F7F7F7F;              // hipMemsetAsync(0x7F); above every row index (n <= 2^30)
constexpr unsigned DR_NO_SLOT = 0xFFFFFFFFu;
constexpr int DR_WAVE_ROUNDS = 8;                 // slots a wave combines before its remaining lanes add on their own

__global__ __launch_bounds__(256) void k_dr_keys(const int32_t* __restrict__ codes, long long n, int c, const unsigned long long* __restrict__ radix,
                                                 const int32_t* __restrict__ word_of, unsigned long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long k = 0; int w = 0;
    for (int cc = 0; cc < c; ++cc) {
        if (word_of[cc] != w) { keys[(long long)w * n + i] = k; k = 0; w = word_of[cc]; }
        k = k * radix[cc] + key_digit<true>(codes[(long long)cc * n + i], radix[cc]);
    }
    keys[(long long)w * n + i] = k;
}

__global__ __launch_bounds__(256) void k_dr_insert(const unsigned long long* __restrict__ keys, long long n, int W, int* __restrict__ slots,
                                                   unsigned* __restrict__ count, unsigned long long cap, unsigned* __restrict__ row_slot,
                                                   unsigned* __restrict__ err) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;                     // no early return: every lane takes part in the ballots below
    unsigned long long slot = 0; bool found = false;
    if (valid) {
        unsigned long long h = 0;
        for (int w = 0; w < W; ++w) h = mix64(h ^ keys[(long long)w * n + i]);
        const unsigned long long cap_mask = cap - 1ull;
        slot = h & cap_mask;
        for (unsigned long long probe = 0; probe < cap; ++probe) {
            int prev = __hip_atomic_load(&slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (prev == DR_EMPTY) { prev = atomicCAS(&slots[slot], DR_EMPTY, (int)i); if (prev == DR_EMPTY) { found = true; break; } }
            if (prev < 0 || (long long)prev >= n) break;                      // never a row index: give up, the flag says so
            bool same = true;
            for (int w = 0; w < W; ++w) same = same && keys[(long long)w * n + prev] == keys[(long long)w * n + i];
            if (same) { found = true; break; }
            slot = (slot + 1ull) & cap_mask;
        }
        if (!found) atomicOr(err, 1u);
        row_slot[i] = found ? (unsigned)slot : DR_NO_SLOT;
        if (found && __hip_atomic_load(&slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (int)i) atomicMin(&slots[slot], (int)i);
    }
    wave_add<DR_WAVE_ROUNDS>(count, (unsigned)slot, found);       // (the arrival rank is of no use here)
}

__global__ __launch_bounds__(256) void k_dr_mark(const int* __restrict__ slots, const unsigned* __restrict__ row_slot, long long n,
                                                 unsigned long long cap, uint8_t* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned s = row_slot[i];
    mask[i] = ((unsigned long long)s < cap && (long long)slots[s] == i) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_dr_copies(const long long* __restrict__ rep_rows, long long G, long long n, const unsigned* __restrict__ row_slot,
                                                   const unsigned* __restrict__ count, unsigned long long cap, unsigned* __restrict__ copies) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const long long r = rep_rows[g];
    const unsigned s = (r >= 0 && r < n) ? row_slot[r] : DR_NO_SLOT;
    const unsigned cnt = (unsigned long long)s < cap ? count[s] : 1u;
    copies[g] = (cnt + 254u) / 255u;
}

__global__ __launch_bounds__(256) void k_dr_source(const long long* __restrict__ rep_rows, const long long* __restrict__ goff, const unsigned* __restrict__ copies,
                                                   long long G, long long M, long long n, const unsigned* __restrict__ row_slot,
                                                   const unsigned* __restrict__ count, unsigned long long cap, long long* __restrict__ src_row,
                                                   uint8_t* __restrict__ mult, unsigned* __restrict__ first_out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= M) return;
    long long g = p;
    if (M != G) {                                 // some group has more than one copy: the last group that starts at or before p
        long long lo = 0, hi = G;
        while (lo < hi) { const long long mid = (lo + hi) >> 1; if (goff[mid] <= p) lo = mid + 1; else hi = mid; }
        g = lo > 0 ? lo - 1 : 0;
    }
    const long long r = rep_rows[g];
    const long long k = p - goff[g];
    const unsigned cp = copies[g];
    const unsigned s = (r >= 0 && r < n) ? row_slot[r] : DR_NO_SLOT;
    const unsigned cnt = (unsigned long long)s < cap ? count[s] : 1u;
    src_row[p] = (r >= 0 && r < n) ? r : 0;
    mult[p] = (uint8_t)(k + 1 == (long long)cp ? cnt - 255u * (cp - 1u) : 255u);
    if (k == 0 && r >= 0 && r < n) first_out[r] = (unsigned)p;
}

__global__ __launch_bounds__(256) void k_dr_inverse(const int* __restrict__ slots, const unsigned* __restrict__ row_slot, const unsigned* __restrict__ first_out,
                                                    long long n, unsigned long long cap, long long* __restrict__ inverse) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned s = row_slot[i];
    const long long r = (unsigned long long)s < cap ? (long long)slots[s] : i;
    inverse[i] = (r >= 0 && r < n) ? (long long)first_out[r] : -1;
}

}  // namespace

// the one copy of the pass: rgbm_table_distinct_rows and the distinct-row view of rgbm_table_train (rgbm.hip) both run it
rgh::DistinctOut rgh::distinct_rows_device(const rgbm_table& tab, int64_t* inverse_out, int64_t max_rows) {
    const rgbm_table* t = &tab;
    if (t->n > (1ll << 30)) throw distinct_cannot("rgbm_table_distinct_rows: more than 2^30 rows");
    if (t->has_mult) throw std::invalid_argument("rgbm_table_distinct_rows: the table carries row multiplicities itself (clear them first)");
    {
        use_device(t->device);
        const long long n = t->n; const int c = t->c;
        // the key words: as few as the radices need (pipeline.distinct_rows: a new word where the next radix would pass 2^63)
        std::vector<unsigned long long> radix((size_t)c); std::vector<int32_t> word_of((size_t)c);
        int W = 1; unsigned __int128 room = 1;
        for (int j = 0; j < c; ++j) {
            radix[j] = (unsigned long long)std::max<int32_t>(t->n_codes[j], 0) + 1ull;
            if (room * radix[j] >= ((unsigned __int128)1 << 63)) { ++W; room = 1; }
            room *= radix[j];
            word_of[j] = W - 1;
        }
        const unsigned long long cap = table_capacity(n);
        // everything the call allocates, with the output table at its largest (M <= n): slots + counts (8 B a slot); per row the slot id, the key
        // words, the compaction's mask and ballots, representative, copies, group offset, source row, first output row, inverse; the output's
        // codes and multiplicities.  Above half of the device memory the call is refused; a table that passes and still does not fit (other tables
        // and fits share the device) fails in the allocator with its own message.
        const unsigned long long work = cap * 8ull + (unsigned long long)n * (4ull + 8ull * W + 2ull + 8ull + 4ull + 8ull + 8ull + 4ull + 8ull + 4ull * c + 1ull);
        size_t mem_free = 0, mem_total = 0;
        HIPCHK(hipMemGetInfo(&mem_free, &mem_total));
        if (work > mem_total / 2)
            throw distinct_cannot("rgbm_table_distinct_rows: the working set (" + std::to_string(work >> 20) + " MB) exceeds half of the device memory");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        DevBuf<unsigned long long> d_radix((size_t)c), keys((size_t)W * n);
        DevBuf<int32_t> d_word((size_t)c);
        d_radix.upload(radix.data(), (size_t)c, s); d_word.upload(word_of.data(), (size_t)c, s);
        DevBuf<int> slots((size_t)cap); DevBuf<unsigned> count((size_t)cap), row_slot((size_t)n), err(1);
        HIPCHK(hipMemsetAsync(slots.p, 0x7F, (size_t)cap * 4, s));
        count.zero(s); err.zero(s);
        const unsigned nb = nblocks(n, 256);
        hipLaunchKernelGGL(k_dr_keys, dim3(nb), dim3(256), 0, s, t->codes.p, n, c, d_radix.p, d_word.p, keys.p);
        hipLaunchKernelGGL(k_dr_insert, dim3(nb), dim3(256), 0, s, keys.p, n, W, slots.p, count.p, cap, row_slot.p, err.p);
        HIPCHK(hipGetLastError());
        unsigned h_err = 0;
        HIPCHK(hipMemcpyAsync(&h_err, err.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (h_err) throw std::runtime_error("rgbm_table_distinct_rows: a probe sequence ran through the whole hash table");
        keys.release();
        // ascending representatives = the groups by first occurrence
        DevBuf<uint8_t> mask((size_t)n);
        hipLaunchKernelGGL(k_dr_mark, dim3(nb), dim3(256), 0, s, slots.p, row_slot.p, n, cap, mask.p);
        const long long nblk = (n + PROWS - 1) / PROWS;
        DevBuf<unsigned long long> ballots((size_t)nblk * PBAL); DevBuf<unsigned> bcount((size_t)nblk); DevBuf<long long> boff((size_t)nblk + 1);
        launch_flag_rows(mask.p, n, nblk, ballots.p, bcount.p, s);
        DevBuf<long long> rep_rows;
        const long long G = scan_emit(ballots.p, bcount.p, boff.p, nblk, 1, nullptr, s, [&](long long g, long long** rows, int32_t**) {
            if (g < 1 || g > n) throw std::runtime_error("rgbm_table_distinct_rows: inconsistent group count");
            rep_rows.alloc((size_t)g); *rows = rep_rows.p;
        });
        // output rows per group (the 255 split) and every group's first output row
        DevBuf<unsigned> copies((size_t)G); DevBuf<long long> goff((size_t)G + 1);
        hipLaunchKernelGGL(k_dr_copies, dim3(nblocks(G, 256)), dim3(256), 0, s, rep_rows.p, G, n, row_slot.p, count.p, cap, copies.p);
        launch_scan_counts(copies.p, G, goff.p, goff.p + G, s);
        HIPCHK(hipGetLastError());
        long long M = 0;
        HIPCHK(hipMemcpyAsync(&M, goff.p + G, sizeof(long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (M < G || M > n) throw std::runtime_error("rgbm_table_distinct_rows: inconsistent output row count");
        if (max_rows >= 0 && M > max_rows) { DistinctOut res; res.rows = M; return res; }      // (the view: not worth a table)
        std::unique_ptr<rgbm_table> o(new rgbm_table());
        o->device = t->device; o->n = M; o->c = c; o->n_codes = t->n_codes; o->col_values = t->col_values; o->col_kind = t->col_kind;
        o->codes.alloc((size_t)M * c); o->mult.alloc((size_t)M);
        DevBuf<long long> src_row((size_t)M); DevBuf<unsigned> first_out((size_t)n);
        hipLaunchKernelGGL(k_dr_source, dim3(nblocks(M, 256)), dim3(256), 0, s, rep_rows.p, goff.p, copies.p, G, M, n, row_slot.p, count.p, cap, src_row.p,
                           o->mult.p, first_out.p);
        launch_gather_rows(t->codes.p, n, c, o->codes.p, M, src_row.p, s);
        HIPCHK(hipGetLastError());
        if (inverse_out) {
            DevBuf<long long> inv((size_t)n);
            hipLaunchKernelGGL(k_dr_inverse, dim3(nb), dim3(256), 0, s, slots.p, row_slot.p, first_out.p, n, cap, inv.p);
            HIPCHK(hipGetLastError());
            static_assert(sizeof(long long) == sizeof(int64_t), "row positions are 64-bit");
            HIPCHK(hipMemcpyAsync(inverse_out, inv.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        HIPCHK(hipStreamSynchronize(s));
        o->has_mult = true; o->mult_total = n;
        DistinctOut res; res.rows = M; res.tab = std::move(o);
        return res;
    }
}

extern "C" {

RGBM_EXPORT int rgbm_table_distinct_rows(const rgbm_table* t, rgbm_table** out, int64_t* n_out, int64_t* inverse_out) {
    if (!t || !out || !n_out || t->n <= 0 || t->c <= 0) return fail(RGBM_ERR_ARG, "rgbm_table_distinct_rows: bad argument");
    return guarded([&]() {
        DistinctOut res = distinct_rows_device(*t, inverse_out, -1);
        *n_out = res.rows;
        *out = res.tab.release();
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_read_row_multiplicity(const rgbm_table* t, uint8_t* mult_out) {
    if (!t || !mult_out) return fail(RGBM_ERR_ARG, "rgbm_table_read_row_multiplicity: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        if (!t->has_mult) { memset(mult_out, 1, (size_t)t->n); return RGBM_OK; }
        HIPCHK(hipMemcpy(mult_out, t->mult.p, (size_t)t->n, hipMemcpyDeviceToHost));
        return RGBM_OK;
    });
}

}  // extern "C"
