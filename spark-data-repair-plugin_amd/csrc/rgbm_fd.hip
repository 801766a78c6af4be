// rgbm_fd.hip -- the measures of functional dependencies on the HBM-resident code table (a relational step; what the steps share is rgbm_prep.h):
//   fd_measures           one left-hand side X (0..11 columns) against many right-hand sides Y in one call: the distinct X-keys, and per Y the
//                         rows a largest-Y-per-group choice keeps (g3), the rows in groups of two or more Y values, the distinct (X, Y) keys
//                         (RepairMisc.discoverFunctionalDeps; repair/fd_codes.py is the statement)
#include "rgbm_prep.h"

namespace {

using namespace rgh;

// ---------------------------------------------------------------------------------------------
// Two routes per right-hand side, chosen by the size of the dense joint table span(X) x (n_codes[Y] + 1):
//   route 0 (LDS), at most FD_LDS counters:
//     k_fd_lds_count    grid (blocks, LDS right-hand sides): every workgroup counts the (X-key, Y digit) pairs of a grid-stride slice of the rows
//                       in 32-bit counters of its own in LDS and flushes the non-zero ones once, one integer atomic per counter and workgroup.
//     k_fd_lds_reduce   grid (LDS right-hand sides): one workgroup walks the span(X) rows of the joint table, L = 2^ceil(log2(n_codes[Y] + 1))
//                       lanes (64 at most, then striding) per X-key: size / max / distinct per key by segmented shuffles, the four sums per
//                       lane, one block reduction, plain stores (nobody else writes the sums of this right-hand side).
//   route 1 (hash), everything else:
//     k_fd_claim_x      once per call: every row claims the slot of its X-key, stores the slot and bumps the group's size.
//     k_fd_claim_xy     per right-hand side: the key slot * (n_codes[Y] + 1) + Y digit is claimed in a second table and counted.
//                       Both take FD_WG_ROWS rows per workgroup and combine its counts per slot in LDS (cache_add) before the global atomics.
//     k_fd_fold_xy      over the second table: atomicMax of the count into the group's maximum, +1 on its distinct-Y counter; the occupied
//                       slots are the distinct (X, Y) keys.
//     k_fd_sum_groups   over the first table: groups, sum of the maxima, sum of the sizes of groups with two or more Y values; each reduced over
//                       the workgroup before one 64-bit atomic.
// All arithmetic is integer: nothing depends on the order of arrival.  Every count is at most n < 2^31, so 32-bit counters hold it.
// ---------------------------------------------------------------------------------------------
constexpr int FD_LDS = 8192;              // 32-bit counters of a dense joint table that a workgroup keeps in LDS (route 0 up to here; as CC_LDS)
constexpr int FD_MAX_LHS = 11;            // left-hand-side columns: with the right-hand side, the 12 columns of a KeySpec
constexpr int FD_WG_ROWS = 4096;          // rows a workgroup of the claim kernels takes (a multiple of 256)
constexpr int FD_CACHE = 256;             // (slot, count) entries a workgroup of the claim kernels combines in LDS (a power of two)
constexpr int FD_SUMS = 4;                // groups, kept, violating, xy_groups
constexpr int FD_UNROLL = 4;              // rows per lane and grid-stride step of k_fd_lds_count

struct FdDesc { long long cnt_off; int32_t col, ny1, rhs, pad; };      // ny1 = n_codes[Y] + 1: the radix of Y's digit

__device__ __forceinline__ long long block_sum(long long v, long long* sh /* [4] */) {      // every lane calls it; the sum on thread 0
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    __syncthreads();                                                    // (sh may still be read from the call before)
    if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void k_fd_lds_count(const int32_t* __restrict__ codes, long long n, KeySpec ks, const FdDesc* __restrict__ desc,
                                                      unsigned* __restrict__ counts) {
    __shared__ unsigned h[FD_LDS];
    const FdDesc d = desc[blockIdx.y];
    const unsigned long long ny1 = (unsigned long long)d.ny1;
    unsigned long long cells = ny1;
    for (int c = 0; c < ks.ncols; ++c) cells *= ks.radix[c];            // <= FD_LDS by the route's rule
    const int m = (int)cells;
    for (int i = threadIdx.x; i < m; i += 256) h[i] = 0;
    __syncthreads();
    const int32_t* ycol = codes + (long long)d.col * n;
    for (long long base = (long long)blockIdx.x * (256 * FD_UNROLL); base < n; base += (long long)gridDim.x * (256 * FD_UNROLL)) {
#pragma unroll
        for (int s = 0; s < FD_UNROLL; ++s) {
            const long long r = base + (long long)s * 256 + threadIdx.x;
            if (r < n) {
                const unsigned long long k = row_key<true>(codes, n, ks, r) * ny1 + key_digit<true>(ycol[r], ny1);     // < cells: both sides clamped
                atomicAdd(&h[(unsigned)k], 1u);
            }
        }
    }
    __syncthreads();
    unsigned* cnt = counts + d.cnt_off;
    for (int i = threadIdx.x; i < m; i += 256) if (h[i]) atomicAdd(&cnt[i], h[i]);
}

__global__ __launch_bounds__(256) void k_fd_lds_reduce(const FdDesc* __restrict__ desc, const unsigned* __restrict__ counts, long long span,
                                                       long long* __restrict__ sums /* [.][FD_SUMS] */) {
    __shared__ long long sh[4];
    const FdDesc d = desc[blockIdx.x];
    const unsigned* cnt = counts + d.cnt_off;
    const int ny1 = d.ny1;
    int L = 1; while (L < ny1 && L < 64) L <<= 1;                       // lanes per X-key
    const int per_wg = 256 / L;
    const int sub = (int)threadIdx.x / L, l = (int)threadIdx.x % L;
    long long groups = 0, kept = 0, viol = 0, xy = 0;
    for (long long k0 = 0; k0 < span; k0 += per_wg) {                    // uniform over the block: every lane reaches the shuffles
        const long long k = k0 + sub;
        unsigned size = 0, mx = 0, dist = 0;
        if (k < span)
            for (int y = l; y < ny1; y += L) { const unsigned c = cnt[k * ny1 + y]; size += c; mx = max(mx, c); dist += c ? 1u : 0u; }
        for (int s = 1; s < L; s <<= 1) {
            size += (unsigned)__shfl_xor((int)size, s); dist += (unsigned)__shfl_xor((int)dist, s); mx = max(mx, (unsigned)__shfl_xor((int)mx, s));
        }
        if (l == 0 && size) { ++groups; kept += mx; xy += dist; if (dist >= 2) viol += size; }
    }
    groups = block_sum(groups, sh); kept = block_sum(kept, sh); viol = block_sum(viol, sh); xy = block_sum(xy, sh);
    if (threadIdx.x == 0) {
        long long* o = sums + (long long)d.rhs * FD_SUMS;
        o[0] = groups; o[1] = kept; o[2] = viol; o[3] = xy;
    }
}

// count[slot] += 1 for the rows of a workgroup, the rows of one slot leaving as ONE global atomic: a direct-mapped cache of FD_CACHE (slot,
// count) entries in LDS.  A slot that finds its entry taken by another adds on its own (many groups: little to combine, and no two rows
// meet on an address); few groups of millions of rows, which would otherwise send one atomic per wave and group to a handful of
// addresses, take the cache.  cache_open and cache_flush are called by every thread of the workgroup.
constexpr unsigned FD_NO_SLOT = 0xFFFFFFFFu;      // (a table of 2^32 slots has a slot of this number: its rows add on their own)
__device__ __forceinline__ void cache_open(unsigned* c_slot, unsigned* c_cnt) {
    for (int i = threadIdx.x; i < FD_CACHE; i += 256) { c_slot[i] = FD_NO_SLOT; c_cnt[i] = 0; }
    __syncthreads();
}
__device__ __forceinline__ void cache_add(unsigned* c_slot, unsigned* c_cnt, unsigned* __restrict__ count, unsigned slot) {
    const unsigned e = slot & (unsigned)(FD_CACHE - 1);
    const unsigned prev = atomicCAS(&c_slot[e], FD_NO_SLOT, slot);
    if (slot != FD_NO_SLOT && (prev == FD_NO_SLOT || prev == slot)) atomicAdd(&c_cnt[e], 1u);
    else atomicAdd(&count[slot], 1u);
}
__device__ __forceinline__ void cache_flush(const unsigned* c_slot, const unsigned* c_cnt, unsigned* __restrict__ count) {
    __syncthreads();
    for (int i = threadIdx.x; i < FD_CACHE; i += 256) if (c_cnt[i]) atomicAdd(&count[c_slot[i]], c_cnt[i]);
}

__global__ __launch_bounds__(256) void k_fd_claim_x(const int32_t* __restrict__ codes, long long n, KeySpec ks, unsigned long long* __restrict__ keys,
                                                    unsigned long long cap_mask, unsigned* __restrict__ gsize, unsigned* __restrict__ row_slot) {
    __shared__ unsigned c_slot[FD_CACHE], c_cnt[FD_CACHE];
    cache_open(c_slot, c_cnt);
    const long long r0 = (long long)blockIdx.x * FD_WG_ROWS;
    for (int k = 0; k < FD_WG_ROWS; k += 256) {
        const long long i = r0 + k + threadIdx.x;
        if (i >= n) break;
        const unsigned s32 = (unsigned)ht_claim(keys, cap_mask, row_key<true>(codes, n, ks, i));
        row_slot[i] = s32;
        cache_add(c_slot, c_cnt, gsize, s32);
    }
    cache_flush(c_slot, c_cnt, gsize);
}

__global__ __launch_bounds__(256) void k_fd_claim_xy(const int32_t* __restrict__ ycol, long long n, unsigned long long ny1,
                                                     const unsigned* __restrict__ row_slot, unsigned long long* __restrict__ keys,
                                                     unsigned long long cap_mask, unsigned* __restrict__ count) {
    __shared__ unsigned c_slot[FD_CACHE], c_cnt[FD_CACHE];
    cache_open(c_slot, c_cnt);
    const long long r0 = (long long)blockIdx.x * FD_WG_ROWS;
    for (int k = 0; k < FD_WG_ROWS; k += 256) {
        const long long i = r0 + k + threadIdx.x;
        if (i >= n) break;
        // slot < 2^32, ny1 <= 2^31: the key stays below 2^63 and never equals HT_EMPTY
        const unsigned s32 = (unsigned)ht_claim(keys, cap_mask, (unsigned long long)row_slot[i] * ny1 + key_digit<true>(ycol[i], ny1));
        cache_add(c_slot, c_cnt, count, s32);
    }
    cache_flush(c_slot, c_cnt, count);
}

__global__ __launch_bounds__(256) void k_fd_fold_xy(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ count,
                                                    unsigned long long cap, unsigned long long ny1, unsigned* __restrict__ gmax,
                                                    unsigned* __restrict__ gdist, long long* __restrict__ sums) {
    __shared__ long long sh[4];
    long long xy = 0;
    for (unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x; s < cap; s += (unsigned long long)gridDim.x * 256) {
        const unsigned long long k = keys[s];
        if (k == HT_EMPTY) continue;
        const unsigned long long g = k / ny1;                            // the group's slot in the first table
        atomicMax(&gmax[g], count[s]);
        atomicAdd(&gdist[g], 1u);
        ++xy;
    }
    xy = block_sum(xy, sh);
    if (threadIdx.x == 0 && xy) atomicAdd(reinterpret_cast<unsigned long long*>(&sums[3]), (unsigned long long)xy);
}

__global__ __launch_bounds__(256) void k_fd_sum_groups(const unsigned long long* __restrict__ keys, unsigned long long cap,
                                                       const unsigned* __restrict__ gsize, const unsigned* __restrict__ gmax,
                                                       const unsigned* __restrict__ gdist, long long* __restrict__ sums) {
    __shared__ long long sh[4];
    long long groups = 0, kept = 0, viol = 0;
    for (unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x; s < cap; s += (unsigned long long)gridDim.x * 256) {
        if (keys[s] == HT_EMPTY) continue;
        ++groups; kept += gmax[s];
        if (gdist[s] >= 2u) viol += gsize[s];
    }
    groups = block_sum(groups, sh); kept = block_sum(kept, sh); viol = block_sum(viol, sh);
    if (threadIdx.x == 0) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(sums);
        if (groups) atomicAdd(&o[0], (unsigned long long)groups);
        if (kept) atomicAdd(&o[1], (unsigned long long)kept);
        if (viol) atomicAdd(&o[2], (unsigned long long)viol);
    }
}

inline unsigned walk_blocks(unsigned long long cap) { return (unsigned)std::min<unsigned long long>((cap + 255) / 256, 256ull * 8ull); }

}  // namespace

extern "C" {

// scratch slots held together: TABLE_A (X keys) TABLE_B ((X, Y) keys) VALS (slot per row) IN_ROWS (size / max / distinct per group)
// IN_COLS ((X, Y) counts) COLS (the sums, the descriptors of the LDS right-hand sides) COUNTS (the dense joint tables of route 0)
RGBM_EXPORT int rgbm_table_fd_measures(rgbm_table* t, const int32_t* lhs_cols, int32_t n_lhs, const int32_t* rhs_cols, int32_t n_rhs,
                                       int64_t* groups_out, int64_t* kept_out, int64_t* violating_out, int64_t* xy_groups_out) {
    const char* const entry = "rgbm_table_fd_measures";
    if (!t || !rhs_cols || !groups_out || !kept_out || !violating_out || !xy_groups_out || n_lhs < 0 || n_lhs > FD_MAX_LHS || n_rhs < 1 ||
        (n_lhs > 0 && !lhs_cols))
        return fail(RGBM_ERR_ARG, "rgbm_table_fd_measures: bad argument (0..11 left-hand-side columns, at least one right-hand side)");
    if (const int rc = refuse_cols(*t, lhs_cols, n_lhs, true, nullptr, entry)) return rc;
    if (const int rc = refuse_cols(*t, rhs_cols, n_rhs, true, nullptr, entry)) return rc;
    for (int r = 0; r < n_rhs; ++r)
        for (int j = 0; j < n_lhs; ++j)
            if (rhs_cols[r] == lhs_cols[j]) return fail(RGBM_ERR_ARG, "rgbm_table_fd_measures: a right-hand side is also on the left-hand side");
    if (t->n >= (1ll << 31)) return fail(RGBM_ERR_PARAM, "rgbm_table_fd_measures: a table of 2^31 rows or more");
    return guarded([&]() {
        unsigned __int128 span = 1;
        const KeySpec ks = key_spec(*t, lhs_cols, n_lhs, entry, &span);                 // 2^63 combinations or more: RGBM_ERR_PARAM
        const long long n = t->n;
        std::vector<int32_t> routes((size_t)n_rhs);
        std::vector<FdDesc> lds;                                                        // the right-hand sides of route 0
        std::vector<int> hashed;                                                        // those of route 1
        long long n_cnt = 0;
        for (int r = 0; r < n_rhs; ++r) {
            const int32_t ny1 = std::max<int32_t>(t->n_codes[rhs_cols[r]], 0) + 1;
            routes[r] = span * (unsigned __int128)ny1 <= (unsigned __int128)FD_LDS ? 0 : 1;
            if (routes[r] == 0) { lds.push_back(FdDesc{n_cnt, rhs_cols[r], ny1, r, 0}); n_cnt += (long long)span * ny1; }
            else hashed.push_back(r);
        }
        std::vector<long long> sums((size_t)n_rhs * FD_SUMS, 0);
        if (n > 0) {
            use_device(t->device);
            std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
            // one buffer: the sums of every right-hand side, the descriptors behind them (both 8-byte aligned)
            const size_t sums_bytes = sums.size() * 8;
            unsigned char* d_head = scr<unsigned char>(*t, SCR_COLS, sums_bytes + lds.size() * sizeof(FdDesc));
            long long* d_sums = reinterpret_cast<long long*>(d_head);
            const FdDesc* d_desc = reinterpret_cast<const FdDesc*>(d_head + sums_bytes);
            HIPCHK(hipMemsetAsync(d_sums, 0, sums_bytes, s));
            if (!lds.empty()) {
                HIPCHK(hipMemcpyAsync(d_head + sums_bytes, lds.data(), lds.size() * sizeof(FdDesc), hipMemcpyHostToDevice, s));
                unsigned* d_cnt = scr<unsigned>(*t, SCR_COUNTS, (size_t)n_cnt);
                HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)n_cnt * 4, s));
                const unsigned nb = std::max(std::min<unsigned>(nblocks(n, 256 * FD_UNROLL * 4), 256u * 8u), 1u);
                hipLaunchKernelGGL(k_fd_lds_count, dim3(nb, (unsigned)lds.size()), dim3(256), 0, s, t->codes.p, n, ks, d_desc, d_cnt);
                HIPCHK(hipGetLastError());
                hipLaunchKernelGGL(k_fd_lds_reduce, dim3((unsigned)lds.size()), dim3(256), 0, s, d_desc, d_cnt, (long long)span, d_sums);
                HIPCHK(hipGetLastError());
            }
            if (!hashed.empty()) {
                // the first table holds at most min(n, span) keys, the second of a right-hand side at most min(n, span * (n_codes[Y] + 1))
                const unsigned long long cap1 = table_capacity(n, span);
                auto cap2_of = [&](int r) { return table_capacity(n, span * (unsigned __int128)(std::max<int32_t>(t->n_codes[rhs_cols[r]], 0) + 1)); };
                unsigned long long cap2_max = 0;
                for (const int r : hashed) cap2_max = std::max(cap2_max, cap2_of(r));
                unsigned long long* keys1 = scr<unsigned long long>(*t, SCR_TABLE_A, (size_t)cap1);
                unsigned long long* keys2 = scr<unsigned long long>(*t, SCR_TABLE_B, (size_t)cap2_max);
                unsigned* row_slot = scr<unsigned>(*t, SCR_VALS, (size_t)n);
                unsigned* gsize = scr<unsigned>(*t, SCR_IN_ROWS, (size_t)cap1 * 3);
                unsigned* gmax = gsize + cap1; unsigned* gdist = gmax + cap1;
                unsigned* cnt2 = scr<unsigned>(*t, SCR_IN_COLS, (size_t)cap2_max);
                HIPCHK(hipMemsetAsync(keys1, 0xFF, (size_t)cap1 * 8, s));
                HIPCHK(hipMemsetAsync(gsize, 0, (size_t)cap1 * 4, s));
                const unsigned nb = nblocks(n, FD_WG_ROWS);
                hipLaunchKernelGGL(k_fd_claim_x, dim3(nb), dim3(256), 0, s, t->codes.p, n, ks, keys1, cap1 - 1, gsize, row_slot);
                HIPCHK(hipGetLastError());
                for (const int r : hashed) {
                    const unsigned long long ny1 = (unsigned long long)std::max<int32_t>(t->n_codes[rhs_cols[r]], 0) + 1ull, cap2 = cap2_of(r);
                    HIPCHK(hipMemsetAsync(keys2, 0xFF, (size_t)cap2 * 8, s));
                    HIPCHK(hipMemsetAsync(cnt2, 0, (size_t)cap2 * 4, s));
                    HIPCHK(hipMemsetAsync(gmax, 0, (size_t)cap1 * 8, s));                // the maxima and the distinct counters behind them
                    long long* o = d_sums + (long long)r * FD_SUMS;
                    hipLaunchKernelGGL(k_fd_claim_xy, dim3(nb), dim3(256), 0, s, t->codes.p + (long long)rhs_cols[r] * n, n, ny1, row_slot, keys2,
                                       cap2 - 1, cnt2);
                    hipLaunchKernelGGL(k_fd_fold_xy, dim3(walk_blocks(cap2)), dim3(256), 0, s, keys2, cnt2, cap2, ny1, gmax, gdist, o);
                    hipLaunchKernelGGL(k_fd_sum_groups, dim3(walk_blocks(cap1)), dim3(256), 0, s, keys1, cap1, gsize, gmax, gdist, o);
                    HIPCHK(hipGetLastError());
                }
            }
            HIPCHK(hipMemcpyAsync(sums.data(), d_sums, sums_bytes, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        groups_out[0] = sums[0];
        for (int r = 0; r < n_rhs; ++r) {
            kept_out[r] = sums[(size_t)r * FD_SUMS + 1]; violating_out[r] = sums[(size_t)r * FD_SUMS + 2]; xy_groups_out[r] = sums[(size_t)r * FD_SUMS + 3];
        }
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        t->fd_routes.swap(routes);
        return RGBM_OK;
    });
}

// no device work: the route of every right-hand side of the table's last successful rgbm_table_fd_measures call, then the two limits
RGBM_EXPORT int rgbm_table_fd_measures_report(const rgbm_table* t, int32_t* out, int32_t n_rhs) {
    if (!out || n_rhs < 0 || (n_rhs > 0 && !t)) return fail(RGBM_ERR_ARG, "rgbm_table_fd_measures_report: bad argument");
    if (t) {
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        if ((size_t)n_rhs != t->fd_routes.size())
            return fail(RGBM_ERR_ARG, "rgbm_table_fd_measures_report: n_rhs is not the number of right-hand sides of the table's last rgbm_table_fd_measures call");
        std::copy(t->fd_routes.begin(), t->fd_routes.end(), out);
    }
    out[n_rhs] = FD_LDS; out[n_rhs + 1] = FD_MAX_LHS;
    return RGBM_OK;
}

}  // extern "C"
