// rgbm_colstats.hip -- column statistics of the HBM-resident code table (a relational step; what the steps share is rgbm_prep.h):
//   column_stats          distinct / NULL counts, min / max, value lengths and equi-height histogram edges of many columns in one call
//                         (RepairMiscApi.computeAndGetStats in code space; repair/table_stats.py is the statement)
#include "rgbm_prep.h"

namespace {

using namespace rgh;

// ---------------------------------------------------------------------------------------------
// column statistics (rgbm_table_column_stats; the statement is repair/table_stats.py column_stats): the counts of every listed column in one
// launch, then one workgroup per column reduces its counts to six numbers and the histogram edges.  The counts never leave the device.
//   k_colstat_count   grid (blocks, listed columns): the two regimes of k_count_codes (32-bit LDS counters flushed with 64-bit atomics up to CC_LDS
//                     codes, 64-bit atomics to HBM above); NULL rows per wave by ballot / popcount, one atomic per wave.  4 B per (row, column).
//   k_colstat_reduce  grid (listed columns): walks the counts in chunks of CS_CHUNK codes (CS_ITEMS consecutive codes per lane), a block scan per
//                     chunk and a running sum between chunks: distinct, min, max, len_sum, len_max, and the first code at which the cumulative
//                     count reaches each target rank  ceil(i * m / n_bins)  (m = non-NULL rows; the ranks wait in LDS, and a chunk that no rank
//                     falls into -- all but n_bins of them at most -- skips the selection).  8 B per code, + 4 B with a length LUT.
// ---------------------------------------------------------------------------------------------
struct CsDesc { long long cnt_off, lut_off; int32_t col, n_codes; };       // lut_off < 0: no length LUT
constexpr int CS_UNROLL = 4;              // independent coalesced loads in flight per lane
constexpr int CS_ITEMS = 8;               // consecutive codes per lane and chunk
constexpr int CS_CHUNK = 256 * CS_ITEMS;
constexpr int CS_STATS = 6;               // nulls, distinct, min_code, max_code, len_sum, len_max
constexpr int CS_MAX_BINS = 254;

__global__ __launch_bounds__(256) void k_colstat_count(const int32_t* __restrict__ codes, long long n, const CsDesc* __restrict__ desc,
                                                       unsigned long long* __restrict__ counts, unsigned long long* __restrict__ stats) {
    __shared__ unsigned h[CC_LDS];
    const CsDesc d = desc[blockIdx.y];
    const int nc = d.n_codes;
    const int32_t* col = codes + (long long)d.col * n;
    unsigned long long* cnt = counts + d.cnt_off;
    const bool lds = nc <= CC_LDS;
    if (lds) { for (int i = threadIdx.x; i < nc; i += 256) h[i] = 0; __syncthreads(); }
    unsigned long long nulls = 0;        // of this wave (every lane holds the same number)
    for (long long base = (long long)blockIdx.x * (256 * CS_UNROLL); base < n; base += (long long)gridDim.x * (256 * CS_UNROLL)) {   // uniform over the block
        int v[CS_UNROLL];
#pragma unroll
        for (int s = 0; s < CS_UNROLL; ++s) {
            const long long r = base + (long long)s * 256 + threadIdx.x;
            v[s] = r < n ? col[r] : 0;
        }
#pragma unroll
        for (int s = 0; s < CS_UNROLL; ++s) {
            const bool in = base + (long long)s * 256 + threadIdx.x < n;
            const bool null = in && (v[s] < 0 || v[s] >= nc);
            nulls += (unsigned long long)__popcll(__ballot(null));
            if (in && !null) { if (lds) atomicAdd(&h[v[s]], 1u); else atomicAdd(&cnt[v[s]], 1ull); }
        }
    }
    if (lane_id() == 0 && nulls) atomicAdd(&stats[(long long)blockIdx.y * CS_STATS], nulls);
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < nc; i += 256) if (h[i]) atomicAdd(&cnt[i], (unsigned long long)h[i]);
    }
}

__global__ __launch_bounds__(256) void k_colstat_reduce(const CsDesc* __restrict__ desc, const unsigned long long* __restrict__ counts,
                                                        const int32_t* __restrict__ luts, long long n, int n_bins,
                                                        long long* __restrict__ stats /* [.][CS_STATS], nulls filled in */,
                                                        int32_t* __restrict__ edges /* [.][n_bins + 1] or null */) {
    __shared__ long long wsum[2][4];
    __shared__ long long red_sum[2][4];
    __shared__ int red_i[3][4];
    __shared__ long long rank[CS_MAX_BINS + 1];           // rank[i] = ceil(i * m / n_bins), i = 1 .. n_bins: ascending
    const CsDesc d = desc[blockIdx.x];
    const int nc = d.n_codes;
    const unsigned long long* cnt = counts + d.cnt_off;
    const int32_t* lut = d.lut_off >= 0 ? luts + d.lut_off : nullptr;
    long long* st = stats + (long long)blockIdx.x * CS_STATS;
    int32_t* ed = edges ? edges + (long long)blockIdx.x * (n_bins + 1) : nullptr;
    const long long m = n - st[0];                        // non-NULL rows
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    if (ed) {
        for (int i = threadIdx.x; i <= n_bins; i += 256) { ed[i] = -1; rank[i] = ((long long)i * m + n_bins - 1) / n_bins; }
        __syncthreads();
    }
    const bool select = ed && m > 0;
    long long distinct = 0, len_sum = 0, carry = 0;
    int mn = 0x7FFFFFFF, mx = -1, len_max = 0;
    int buf = 0, next_edge = 1;                           // next_edge (uniform): the first edge that no earlier chunk has placed
    long long c[CS_ITEMS], c_next[CS_ITEMS];
    int l[CS_ITEMS], l_next[CS_ITEMS];
    auto load = [&](long long chunk, long long (&cc)[CS_ITEMS], int (&ll)[CS_ITEMS]) {
        const long long c0 = chunk + (long long)threadIdx.x * CS_ITEMS;
#pragma unroll
        for (int k = 0; k < CS_ITEMS; ++k) { const bool in = c0 + k < nc; cc[k] = in ? (long long)cnt[c0 + k] : 0; ll[k] = in && lut ? lut[c0 + k] : 0; }
    };
    load(0, c, l);
    for (long long chunk = 0; chunk < nc; chunk += CS_CHUNK, buf ^= 1) {
        load(chunk + CS_CHUNK, c_next, l_next);           // the next chunk's loads are in flight while this one is scanned (beyond the end: zeros, no load)
        const long long c0 = chunk + (long long)threadIdx.x * CS_ITEMS;
        long long mine = 0;
#pragma unroll
        for (int k = 0; k < CS_ITEMS; ++k) mine += c[k];
        long long incl = mine;                            // inclusive scan of `mine` over the wave, then over the block
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) { const long long o = __shfl_up(incl, s); if (lane >= s) incl += o; }
        if (lane == 63) wsum[buf][wave] = incl;
        __syncthreads();                                  // (wsum is double buffered: one barrier per chunk)
        long long before = carry + incl - mine, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const long long t = wsum[buf][w]; if (w < wave) before += t; all += t; }
        carry += all;
        // an edge lands in this chunk iff the first unplaced rank is within the rows counted so far (uniform over the block)
        const bool here = select && next_edge <= n_bins && rank[next_edge] <= carry;
        int e = next_edge;
        if (here) while (e <= n_bins && rank[e] <= before) ++e;         // placed by the codes before this lane's
#pragma unroll
        for (int k = 0; k < CS_ITEMS; ++k) {
            if (c[k] <= 0) continue;
            const int code = (int)(c0 + k);
            ++distinct; mn = min(mn, code); mx = max(mx, code);
            len_sum += c[k] * (long long)l[k]; len_max = max(len_max, l[k]);
            before += c[k];
            if (here) while (e <= n_bins && rank[e] <= before) ed[e++] = code;   // the ranks in (before - c, before]
        }
        if (here) while (next_edge <= n_bins && rank[next_edge] <= carry) ++next_edge;
#pragma unroll
        for (int k = 0; k < CS_ITEMS; ++k) { c[k] = c_next[k]; l[k] = l_next[k]; }
    }
    // block reduction of the five per-lane results
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        distinct += __shfl_xor(distinct, s); len_sum += __shfl_xor(len_sum, s);
        mn = min(mn, __shfl_xor(mn, s)); mx = max(mx, __shfl_xor(mx, s)); len_max = max(len_max, __shfl_xor(len_max, s));
    }
    if (lane == 0) { red_sum[0][wave] = distinct; red_sum[1][wave] = len_sum; red_i[0][wave] = mn; red_i[1][wave] = mx; red_i[2][wave] = len_max; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            distinct += red_sum[0][w]; len_sum += red_sum[1][w];
            mn = min(mn, red_i[0][w]); mx = max(mx, red_i[1][w]); len_max = max(len_max, red_i[2][w]);
        }
        st[1] = distinct; st[2] = mx < 0 ? -1 : mn; st[3] = mx; st[4] = len_sum; st[5] = len_max;
        if (ed && mx >= 0) ed[0] = mn;
    }
}

}  // namespace

extern "C" {

// scratch slots held together: TABLE_A (column descriptors) TABLE_B (the six numbers per column) COLS (edges) IN_COLS (length LUTs) VALS (counts)
RGBM_EXPORT int rgbm_table_column_stats(const rgbm_table* t, const int32_t* cols, int32_t n_cols, const int32_t* const* len_lut, int32_t n_bins,
                                        int64_t* stats_out, int32_t* edges_out) {
    if (!t || !cols || !stats_out || n_cols < 1) return fail(RGBM_ERR_ARG, "rgbm_table_column_stats: bad argument (at least one column)");
    if (n_bins < 0 || n_bins > CS_MAX_BINS) return fail(RGBM_ERR_PARAM, "rgbm_table_column_stats: n_bins must be 0 or 1..254");
    if (n_bins > 0 && !edges_out) return fail(RGBM_ERR_ARG, "rgbm_table_column_stats: edges_out is NULL with n_bins > 0");
    if (n_cols > 65535) return fail(RGBM_ERR_PARAM, "rgbm_table_column_stats: more than 65535 listed columns");
    if (const int rc = refuse_cols(*t, cols, n_cols, false, nullptr, "rgbm_table_column_stats")) return rc;
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        std::vector<CsDesc> desc((size_t)n_cols);
        long long n_cnt = 0, n_lut = 0;
        for (int j = 0; j < n_cols; ++j) {
            const int nc = t->n_codes[cols[j]];
            const bool has_lut = len_lut && len_lut[j];
            desc[j] = CsDesc{n_cnt, has_lut ? n_lut : -1, cols[j], nc};
            n_cnt += nc; if (has_lut) n_lut += nc;
        }
        const CsDesc* d_desc = scr_upload<CsDesc>(*t, SCR_TABLE_A, desc.data(), desc.size(), s);
        int32_t* d_luts = scr<int32_t>(*t, SCR_IN_COLS, (size_t)n_lut);           // every LUT goes from the caller's array to its place
        for (int j = 0; j < n_cols; ++j)
            if (desc[j].lut_off >= 0) HIPCHK(hipMemcpyAsync(d_luts + desc[j].lut_off, len_lut[j], (size_t)desc[j].n_codes * 4, hipMemcpyHostToDevice, s));
        unsigned long long* d_cnt = scr<unsigned long long>(*t, SCR_VALS, (size_t)n_cnt);
        long long* d_stats = scr<long long>(*t, SCR_TABLE_B, (size_t)n_cols * CS_STATS);
        int32_t* d_edges = n_bins > 0 ? scr<int32_t>(*t, SCR_COLS, (size_t)n_cols * (n_bins + 1)) : nullptr;
        HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)n_cnt * 8, s));
        HIPCHK(hipMemsetAsync(d_stats, 0, (size_t)n_cols * CS_STATS * 8, s));
        const unsigned nb = std::max(std::min<unsigned>(nblocks(t->n, 256 * CS_UNROLL * 4), 256u * 8u), 1u);
        hipLaunchKernelGGL(k_colstat_count, dim3(nb, (unsigned)n_cols), dim3(256), 0, s, t->codes.p, (long long)t->n, d_desc, d_cnt,
                           reinterpret_cast<unsigned long long*>(d_stats));
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_colstat_reduce, dim3((unsigned)n_cols), dim3(256), 0, s, d_desc, d_cnt, d_luts, (long long)t->n, (int)n_bins, d_stats, d_edges);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(stats_out, d_stats, (size_t)n_cols * CS_STATS * 8, hipMemcpyDeviceToHost, s));
        if (d_edges) HIPCHK(hipMemcpyAsync(edges_out, d_edges, (size_t)n_cols * (n_bins + 1) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

}  // extern "C"
