// rgbm_kmeans.hip -- a relational step on the HBM-resident code table (what the steps share is rgbm_prep.h):
//   kmeans_assign / read  one Lloyd step of the q-gram k-means of RepairMisc.splitInputTable, in code space (RepairMiscApi.scala:52-153)
// =============================================================================================
// q-gram k-means in code space (RepairMisc.splitInputTable; the statement is repair/qgram_kmeans.py): one Lloyd assignment
// step over the resident codes.  The host hands P = -2 E C^T ([d_tot][k] float64, one row per dictionary entry of the listed columns) and
// h_k = |C_k|^2; the score of a row for cluster kk is  ((h[kk] + P[off_0 + code_0][kk]) + P[off_1 + code_1][kk]) + ...  in `cols` order,
// float64, additions only (a NULL code adds nothing); the label is the lowest kk with the least score.
//   k_kmeans_assign   one row per lane, consecutive lanes on consecutive rows (every column load coalesced), KM_UNROLL rows a lane in flight.
//                     The clusters are scored in register chunks of KM_KC: a chunk walks the columns once, so a table of k <= KM_KC clusters
//                     reads its codes once for the scores (ceil(k / KM_KC) times otherwise, the re-reads from the caches: a workgroup's
//                     tile is 16 KiB per column) and once more for the counts.  The order of the additions of one cluster never changes.
//                     One workgroup of 1024 threads per CU owns the CU's 160 KiB of LDS: 96 KiB for P and h, 56 KiB for
//                     the counters, 8 KiB left.  P and h live in LDS up to KM_LDS_P_DOUBLES doubles, a code's row padded to an ODD number of doubles so that rows of
//                     different codes start in different 8-byte bank slots; above the bound they are read where they lie (global memory).
//                     counts[kk][code]: 32-bit LDS counters up to KM_LDS_COUNTERS of them, the non-zero ones flushed with 64-bit global
//                     atomics; above that 64-bit global atomics per (row, column).  A workgroup sees at most KM_ROWS_PER_WG_MAX rows of at
//                     most KM_MAX_COLS columns: 2^30 increments, a 32-bit counter cannot wrap.  sizes / n_changed: the lanes of a wave
//                     that hold the same label add once (ballot + popcount) into LDS, one global atomic per workgroup and cluster.
//                     Every sum is an integer sum: the result does not depend on the launch geometry.
// Algorithmic bytes per row: 4 B per column (scores) + 4 B per column (counts) + 4 B previous label + 4 B new label.
// =============================================================================================
#include "rgbm_prep.h"

namespace {

using namespace rgh;

constexpr int KM_B = 1024;                                  // threads per workgroup: the 16 waves a CU holds at this kernel's registers
constexpr int KM_UNROLL = 4;                                // rows a lane keeps in flight
constexpr int KM_KC = 8;                                    // clusters scored per register chunk
constexpr int KM_LDS_P_DOUBLES = 12288;                     // P and h in LDS: (d_tot + 1) * (k | 1) doubles at most (96 KiB)
constexpr int KM_LDS_COUNTERS = 14336;                      // counts in LDS: k * d_tot 32-bit counters at most (56 KiB)
constexpr long long KM_ROWS_PER_WG_MAX = 1ll << 20;
constexpr int KM_MAX_COLS = 1024, KM_MAX_K = 64;
constexpr long long KM_MAX_CELLS = 1ll << 27;               // d_tot * k

struct KmCol { long long off; int32_t col, n_codes; };

// p: [d_tot + 1][k], row d_tot = h.  out: sizes [k], then n_changed.
template <bool P_LDS, bool C_LDS>
__global__ __launch_bounds__(KM_B) void k_kmeans_assign(const int32_t* __restrict__ codes, long long n, const KmCol* __restrict__ cd, int ncols, int k,
                                                        const double* __restrict__ p, long long d_tot, int first, long long rows_per_wg,
                                                        int32_t* __restrict__ assign, unsigned long long* __restrict__ counts,
                                                        unsigned long long* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char km_smem[];
    const int tid = threadIdx.x;
    const int st = P_LDS ? (k | 1) : k;                                          // doubles from one code's row to the next
    const unsigned n_lp = P_LDS ? (unsigned)(d_tot + 1) * (unsigned)st : 0u;
    const unsigned n_lc = C_LDS ? (unsigned)k * (unsigned)d_tot : 0u;
    double* lp = reinterpret_cast<double*>(km_smem);
    unsigned* lc = reinterpret_cast<unsigned*>(km_smem + (size_t)n_lp * 8);
    unsigned* lsz = lc + n_lc;                                                  // [k] sizes, [k] = rows that changed their label
    if (P_LDS) {
        const unsigned tot = (unsigned)(d_tot + 1) * (unsigned)k;
        for (unsigned i = tid; i < tot; i += KM_B) lp[(i / (unsigned)k) * (unsigned)st + i % (unsigned)k] = p[i];
    }
    for (unsigned i = tid; i < n_lc + (unsigned)k + 1u; i += KM_B) lc[i] = 0;    // (lsz follows lc)
    __syncthreads();
    const double* P = P_LDS ? lp : p;
    const double* hrow = P + d_tot * st;
    const long long begin = (long long)blockIdx.x * rows_per_wg;
    const long long end = begin + rows_per_wg < n ? begin + rows_per_wg : n;
    for (long long base = begin; base < end; base += (long long)KM_B * KM_UNROLL) {
        bool in[KM_UNROLL]; int best[KM_UNROLL]; double bs[KM_UNROLL];
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) { in[u] = base + (long long)u * KM_B + tid < end; best[u] = 0; bs[u] = 0.0; }
        for (int kc = 0; kc < k; kc += KM_KC) {
            const int kn = k - kc < KM_KC ? k - kc : KM_KC;
            double s[KM_UNROLL][KM_KC];
#pragma unroll
            for (int c = 0; c < KM_KC; ++c) {
                const double hv = c < kn ? hrow[kc + c] : 0.0;
#pragma unroll
                for (int u = 0; u < KM_UNROLL; ++u) s[u][c] = hv;
            }
            for (int j = 0; j < ncols; ++j) {
                const KmCol d = cd[j];
                const int32_t* col = codes + (long long)d.col * n + base + tid;
                int v[KM_UNROLL];
#pragma unroll
                for (int u = 0; u < KM_UNROLL; ++u) v[u] = in[u] ? col[(long long)u * KM_B] : -1;      // KM_UNROLL coalesced loads in flight
#pragma unroll
                for (int u = 0; u < KM_UNROLL; ++u) {
                    if (v[u] < 0 || v[u] >= d.n_codes) continue;                                        // NULL adds nothing
                    const double* q = P + (d.off + v[u]) * st + kc;
#pragma unroll
                    for (int c = 0; c < KM_KC; ++c) if (c < kn) s[u][c] = s[u][c] + q[c];
                }
            }
#pragma unroll
            for (int u = 0; u < KM_UNROLL; ++u) {
#pragma unroll
                for (int c = 0; c < KM_KC; ++c)
                    if (c < kn && ((kc == 0 && c == 0) || s[u][c] < bs[u])) { bs[u] = s[u][c]; best[u] = kc + c; }   // ascending, strict: the lowest id wins
            }
        }
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) {
            const long long r = base + (long long)u * KM_B + tid;
            bool moved = false;
            if (in[u]) {
                moved = first || assign[r] != best[u];
                assign[r] = best[u];
            }
            const unsigned long long mv = __ballot(moved);
            if (lane_id() == 0 && mv) atomicAdd(&lsz[k], (unsigned)__popcll(mv));
            unsigned long long pend = __ballot(in[u]);
            while (pend) {                                                       // one LDS atomic per label the wave holds
                const int leader = __ffsll((long long)pend) - 1;
                const int lab = __shfl(best[u], leader);
                const unsigned long long same = __ballot(in[u] && best[u] == lab);
                if (lane_id() == leader) atomicAdd(&lsz[lab], (unsigned)__popcll(same));
                pend &= ~same;
            }
        }
        for (int j = 0; j < ncols; ++j) {
            const KmCol d = cd[j];
            const int32_t* col = codes + (long long)d.col * n + base + tid;
            int v[KM_UNROLL];
#pragma unroll
            for (int u = 0; u < KM_UNROLL; ++u) v[u] = in[u] ? col[(long long)u * KM_B] : -1;
#pragma unroll
            for (int u = 0; u < KM_UNROLL; ++u) {
                if (v[u] < 0 || v[u] >= d.n_codes) continue;
                const long long cell = (long long)best[u] * d_tot + d.off + v[u];
                if (C_LDS) atomicAdd(&lc[cell], 1u);
                else atomicAdd(&counts[cell], 1ull);
            }
        }
    }
    __syncthreads();
    if (C_LDS)
        for (unsigned i = tid; i < n_lc; i += KM_B) { const unsigned v = lc[i]; if (v) atomicAdd(&counts[i], (unsigned long long)v); }
    for (int i = tid; i <= k; i += KM_B) { const unsigned v = lsz[i]; if (v) atomicAdd(&out[i], (unsigned long long)v); }
}

template <bool P_LDS, bool C_LDS>
void kmeans_launch(unsigned grid, size_t lds, hipStream_t s, const int32_t* codes, long long n, const KmCol* cd, int ncols, int k, const double* p,
                   long long d_tot, int first, long long rows_per_wg, int32_t* assign, unsigned long long* counts, unsigned long long* out) {
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_kmeans_assign<P_LDS, C_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_kmeans_assign<P_LDS, C_LDS>), dim3(grid), dim3(KM_B), lds, s, codes, n, cd, ncols, k, p, d_tot, first, rows_per_wg, assign,
                       counts, out);
}

}  // namespace

extern "C" {

// scratch slots held together: TABLE_A (P, h) TABLE_B (column descriptors) VALS (counts, sizes, n_changed)
RGBM_EXPORT int rgbm_table_kmeans_assign(rgbm_table* t, const int32_t* cols, int32_t n_cols, const int64_t* code_off, int32_t k, const double* p,
                                         int64_t d_tot, const double* h, int32_t first, int64_t* counts_out, int64_t* sizes_out,
                                         int64_t* n_changed_out) {
    if (!t || !p || !h || !counts_out || !sizes_out || !n_changed_out) return fail(RGBM_ERR_ARG, "rgbm_table_kmeans_assign: bad argument");
    return guarded([&]() {
        use_device(t->device);
        if (k < 2 || k > KM_MAX_K) throw std::invalid_argument("rgbm_table_kmeans_assign: k must be 2 .. 64");
        if (n_cols < 1 || n_cols > KM_MAX_COLS || !cols || !code_off) throw std::invalid_argument("rgbm_table_kmeans_assign: 1 .. 1024 columns expected");
        check_cols(*t, cols, n_cols, "rgbm_table_kmeans_assign");
        if (d_tot < 1 || d_tot > KM_MAX_CELLS / k) throw std::invalid_argument("rgbm_table_kmeans_assign: d_tot * k must be 1 .. 2^27");
        std::vector<KmCol> cd((size_t)n_cols);
        for (int j = 0; j < n_cols; ++j) {
            const int32_t nc = std::max<int32_t>(t->n_codes[cols[j]], 0);
            if (code_off[j] < 0 || code_off[j] > d_tot - nc) throw std::invalid_argument("rgbm_table_kmeans_assign: a column's codes do not fit into d_tot");
            cd[j] = KmCol{(long long)code_off[j], cols[j], nc};
        }
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!first && !t->km_valid) throw std::invalid_argument("rgbm_table_kmeans_assign: first == 0 without a previous assignment of this table");
        const long long n = t->n;
        const size_t cells = (size_t)k * (size_t)d_tot;
        if (t->km_assign.n < (size_t)std::max<long long>(n, 1)) t->km_assign.alloc((size_t)std::max<long long>(n, 1));      // (only when there is no previous one)
        const KmCol* d_cd = scr_upload<KmCol>(*t, SCR_TABLE_B, cd.data(), cd.size(), s);
        double* d_p = scr<double>(*t, SCR_TABLE_A, cells + (size_t)k);
        HIPCHK(hipMemcpyAsync(d_p, p, cells * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_p + cells, h, (size_t)k * 8, hipMemcpyHostToDevice, s));
        unsigned long long* d_out = scr<unsigned long long>(*t, SCR_VALS, cells + (size_t)k + 1);     // counts, sizes, n_changed
        HIPCHK(hipMemsetAsync(d_out, 0, (cells + (size_t)k + 1) * 8, s));
        if (n > 0) {
            const bool p_lds = (d_tot + 1) * (long long)(k | 1) <= KM_LDS_P_DOUBLES, c_lds = (long long)cells <= KM_LDS_COUNTERS;
            const size_t lds = (p_lds ? (size_t)(d_tot + 1) * (size_t)(k | 1) * 8 : 0) + ((c_lds ? cells : 0) + (size_t)k + 1) * 4;
            // two rounds of workgroups (one per CU) over the device at most, each on a whole number of load tiles and no more than KM_ROWS_PER_WG_MAX rows
            const long long tile = (long long)KM_B * KM_UNROLL;
            long long chunks = std::min<long long>((n + tile - 1) / tile, 512);
            chunks = std::max<long long>(chunks, (n + KM_ROWS_PER_WG_MAX - 1) / KM_ROWS_PER_WG_MAX);
            const long long rows_per_wg = ((n + chunks - 1) / chunks + tile - 1) / tile * tile;
            const unsigned grid = (unsigned)((n + rows_per_wg - 1) / rows_per_wg);
            // (P in LDS implies the counters in LDS: k * d_tot < (d_tot + 1) * (k | 1) <= KM_LDS_P_DOUBLES < KM_LDS_COUNTERS)
            static_assert(KM_LDS_P_DOUBLES <= KM_LDS_COUNTERS, "a table whose P fits the LDS keeps its counters there too");
            auto go = p_lds ? kmeans_launch<true, true> : (c_lds ? kmeans_launch<false, true> : kmeans_launch<false, false>);
            go(grid, lds, s, t->codes.p, n, d_cd, (int)n_cols, (int)k, d_p, (long long)d_tot, first ? 1 : 0, rows_per_wg, t->km_assign.p, d_out, d_out + cells);
            HIPCHK(hipGetLastError());
        }
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are 64-bit");
        HIPCHK(hipMemcpyAsync(counts_out, d_out, cells * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(sizes_out, d_out + cells, (size_t)k * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(n_changed_out, d_out + cells + k, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        t->km_valid = true;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_kmeans_read(const rgbm_table* t, int32_t* assign_out) {
    if (!t || !assign_out) return fail(RGBM_ERR_ARG, "rgbm_table_kmeans_read: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!t->km_valid) throw std::invalid_argument("rgbm_table_kmeans_read: no rgbm_table_kmeans_assign result on this table");
        HIPCHK(hipMemcpyAsync(assign_out, t->km_assign.p, (size_t)t->n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

}  // extern "C"
