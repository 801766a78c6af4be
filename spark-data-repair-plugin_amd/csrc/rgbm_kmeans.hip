// rgbm_kmeans.hip -- a relational step on the HBM-resident code table (what the steps share is rgbm_prep.h):
//   kmeans_assign / read  one Lloyd step of the q-gram k-means of RepairMisc.splitInputTable, in code space (RepairMiscApi.scala:52-153)
//   kmeans_bisect         one pass of a level of the bisecting k-means (clustering_alg = "bisecting"; repair/qgram_bisect.py)
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
//   k_kmeans_bisect   the same shape for one pass of a bisecting level: the label of a row names a tree node, slot_of[label] the slot s of the
//                     node being split (or -1: the row is left alone, its codes are not even loaded), and the row is scored against the two
//                     children of ITS slot only:  s0 = h[2s] + P[..][2s] + ..., s1 the same at 2s + 1, right child iff s1 < s0.  Two doubles of
//                     P per attribute at any m.  LDS: 96 KiB of counters first (KB_LDS_COUNTERS: an LDS atomic in place of a
//                     64-bit global one per row and column), 44 KiB for P and h (KB_LDS_P_DOUBLES, odd row stride as above), and slot_of /
//                     child / sizes behind them (at most 16 KiB + 4 B).  Staging, the counting walk and the flush are k_kmeans_assign's.
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
constexpr int KB_LDS_P_DOUBLES = 5632;                      // bisect: P and h in LDS: (d_tot + 1) * (2m | 1) doubles at most (44 KiB)
constexpr int KB_LDS_COUNTERS = 24576;                      // bisect: counts in LDS: 2m * d_tot 32-bit counters at most (96 KiB)
constexpr int KB_MAX_M = 512;                               // slots of one pass
constexpr int KB_MAX_NODES = 2048;                          // tree nodes a label may name
constexpr int KB_MAX_SWEEPS = 32;                           // windows of slots one pass is swept in at most, the counters of a window in LDS
constexpr int KB_BALLOT_M = 4;                              // up to this many slots the sizes are added once per wave and child (ballot)

struct KmCol { long long off; int32_t col, n_codes; };

// ---- what the two kernels share ----
// p [rows][k] -> lp with `st` doubles from one row to the next
__device__ __forceinline__ void km_stage_p(double* lp, const double* __restrict__ p, unsigned rows, unsigned k, unsigned st, int tid) {
    const unsigned tot = rows * k;
    for (unsigned i = tid; i < tot; i += KM_B) lp[(i / k) * st + i % k] = p[i];
}

// the counting walk over one load tile: counts[best[u]][off_j + code] += 1 for every row u the lane holds (in[u]) and every column
template <bool C_LDS>
__device__ __forceinline__ void km_count_tile(const int32_t* __restrict__ codes, long long n, const KmCol* __restrict__ cd, int ncols, long long at,
                                              const bool (&in)[KM_UNROLL], const int (&best)[KM_UNROLL], long long d_tot, unsigned* lc,
                                              unsigned long long* __restrict__ counts) {
    for (int j = 0; j < ncols; ++j) {
        const KmCol d = cd[j];
        const int32_t* col = codes + (long long)d.col * n + at;
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

// one LDS atomic per label the wave holds among its lanes with `in`
__device__ __forceinline__ void km_add_sizes(bool in, int lab, unsigned* lsz) {
    unsigned long long pend = __ballot(in);
    while (pend) {
        const int leader = __ffsll((long long)pend) - 1;
        const int l = __shfl(lab, leader);
        const unsigned long long same = __ballot(in && lab == l);
        if (lane_id() == leader) atomicAdd(&lsz[l], (unsigned)__popcll(same));
        pend &= ~same;
    }
}

// the workgroup's LDS counters (the non-zero ones) and its n_sz sizes / n_changed words into global memory
__device__ __forceinline__ void km_flush(const unsigned* lc, unsigned n_lc, unsigned long long* __restrict__ counts, const unsigned* lsz, int n_sz,
                                         unsigned long long* __restrict__ out, int tid) {
    for (unsigned i = tid; i < n_lc; i += KM_B) { const unsigned v = lc[i]; if (v) atomicAdd(&counts[i], (unsigned long long)v); }
    for (int i = tid; i < n_sz; i += KM_B) { const unsigned v = lsz[i]; if (v) atomicAdd(&out[i], (unsigned long long)v); }
}

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
    if (P_LDS) km_stage_p(lp, p, (unsigned)(d_tot + 1), (unsigned)k, (unsigned)st, tid);
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
            km_add_sizes(in[u], best[u], lsz);
        }
        km_count_tile<C_LDS>(codes, n, cd, ncols, base + tid, in, best, d_tot, lc, counts);
    }
    __syncthreads();
    km_flush(lc, n_lc, counts, lsz, k + 1, out, tid);
}

template <bool P_LDS, bool C_LDS>
void kmeans_launch(unsigned grid, size_t lds, hipStream_t s, const int32_t* codes, long long n, const KmCol* cd, int ncols, int k, const double* p,
                   long long d_tot, int first, long long rows_per_wg, int32_t* assign, unsigned long long* counts, unsigned long long* out) {
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_kmeans_assign<P_LDS, C_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_kmeans_assign<P_LDS, C_LDS>), dim3(grid), dim3(KM_B), lds, s, codes, n, cd, ncols, k, p, d_tot, first, rows_per_wg, assign,
                       counts, out);
}

// One pass of a bisecting level.  p: [d_tot + 1][2m], row d_tot = h.  tabs: slot_of [n_nodes], then child [2m].  out: sizes [2m], then n_changed.
// A row is scored when its label lies in [0, n_nodes) and names a slot of the window [s_lo, s_lo + s_n); every other row keeps its label (first:
// becomes node 0) and is counted nowhere.  The LDS counters are the window's: 2 s_n * d_tot of them (the host sweeps the windows, see the entry).
// WIN false: the window is every slot, and the kernel is compiled without the window's arithmetic (with it a pass at m = 1 took 0.40 ms
// in place of 0.30 on the bench table: profiles/kmeans_bisect_bench.json).
template <bool P_LDS, bool C_LDS, bool WIN>
__global__ __launch_bounds__(KM_B) void k_kmeans_bisect(const int32_t* __restrict__ codes, long long n, const KmCol* __restrict__ cd, int ncols, int m,
                                                        const double* __restrict__ p, long long d_tot, const int32_t* __restrict__ tabs, int n_nodes,
                                                        int s_lo, int s_n, int first, long long rows_per_wg, int32_t* __restrict__ assign,
                                                        unsigned long long* __restrict__ counts, unsigned long long* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char km_smem[];
    const int tid = threadIdx.x;
    const int k = 2 * m;
    const int st = P_LDS ? (k | 1) : k;
    const unsigned n_lp = P_LDS ? (unsigned)(d_tot + 1) * (unsigned)st : 0u;
    const unsigned n_lc = C_LDS ? (WIN ? 2u * (unsigned)s_n : (unsigned)k) * (unsigned)d_tot : 0u;
    double* lp = reinterpret_cast<double*>(km_smem);
    unsigned* lc = reinterpret_cast<unsigned*>(km_smem + (size_t)n_lp * 8);
    unsigned* lsz = lc + n_lc;                                                  // [2m] sizes, [2m] = rows that changed their label
    int* lslot = reinterpret_cast<int*>(lsz + k + 1);                           // [n_nodes]
    int* lchild = lslot + n_nodes;                                              // [2m]
    if (P_LDS) km_stage_p(lp, p, (unsigned)(d_tot + 1), (unsigned)k, (unsigned)st, tid);
    for (unsigned i = tid; i < n_lc + (unsigned)k + 1u; i += KM_B) lc[i] = 0;    // (lsz follows lc)
    for (int i = tid; i < n_nodes + k; i += KM_B) lslot[i] = tabs[i];            // (lchild follows lslot)
    __syncthreads();
    const double* P = P_LDS ? lp : p;
    const double* hrow = P + d_tot * st;
    const long long begin = (long long)blockIdx.x * rows_per_wg;
    const long long end = begin + rows_per_wg < n ? begin + rows_per_wg : n;
    for (long long base = begin; base < end; base += (long long)KM_B * KM_UNROLL) {
        bool in[KM_UNROLL], act[KM_UNROLL]; int lab[KM_UNROLL], s2[KM_UNROLL]; double s0[KM_UNROLL], s1[KM_UNROLL];
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) {
            const long long r = base + (long long)u * KM_B + tid;
            in[u] = r < end;
            lab[u] = in[u] ? (first ? 0 : assign[r]) : -1;
        }
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) {
            const int sl = (unsigned)lab[u] < (unsigned)n_nodes ? lslot[lab[u]] : -1;
            act[u] = WIN ? (unsigned)(sl - s_lo) < (unsigned)s_n : sl >= 0;       // (sl = -1 is outside every window)
            s2[u] = act[u] ? 2 * sl : 0;                                         // the left child's column of P, counters and sizes
            s0[u] = hrow[s2[u]]; s1[u] = hrow[s2[u] + 1];
        }
        for (int j = 0; j < ncols; ++j) {
            const KmCol d = cd[j];
            const int32_t* col = codes + (long long)d.col * n + base + tid;
            int v[KM_UNROLL];
#pragma unroll
            for (int u = 0; u < KM_UNROLL; ++u) v[u] = act[u] ? col[(long long)u * KM_B] : -1;     // a row outside the slots loads nothing
#pragma unroll
            for (int u = 0; u < KM_UNROLL; ++u) {
                if (v[u] < 0 || v[u] >= d.n_codes) continue;                                        // NULL adds nothing
                const double* q = P + (d.off + v[u]) * st + s2[u];
                s0[u] = s0[u] + q[0];
                s1[u] = s1[u] + q[1];
            }
        }
        int best[KM_UNROLL];
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) {
            const long long r = base + (long long)u * KM_B + tid;
            best[u] = s2[u] + (s1[u] < s0[u] ? 1 : 0);                           // strict: a tie goes left
            const int now = act[u] ? lchild[best[u]] : lab[u];
            const bool moved = act[u] && now != lab[u];
            if (in[u] && (first || moved)) assign[r] = now;                      // (first: a row outside the slots is node 0)
            const unsigned long long mv = __ballot(moved);
            if (lane_id() == 0 && mv) atomicAdd(&lsz[k], (unsigned)__popcll(mv));
            if (m <= KB_BALLOT_M) km_add_sizes(act[u], best[u], lsz);
            else if (act[u]) atomicAdd(&lsz[best[u]], 1u);
        }
        if (WIN) {
#pragma unroll
            for (int u = 0; u < KM_UNROLL; ++u) best[u] -= 2 * s_lo;              // the window's counters start at its first child
        }
        km_count_tile<C_LDS>(codes, n, cd, ncols, base + tid, act, best, d_tot, lc, counts);
    }
    __syncthreads();
    km_flush(lc, n_lc, counts + (WIN ? 2ll * s_lo * d_tot : 0ll), lsz, k + 1, out, tid);
}

template <bool P_LDS, bool C_LDS, bool WIN>
void bisect_launch(unsigned grid, size_t lds, hipStream_t s, const int32_t* codes, long long n, const KmCol* cd, int ncols, int m, const double* p,
                   long long d_tot, const int32_t* tabs, int n_nodes, int s_lo, int s_n, int first, long long rows_per_wg, int32_t* assign,
                   unsigned long long* counts, unsigned long long* out) {
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_kmeans_bisect<P_LDS, C_LDS, WIN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_kmeans_bisect<P_LDS, C_LDS, WIN>), dim3(grid), dim3(KM_B), lds, s, codes, n, cd, ncols, m, p, d_tot, tabs, n_nodes, s_lo, s_n, first,
                       rows_per_wg, assign, counts, out);
}

// the refusals the two entries share; returns the column descriptors
std::vector<KmCol> km_columns(const rgbm_table& t, const int32_t* cols, int32_t n_cols, const int64_t* code_off, int64_t d_tot, int64_t k, const char* entry) {
    const std::string e(entry);
    if (n_cols < 1 || n_cols > KM_MAX_COLS || !cols || !code_off) throw std::invalid_argument(e + ": 1 .. 1024 columns expected");
    check_cols(t, cols, n_cols, entry);
    if (d_tot < 1 || d_tot > KM_MAX_CELLS / k) throw std::invalid_argument(e + ": d_tot * k must be 1 .. 2^27");
    std::vector<KmCol> cd((size_t)n_cols);
    for (int j = 0; j < n_cols; ++j) {
        const int32_t nc = std::max<int32_t>(t.n_codes[cols[j]], 0);
        if (code_off[j] < 0 || code_off[j] > d_tot - nc) throw std::invalid_argument(e + ": a column's codes do not fit into d_tot");
        cd[j] = KmCol{(long long)code_off[j], cols[j], nc};
    }
    return cd;
}

// two rounds of workgroups (one per CU) over the device at most, each on a whole number of load tiles and no more than KM_ROWS_PER_WG_MAX rows
void km_grid(long long n, long long* rows_per_wg, unsigned* grid) {
    const long long tile = (long long)KM_B * KM_UNROLL;
    long long chunks = std::min<long long>((n + tile - 1) / tile, 512);
    chunks = std::max<long long>(chunks, (n + KM_ROWS_PER_WG_MAX - 1) / KM_ROWS_PER_WG_MAX);
    *rows_per_wg = ((n + chunks - 1) / chunks + tile - 1) / tile * tile;
    *grid = (unsigned)((n + *rows_per_wg - 1) / *rows_per_wg);
}

// The device side of a step of either entry (prep_mu held, every refusal behind): P, h and the column descriptors up, the k * d_tot + k + 1
// result words zeroed, launch(d_cd, d_p, d_counts, d_sizes, rows_per_wg, grid) when there are rows, counts / sizes / n_changed down.
// scratch slots held together: TABLE_A (P, h) TABLE_B (column descriptors) VALS (counts, sizes, n_changed); COLS is the launch's own
template <typename Launch>
void km_step(rgbm_table& t, hipStream_t s, const std::vector<KmCol>& cd, int k, const double* p, const double* h, int64_t d_tot, int64_t* counts_out,
             int64_t* sizes_out, int64_t* n_changed_out, Launch&& launch) {
    const long long n = t.n;
    const size_t cells = (size_t)k * (size_t)d_tot;
    if (t.km_assign.n < (size_t)std::max<long long>(n, 1)) t.km_assign.alloc((size_t)std::max<long long>(n, 1));      // (only when there is no previous one)
    const KmCol* d_cd = scr_upload<KmCol>(t, SCR_TABLE_B, cd.data(), cd.size(), s);
    double* d_p = scr<double>(t, SCR_TABLE_A, cells + (size_t)k);
    HIPCHK(hipMemcpyAsync(d_p, p, cells * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_p + cells, h, (size_t)k * 8, hipMemcpyHostToDevice, s));
    unsigned long long* d_out = scr<unsigned long long>(t, SCR_VALS, cells + (size_t)k + 1);     // counts, sizes, n_changed
    HIPCHK(hipMemsetAsync(d_out, 0, (cells + (size_t)k + 1) * 8, s));
    if (n > 0) {
        long long rows_per_wg; unsigned grid;
        km_grid(n, &rows_per_wg, &grid);
        launch(d_cd, d_p, d_out, d_out + cells, rows_per_wg, grid);
        HIPCHK(hipGetLastError());
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are 64-bit");
    HIPCHK(hipMemcpyAsync(counts_out, d_out, cells * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sizes_out, d_out + cells, (size_t)k * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_changed_out, d_out + cells + k, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    t.km_valid = true;
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
        const std::vector<KmCol> cd = km_columns(*t, cols, n_cols, code_off, d_tot, k, "rgbm_table_kmeans_assign");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!first && !t->km_valid) throw std::invalid_argument("rgbm_table_kmeans_assign: first == 0 without a previous assignment of this table");
        const size_t cells = (size_t)k * (size_t)d_tot;
        km_step(*t, s, cd, (int)k, p, h, d_tot, counts_out, sizes_out, n_changed_out,
                [&](const KmCol* d_cd, const double* d_p, unsigned long long* d_counts, unsigned long long* d_out, long long rows_per_wg, unsigned grid) {
            const bool p_lds = (d_tot + 1) * (long long)(k | 1) <= KM_LDS_P_DOUBLES, c_lds = (long long)cells <= KM_LDS_COUNTERS;
            const size_t lds = (p_lds ? (size_t)(d_tot + 1) * (size_t)(k | 1) * 8 : 0) + ((c_lds ? cells : 0) + (size_t)k + 1) * 4;
            // (P in LDS implies the counters in LDS: k * d_tot < (d_tot + 1) * (k | 1) <= KM_LDS_P_DOUBLES < KM_LDS_COUNTERS)
            static_assert(KM_LDS_P_DOUBLES <= KM_LDS_COUNTERS, "a table whose P fits the LDS keeps its counters there too");
            auto go = p_lds ? kmeans_launch<true, true> : (c_lds ? kmeans_launch<false, true> : kmeans_launch<false, false>);
            go(grid, lds, s, t->codes.p, t->n, d_cd, (int)n_cols, (int)k, d_p, (long long)d_tot, first ? 1 : 0, rows_per_wg, t->km_assign.p, d_counts, d_out);
        });
        return RGBM_OK;
    });
}

// scratch slots held together: those of km_step, and COLS (slot_of, child)
RGBM_EXPORT int rgbm_table_kmeans_bisect(rgbm_table* t, const int32_t* cols, int32_t n_cols, const int64_t* code_off, int64_t d_tot, const int32_t* slot_of,
                                         int32_t n_nodes, int32_t m, const int32_t* child, const double* p, const double* h, int32_t first,
                                         int64_t* counts_out, int64_t* sizes_out, int64_t* n_changed_out) {
    if (!t || !p || !h || !counts_out || !sizes_out || !n_changed_out) return fail(RGBM_ERR_ARG, "rgbm_table_kmeans_bisect: bad argument");
    return guarded([&]() {
        use_device(t->device);
        if (m < 1 || m > KB_MAX_M) throw std::invalid_argument("rgbm_table_kmeans_bisect: m must be 1 .. 512");
        if (n_nodes < 1 || n_nodes > KB_MAX_NODES || !slot_of || !child) throw std::invalid_argument("rgbm_table_kmeans_bisect: 1 .. 2048 nodes expected");
        const int k = 2 * m;
        const std::vector<KmCol> cd = km_columns(*t, cols, n_cols, code_off, d_tot, k, "rgbm_table_kmeans_bisect");
        std::vector<int32_t> tabs((size_t)n_nodes + (size_t)k);
        for (int i = 0; i < n_nodes; ++i) {
            if (slot_of[i] < -1 || slot_of[i] >= m) throw std::invalid_argument("rgbm_table_kmeans_bisect: a slot_of entry outside -1 .. m - 1");
            tabs[(size_t)i] = slot_of[i];
        }
        for (int i = 0; i < k; ++i) {
            if (child[i] < 0 || child[i] >= n_nodes) throw std::invalid_argument("rgbm_table_kmeans_bisect: a child label outside 0 .. n_nodes - 1");
            tabs[(size_t)n_nodes + (size_t)i] = child[i];
        }
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!first && !t->km_valid) throw std::invalid_argument("rgbm_table_kmeans_bisect: first == 0 without labels on this table");
        km_step(*t, s, cd, k, p, h, d_tot, counts_out, sizes_out, n_changed_out,
                [&](const KmCol* d_cd, const double* d_p, unsigned long long* d_counts, unsigned long long* d_out, long long rows_per_wg, unsigned grid) {
            const int32_t* d_tabs = scr_upload<int32_t>(*t, SCR_COLS, tabs.data(), tabs.size(), s);
            const bool p_lds = (d_tot + 1) * (long long)(k | 1) <= KB_LDS_P_DOUBLES;
            // The counters of `win` slots fit the LDS.  Fewer than m: the pass is swept window by window, a sweep scoring the rows of its own slots
            // (a row never leaves its window: its children name its slot, which is checked here; a caller's table that does not say so, more than
            // KB_MAX_SWEEPS windows, or first != 0 with no labels to re-read take the one launch with global counters).  sizes and n_changed add up
            // in global memory over the sweeps.
            int win = (int)std::min<long long>(m, KB_LDS_COUNTERS / (2 * (long long)d_tot));
            bool closed = true;
            for (int i = 0; i < k && closed; ++i) closed = slot_of[child[i]] == i / 2;
            if (win < m && (win < 1 || !closed || first || (m + win - 1) / win > KB_MAX_SWEEPS)) win = 0;
            const bool c_lds = win > 0;
            // (P in LDS implies the counters in LDS, as above); slot_of, child, sizes and n_changed: 4 B each behind them
            static_assert(KB_LDS_P_DOUBLES <= KB_LDS_COUNTERS, "a pass whose P fits the LDS keeps its counters there too");
            static_assert((size_t)KB_LDS_P_DOUBLES * 8 + (size_t)KB_LDS_COUNTERS * 4 + ((size_t)KB_MAX_NODES + 4 * KB_MAX_M + 1) * 4 <= 160 * 1024,
                          "P, the counters and the tables of the largest pass fit a CU's LDS");
            const size_t lds = (p_lds ? (size_t)(d_tot + 1) * (size_t)(k | 1) * 8 : 0) +
                               ((c_lds ? 2 * (size_t)win * (size_t)d_tot : 0) + (size_t)k + 1 + tabs.size()) * 4;
            auto go = p_lds ? bisect_launch<true, true, false>
                            : (!c_lds ? bisect_launch<false, false, false> : (win < m ? bisect_launch<false, true, true> : bisect_launch<false, true, false>));
            for (int s_lo = 0; s_lo < m; s_lo += c_lds ? win : m)
                go(grid, lds, s, t->codes.p, t->n, d_cd, (int)n_cols, (int)m, d_p, (long long)d_tot, d_tabs, (int)n_nodes, s_lo,
                   c_lds ? std::min(win, m - s_lo) : (int)m, first ? 1 : 0, rows_per_wg, t->km_assign.p, d_counts, d_out);
        });
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
