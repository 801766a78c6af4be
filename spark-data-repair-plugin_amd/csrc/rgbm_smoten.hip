// rgbm_smoten.hip -- a relational step next to the HBM-resident code table (what the steps share is rgbm_prep.h):
// =============================================================================================
// SMOTEN in code space (the over-sampling half of rebalance_training_data; the statement is repair/rebalance_codes.py), and
// rgbm_table_concat, which puts the pieces of the rebalanced training table together.  Every column is nominal, so the Value Difference
// Metric between two rows is a sum over the features of a quantity that depends on the pair of codes alone:
//   P_f[v][c] = (fit rows with code v in feature f and class c) / (fit rows with code v)          one double division
//   d_f(a, b) = (sum over the classes, ascending from 0.0, of |P_f[a][c] - P_f[b][c]|) squared    a plain product (vdm_pair)
//   dist      = sum over the features, in the caller's order from 0.0, of d_f
// All in double without contraction (the library is built with -ffp-contract=off -fno-fast-math): the bits of the numpy statement.
//   k_vdm_gather   the fit rows' target and feature codes, compacted [f][n_fit]; a code outside the dictionary raises the NULL flag
//   k_vdm_count    counts [V_f][K] per feature, 32-bit integer atomics;  k_vdm_prob: P_f
//   k_vdm_tables   D_f [V_f][V_f] for the features with V_f <= VDM_TABLE_CODES; the others are evaluated from P_f pair by pair, K terms
//                  each, by the same vdm_pair: both routes give the same bits
//   k_vdm_knn      a lane owns a query row of the class, the candidates stream through LDS in tiles of VDM_CAND_TILE rows; the pair tables
//                  sit in LDS when they fit beside the tiles, otherwise they are read where they lie.  A lane keeps its k best in registers
//                  and visits the candidates in ascending position with a strict <: the stable order by (distance, position).  The
//                  candidate range is split over blockIdx.y (a class of a few thousand rows has too few query tiles for 256 CUs); each
//                  split leaves a partial list
//   k_vdm_merge    joins the partial lists of a query in split order with the same strict <: splits hold ascending position ranges
//   k_vdm_emit     one thread per (new row, column): the class, the mode of the k neighbours' codes (ties: the smallest code), or -1
// One knn launch evaluates at most VDM_LAUNCH_PAIRS (query, candidate, feature) triples (RGBM_VDM_LAUNCH_PAIRS overrides it; the query
// tiles are spread over as many launches as that takes); RGBM_VDM_SPLITS overrides the number of candidate splits (tests).
// LDS of a workgroup: f x (VDM_QUERY_TILE + VDM_CAND_TILE) x 4 B of codes (80 KiB at the f limit) + the pair tables, VDM_LDS_BYTES at most.
// =============================================================================================
#include "rgbm_prep.h"

#include <cmath>
#include <limits>

namespace {

using namespace rgh;

constexpr int VDM_TABLE_CODES = 64;                 // a feature with at most this many codes gets a pair table
constexpr int VDM_QUERY_TILE = 256;                 // query rows of a workgroup = its threads
constexpr int VDM_CAND_TILE = 64;                   // candidate rows staged at a time
constexpr int VDM_MAX_K = 16;
constexpr int VDM_MAX_FEATURES = 64;
constexpr int VDM_MAX_SPLITS = 32;
constexpr int VDM_TARGET_WGS = 512;                 // workgroups a class should give: two per CU
constexpr long long VDM_LAUNCH_PAIRS = 1ll << 32;   // (query, candidate, feature) triples of one launch
constexpr long long VDM_MAX_P = 1ll << 28;          // entries of all P tables together
constexpr size_t VDM_LDS_BYTES = 158 * 1024;

struct VdmFeat { long long p_off; int32_t d_off; int32_t V; int32_t has_table; int32_t pad_; };

__device__ __forceinline__ double vdm_pair(const double* __restrict__ p, int K, int a, int b) {
    const double* pa = p + (long long)a * K;
    const double* pb = p + (long long)b * K;
    double s = 0.0;
    for (int c = 0; c < K; ++c) s = s + fabs(pa[c] - pb[c]);
    return s * s;
}

// (d, idx) into the ascending list bd / bi of k <= KM entries, behind every entry that is not larger: the caller has seen d < worst
template <int KM>
__device__ __forceinline__ void vdm_insert(double (&bd)[KM], int (&bi)[KM], double& worst, int k, double d, int idx) {
    bool placed = false;
#pragma unroll
    for (int s = KM - 1; s >= 0; --s) {
        if (s < k && !placed) {
            bool shift = false;
            if (s > 0) shift = d < bd[s > 0 ? s - 1 : 0];
            if (shift) { bd[s] = bd[s > 0 ? s - 1 : 0]; bi[s] = bi[s > 0 ? s - 1 : 0]; }
            else { bd[s] = d; bi[s] = idx; placed = true; }
        }
    }
#pragma unroll
    for (int s = 0; s < KM; ++s) if (s == k - 1) worst = bd[s];
}

// blockIdx.y = feature, f = the target: x [f][n_fit] / y [n_fit]
__global__ __launch_bounds__(256) void k_vdm_gather(const int32_t* __restrict__ codes, long long n, const long long* __restrict__ fit, long long n_fit,
                                                    const int32_t* __restrict__ cols, const int32_t* __restrict__ ncodes, int f,
                                                    int32_t* __restrict__ x, int32_t* __restrict__ y, unsigned* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_fit) return;
    const int j = (int)blockIdx.y;
    int32_t v = codes[(long long)cols[j] * n + fit[i]];
    if (v < 0 || v >= ncodes[j]) { atomicOr(bad, 1u); v = 0; }
    if (j < f) x[(long long)j * n_fit + i] = v; else y[i] = v;
}

__global__ __launch_bounds__(256) void k_vdm_count(const int32_t* __restrict__ x, const int32_t* __restrict__ y, long long n_fit,
                                                   const VdmFeat* __restrict__ feats, int K, unsigned* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_fit) return;
    const int j = (int)blockIdx.y;
    atomicAdd(&cnt[feats[j].p_off + (long long)x[(long long)j * n_fit + i] * K + y[i]], 1u);
}

// one thread per (feature, code): the row sum is an integer, so any order of adding gives the double the statement divides by
__global__ __launch_bounds__(256) void k_vdm_prob(const unsigned* __restrict__ cnt, const VdmFeat* __restrict__ feats, int K, double* __restrict__ p) {
    const VdmFeat ft = feats[blockIdx.y];
    const int v = (int)(blockIdx.x * 256 + threadIdx.x);
    if (v >= ft.V) return;
    const long long o = ft.p_off + (long long)v * K;
    unsigned long long s = 0;
    for (int c = 0; c < K; ++c) s += cnt[o + c];
    const double sd = (double)s;
    for (int c = 0; c < K; ++c) p[o + c] = s ? (double)cnt[o + c] / sd : 0.0;
}

__global__ __launch_bounds__(256) void k_vdm_tables(const double* __restrict__ p, const VdmFeat* __restrict__ feats, int K, double* __restrict__ d) {
    const VdmFeat ft = feats[blockIdx.y];
    const int e = (int)(blockIdx.x * 256 + threadIdx.x);
    if (!ft.has_table || e >= ft.V * ft.V) return;
    d[ft.d_off + e] = vdm_pair(p + ft.p_off, K, e / ft.V, e % ft.V);
}

// grid (query tiles of this launch, candidate splits).  LDS: [d_lds doubles: the pair tables] [f][QUERY_TILE] [f][CAND_TILE] ints.
// A query's slot of feature j holds d_off + a * V (the row of its pair table) or, without a table, -(1 + a).
template <int KM>
__global__ __launch_bounds__(VDM_QUERY_TILE) void k_vdm_knn(const int32_t* __restrict__ x, long long n_fit, const int32_t* __restrict__ rows, int m, int f,
                                                            const VdmFeat* __restrict__ feats, const double* __restrict__ p,
                                                            const double* __restrict__ d_tab, int d_lds, int K, int k, int q_begin,
                                                            int cand_per_split, double* __restrict__ part_d, int32_t* __restrict__ part_i) {
    extern __shared__ double vdm_lds[];
    int* lq = reinterpret_cast<int*>(vdm_lds + d_lds);
    int* lc = lq + f * VDM_QUERY_TILE;
    const double* tab = d_lds ? vdm_lds : d_tab;
    const int tid = (int)threadIdx.x;
    const int q = q_begin + (int)blockIdx.x * VDM_QUERY_TILE + tid;
    const bool live = q < m;
    for (int i = tid; i < d_lds; i += VDM_QUERY_TILE) vdm_lds[i] = d_tab[i];
    const long long qrow = live ? rows[q] : 0;
    for (int j = 0; j < f; ++j) {
        const VdmFeat ft = feats[j];
        const int a = live ? x[(long long)j * n_fit + qrow] : 0;
        lq[j * VDM_QUERY_TILE + tid] = ft.has_table ? ft.d_off + a * ft.V : -(1 + a);
    }
    const int c0 = (int)blockIdx.y * cand_per_split, c1 = min(m, c0 + cand_per_split);
    double bd[KM]; int bi[KM];
#pragma unroll
    for (int s = 0; s < KM; ++s) { bd[s] = std::numeric_limits<double>::infinity(); bi[s] = -1; }
    double worst = std::numeric_limits<double>::infinity();
    for (int t0 = c0; t0 < c1; t0 += VDM_CAND_TILE) {
        const int nt = min(VDM_CAND_TILE, c1 - t0);
        __syncthreads();                                   // the tile before this one has been read (first tile: nothing)
        for (int i = tid; i < f * VDM_CAND_TILE; i += VDM_QUERY_TILE) {
            const int j = i / VDM_CAND_TILE, e = i % VDM_CAND_TILE;
            if (e < nt) lc[i] = x[(long long)j * n_fit + rows[t0 + e]];
        }
        __syncthreads();                                   // (covers the tables and the query slots as well)
        if (live) {
            for (int e = 0; e < nt; ++e) {
                const int cj = t0 + e;
                if (cj == q) continue;
                double dist = 0.0;
                for (int j = 0; j < f; ++j) {
                    const int qa = lq[j * VDM_QUERY_TILE + tid], b = lc[j * VDM_CAND_TILE + e];
                    dist = dist + (qa >= 0 ? tab[qa + b] : vdm_pair(p + feats[j].p_off, K, -1 - qa, b));
                }
                if (dist < worst) vdm_insert<KM>(bd, bi, worst, k, dist, cj);
            }
        }
    }
    if (live) {
        const long long o = ((long long)blockIdx.y * m + q) * k;
#pragma unroll
        for (int s = 0; s < KM; ++s) if (s < k) { part_d[o + s] = bd[s]; part_i[o + s] = bi[s]; }
    }
}

template <int KM>
__global__ __launch_bounds__(256) void k_vdm_merge(const double* __restrict__ part_d, const int32_t* __restrict__ part_i, int m, int k, int splits,
                                                   long long* __restrict__ nn) {
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= m) return;
    double bd[KM]; int bi[KM];
#pragma unroll
    for (int s = 0; s < KM; ++s) { bd[s] = std::numeric_limits<double>::infinity(); bi[s] = -1; }
    double worst = std::numeric_limits<double>::infinity();
    for (int sp = 0; sp < splits; ++sp) {
        const long long o = ((long long)sp * m + q) * k;
        for (int e = 0; e < k; ++e) {
            const int idx = part_i[o + e];
            if (idx < 0) break;
            const double d = part_d[o + e];
            if (d < worst) vdm_insert<KM>(bd, bi, worst, k, d, idx);
        }
    }
#pragma unroll
    for (int s = 0; s < KM; ++s) if (s < k) nn[(long long)q * k + s] = bi[s];
}

// grid (new rows of the class, columns).  role[col]: the feature's index, -1 (no part: NULL) or -2 (the target)
__global__ __launch_bounds__(256) void k_vdm_emit(const int32_t* __restrict__ x, long long n_fit, const int32_t* __restrict__ rows, int m,
                                                  const long long* __restrict__ nn, int k, const long long* __restrict__ picks, long long n_new,
                                                  const int32_t* __restrict__ role, int32_t klass, int32_t* __restrict__ out, long long n_out,
                                                  long long out_base) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_new) return;
    const int col = (int)blockIdx.y, r = role[col];
    int32_t v = -1;
    if (r == -2) v = klass;
    else if (r >= 0) {
        const long long* mine = nn + picks[i] * k;
        int32_t cs[VDM_MAX_K];
#pragma unroll
        for (int e = 0; e < VDM_MAX_K; ++e) {
            const long long nb = e < k ? mine[e] : -1;
            cs[e] = (nb >= 0 && nb < m) ? x[(long long)r * n_fit + rows[nb]] : -1;
        }
        int best = 0;
#pragma unroll
        for (int e = 0; e < VDM_MAX_K; ++e) {
            int cnt = 0;
#pragma unroll
            for (int g = 0; g < VDM_MAX_K; ++g) cnt += (cs[e] >= 0 && cs[g] == cs[e]) ? 1 : 0;
            if (cnt > best || (cnt == best && cnt > 0 && cs[e] < v)) { best = cnt; v = cs[e]; }
        }
    }
    out[(long long)col * n_out + out_base + i] = v;
}

// blockIdx.y = column: the rows of one part behind those of the parts before it
__global__ __launch_bounds__(256) void k_concat_part(const int32_t* __restrict__ in, long long n_in, int32_t* __restrict__ out, long long n_out,
                                                     long long base) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_in) out[(long long)blockIdx.y * n_out + base + i] = in[(long long)blockIdx.y * n_in + i];
}

// the candidate splits of a class of m rows: whole candidate tiles each, none empty
struct VdmSplit { int splits, cand_per_split; };
VdmSplit vdm_split(int m, int splits_wanted) {
    const int qtiles = (int)nblocks(m, VDM_QUERY_TILE), ctiles = (int)nblocks(m, VDM_CAND_TILE);
    int splits = splits_wanted > 0 ? splits_wanted : (VDM_TARGET_WGS + qtiles - 1) / qtiles;
    splits = std::max(1, std::min(splits, std::min(VDM_MAX_SPLITS, ctiles)));
    const int cand_per_split = (ctiles + splits - 1) / splits * VDM_CAND_TILE;
    return VdmSplit{(m + cand_per_split - 1) / cand_per_split, cand_per_split};
}

// part_d / part_i hold splits x m x k entries at least
template <int KM>
void knn_class(hipStream_t s, const int32_t* d_x, long long n_fit, const int32_t* d_rows, int m, int f, const VdmFeat* d_feats, const double* d_p,
               const double* d_tab, int d_lds, int K, int k, long long launch_pairs, int splits_wanted, const DevBuf<double>& part_d,
               const DevBuf<int32_t>& part_i, long long* d_nn) {
    const int qtiles = (int)nblocks(m, VDM_QUERY_TILE);
    const int splits = vdm_split(m, splits_wanted).splits, cand_per_split = vdm_split(m, splits_wanted).cand_per_split;
    const size_t lds = (size_t)d_lds * 8 + (size_t)f * (VDM_QUERY_TILE + VDM_CAND_TILE) * 4;
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_vdm_knn<KM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)VDM_LDS_BYTES));
    const long long per_tile = (long long)VDM_QUERY_TILE * m * f;
    const int tiles_per_launch = (int)std::max<long long>(1, std::min<long long>(qtiles, launch_pairs / per_tile));
    for (int t0 = 0; t0 < qtiles; t0 += tiles_per_launch) {
        const int nt = std::min(tiles_per_launch, qtiles - t0);
        hipLaunchKernelGGL((k_vdm_knn<KM>), dim3((unsigned)nt, (unsigned)splits), dim3(VDM_QUERY_TILE), lds, s, d_x, n_fit, d_rows, m, f, d_feats, d_p,
                           d_tab, d_lds, K, k, t0 * VDM_QUERY_TILE, cand_per_split, part_d.p, part_i.p);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL((k_vdm_merge<KM>), dim3(nblocks(m, 256)), dim3(256), 0, s, part_d.p, part_i.p, m, k, splits, d_nn);
    HIPCHK(hipGetLastError());
}

}  // namespace

extern "C" {

RGBM_EXPORT int rgbm_table_smoten(const rgbm_table* t, int32_t target_col, const int32_t* feat_cols, int32_t f, const int64_t* fit_rows,
                                  int64_t n_fit, int32_t k, const int32_t* classes, int32_t n_classes, const int64_t* pick_off,
                                  const int64_t* picks, int64_t* nn_out, rgbm_table** out) {
    if (!t || !feat_cols || f < 1 || !fit_rows || n_fit < 1 || !classes || n_classes < 1 || !pick_off || !picks || !out)
        return fail(RGBM_ERR_ARG, "rgbm_table_smoten: bad argument (at least one feature, fit row and class)");
    return guarded([&]() {
        use_device(t->device);
        if (k < 1 || k > VDM_MAX_K) throw std::invalid_argument("rgbm_table_smoten: k outside 1 .. 16");
        if (f > VDM_MAX_FEATURES) throw std::invalid_argument("rgbm_table_smoten: more than 64 features");
        if (n_fit >= (1ll << 31)) throw std::invalid_argument("rgbm_table_smoten: 2^31 fit rows or more");
        check_cols(*t, &target_col, 1, "rgbm_table_smoten: target column");
        check_cols(*t, feat_cols, f, "rgbm_table_smoten: feature column");
        std::vector<int32_t> role((size_t)t->c, -1), cols((size_t)f + 1), ncodes((size_t)f + 1);
        role[target_col] = -2;
        for (int j = 0; j < f; ++j) {
            if (role[feat_cols[j]] != -1) throw std::invalid_argument("rgbm_table_smoten: a feature column is listed twice or is the target");
            role[feat_cols[j]] = j; cols[j] = feat_cols[j]; ncodes[j] = t->n_codes[feat_cols[j]];
        }
        cols[f] = target_col; ncodes[f] = t->n_codes[target_col];
        const int K = t->n_codes[target_col];
        if (K < 1) throw std::invalid_argument("rgbm_table_smoten: the target column has no code");
        if (pick_off[0] != 0) throw std::invalid_argument("rgbm_table_smoten: pick_off does not start at 0");
        for (int ci = 0; ci < n_classes; ++ci) {
            if (classes[ci] < 0 || classes[ci] >= K || (ci > 0 && classes[ci] <= classes[ci - 1]))
                throw std::invalid_argument("rgbm_table_smoten: the classes are not ascending codes of the target");
            if (pick_off[ci + 1] < pick_off[ci]) throw std::invalid_argument("rgbm_table_smoten: pick_off decreases");
        }
        const int64_t n_out = pick_off[n_classes];
        if (n_out < 1) throw std::invalid_argument("rgbm_table_smoten: no row to make");
        for (int64_t i = 0; i < n_fit; ++i)
            if (fit_rows[i] < 0 || fit_rows[i] >= t->n) throw std::invalid_argument("rgbm_table_smoten: fit row position out of range");
        std::vector<VdmFeat> feats((size_t)f);
        long long p_tot = 0; int d_tot = 0;
        for (int j = 0; j < f; ++j) {
            const int V = ncodes[j];
            feats[j].p_off = p_tot; feats[j].V = V; feats[j].has_table = V <= VDM_TABLE_CODES; feats[j].d_off = d_tot; feats[j].pad_ = 0;
            p_tot += (long long)V * K;
            if (p_tot > VDM_MAX_P) throw std::invalid_argument("rgbm_table_smoten: the P tables hold more than 2^28 entries");
            if (feats[j].has_table) d_tot += V * V;
        }
        long long launch_pairs = VDM_LAUNCH_PAIRS; int splits_wanted = 0;
        if (const char* e = getenv("RGBM_VDM_LAUNCH_PAIRS")) launch_pairs = std::max<long long>(1, atoll(e));
        if (const char* e = getenv("RGBM_VDM_SPLITS")) splits_wanted = (int)std::max<long long>(0, std::min<long long>(atoll(e), VDM_MAX_SPLITS));

        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const size_t NF = (size_t)n_fit;
        DevBuf<long long> d_fit(NF); DevBuf<int32_t> d_x((size_t)f * NF), d_y(NF), d_cols((size_t)f + 1), d_ncodes((size_t)f + 1);
        DevBuf<unsigned> d_bad(1);
        d_fit.upload(reinterpret_cast<const long long*>(fit_rows), NF, s);
        d_cols.upload(cols.data(), cols.size(), s); d_ncodes.upload(ncodes.data(), ncodes.size(), s);
        d_bad.zero(s);
        hipLaunchKernelGGL(k_vdm_gather, dim3(nblocks(n_fit, 256), (unsigned)f + 1), dim3(256), 0, s, t->codes.p, (long long)t->n, d_fit.p, (long long)n_fit,
                           d_cols.p, d_ncodes.p, (int)f, d_x.p, d_y.p, d_bad.p);
        HIPCHK(hipGetLastError());
        std::vector<int32_t> y(NF); unsigned bad = 0;
        d_y.download(y.data(), NF, s); d_bad.download(&bad, 1, s);
        HIPCHK(hipStreamSynchronize(s));
        if (bad) throw std::invalid_argument("rgbm_table_smoten: a fit row holds a NULL in the target or a feature");

        // the rows of every class, as positions within the fit rows, in their order
        std::vector<int32_t> cls_of((size_t)K, -1);
        for (int ci = 0; ci < n_classes; ++ci) cls_of[classes[ci]] = ci;
        std::vector<long long> m_of((size_t)n_classes, 0), row_off((size_t)n_classes + 1, 0);
        for (size_t i = 0; i < NF; ++i) if (cls_of[y[i]] >= 0) ++m_of[cls_of[y[i]]];
        for (int ci = 0; ci < n_classes; ++ci) {
            if (m_of[ci] <= k) throw std::invalid_argument("rgbm_table_smoten: a class with no more than k fit rows");
            row_off[ci + 1] = row_off[ci] + m_of[ci];
            for (int64_t i = pick_off[ci]; i < pick_off[ci + 1]; ++i)
                if (picks[i] < 0 || picks[i] >= m_of[ci]) throw std::invalid_argument("rgbm_table_smoten: a pick outside its class");
        }
        const size_t M = (size_t)row_off[n_classes];
        std::vector<int32_t> rows(M); std::vector<long long> fill(row_off.begin(), row_off.end() - 1);
        for (size_t i = 0; i < NF; ++i) if (cls_of[y[i]] >= 0) rows[(size_t)fill[cls_of[y[i]]]++] = (int32_t)i;

        DevBuf<VdmFeat> d_feats((size_t)f); DevBuf<unsigned> d_cnt((size_t)p_tot); DevBuf<double> d_p((size_t)p_tot), d_tab((size_t)std::max(d_tot, 1));
        DevBuf<int32_t> d_rows(M), d_role((size_t)t->c); DevBuf<long long> d_picks((size_t)n_out), d_nn(M * (size_t)k);
        d_feats.upload(feats.data(), feats.size(), s); d_rows.upload(rows.data(), M, s); d_role.upload(role.data(), role.size(), s);
        d_picks.upload(reinterpret_cast<const long long*>(picks), (size_t)n_out, s);
        d_cnt.zero(s);
        int v_max = 1;
        for (int j = 0; j < f; ++j) v_max = std::max(v_max, ncodes[j]);
        hipLaunchKernelGGL(k_vdm_count, dim3(nblocks(n_fit, 256), (unsigned)f), dim3(256), 0, s, d_x.p, d_y.p, (long long)n_fit, d_feats.p, K, d_cnt.p);
        hipLaunchKernelGGL(k_vdm_prob, dim3(nblocks(v_max, 256), (unsigned)f), dim3(256), 0, s, d_cnt.p, d_feats.p, K, d_p.p);
        if (d_tot > 0)
            hipLaunchKernelGGL(k_vdm_tables, dim3(nblocks(VDM_TABLE_CODES * VDM_TABLE_CODES, 256), (unsigned)f), dim3(256), 0, s, d_p.p, d_feats.p, K, d_tab.p);
        HIPCHK(hipGetLastError());

        std::unique_ptr<rgbm_table> o(new rgbm_table());
        o->device = t->device; o->n = n_out; o->c = t->c; o->n_codes = t->n_codes; o->col_values = t->col_values; o->col_kind = t->col_kind;
        o->codes.alloc((size_t)n_out * t->c);
        const size_t tile_bytes = (size_t)f * (VDM_QUERY_TILE + VDM_CAND_TILE) * 4;
        const int d_lds = (d_tot > 0 && tile_bytes + (size_t)d_tot * 8 <= VDM_LDS_BYTES) ? d_tot : 0;
        size_t part_n = 1;
        for (int ci = 0; ci < n_classes; ++ci) part_n = std::max(part_n, (size_t)vdm_split((int)m_of[ci], splits_wanted).splits * (size_t)m_of[ci] * (size_t)k);
        DevBuf<double> part_d(part_n); DevBuf<int32_t> part_i(part_n);
        for (int ci = 0; ci < n_classes; ++ci) {
            const int m = (int)m_of[ci];
            const int32_t* cr = d_rows.p + row_off[ci];
            long long* cnn = d_nn.p + row_off[ci] * k;
            if (k <= 8) knn_class<8>(s, d_x.p, n_fit, cr, m, f, d_feats.p, d_p.p, d_tab.p, d_lds, K, k, launch_pairs, splits_wanted, part_d, part_i, cnn);
            else knn_class<16>(s, d_x.p, n_fit, cr, m, f, d_feats.p, d_p.p, d_tab.p, d_lds, K, k, launch_pairs, splits_wanted, part_d, part_i, cnn);
            const long long n_new = pick_off[ci + 1] - pick_off[ci];
            if (n_new > 0) {
                hipLaunchKernelGGL(k_vdm_emit, dim3(nblocks(n_new, 256), (unsigned)t->c), dim3(256), 0, s, d_x.p, (long long)n_fit, cr, m, cnn, (int)k,
                                   d_picks.p + pick_off[ci], n_new, d_role.p, classes[ci], o->codes.p, (long long)n_out, (long long)pick_off[ci]);
                HIPCHK(hipGetLastError());
            }
        }
        if (nn_out) d_nn.download(reinterpret_cast<long long*>(nn_out), M * (size_t)k, s);
        HIPCHK(hipStreamSynchronize(s));
        *out = o.release();
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_concat(const rgbm_table* const* parts, int32_t n_parts, rgbm_table** out) {
    if (!parts || n_parts < 1 || !out) return fail(RGBM_ERR_ARG, "rgbm_table_concat: bad argument (at least one part)");
    for (int i = 0; i < n_parts; ++i) if (!parts[i]) return fail(RGBM_ERR_ARG, "rgbm_table_concat: a part is NULL");
    return guarded([&]() {
        const rgbm_table* a = parts[0];
        use_device(a->device);
        int64_t n_out = 0;
        for (int i = 0; i < n_parts; ++i) {
            const rgbm_table* b = parts[i];
            if (b->device != a->device || b->c != a->c || b->n_codes != a->n_codes || b->col_kind != a->col_kind || b->col_values != a->col_values)
                throw std::invalid_argument("rgbm_table_concat: the parts differ in shape, dictionaries or device");
            n_out += b->n;
        }
        StreamGuard sg;
        std::unique_ptr<rgbm_table> o(new rgbm_table());
        o->device = a->device; o->n = n_out; o->c = a->c; o->n_codes = a->n_codes; o->col_values = a->col_values; o->col_kind = a->col_kind;
        o->codes.alloc((size_t)n_out * a->c);
        long long base = 0;
        for (int i = 0; i < n_parts; ++i) {
            const rgbm_table* b = parts[i];
            hipLaunchKernelGGL(k_concat_part, dim3(nblocks(b->n, 256), (unsigned)b->c), dim3(256), 0, sg.s, b->codes.p, (long long)b->n, o->codes.p,
                               (long long)n_out, base);
            base += b->n;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(sg.s));
        *out = o.release();
        return RGBM_OK;
    });
}

}  // extern "C"
