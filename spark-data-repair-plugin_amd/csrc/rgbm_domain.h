// rgbm_domain.h -- the ONE copy of the cell-domain arithmetic (internal, never installed), for the two sources whose kernels evaluate it:
// rgbm_domain.hip (k_cell_domains: the cells the caller lists) and rgbm_cellset.hip (k_cs_drop_weak: the cells of the table's cell set).
// Without relocatable device code a kernel is compiled into the source that launches it, so the body is a __device__ function here.
// The value-space statement is repair/domain.py cell_domains, which it must equal -- counts exactly, probabilities bit for bit.
#pragma once
#include "rgbm_prep.h"

namespace rgh {

constexpr int DOM_MAXK = 8;                                 // correlated attributes of one cell-domain call

struct DomAttr { long long off, sn, sv, min_cnt; int32_t col, d_c; };
struct DomCell { bool weak; int32_t top; double top_prob; };

// bin of (row r, column col): the code through the column's LUT (if any); NULL / out of range -> slot d = nbins
__device__ __forceinline__ int pc_bin(const int32_t* __restrict__ codes, long long n, int col, long long r, const int32_t* __restrict__ colinfo,
                                      const long long* __restrict__ lut_off, const int32_t* __restrict__ luts) {
    int v = codes[(long long)col * n + r];
    const int nc = colinfo[2 * col], d = colinfo[2 * col + 1];
    if (v < 0 || v >= nc) return d;
    const long long lo = lut_off[col];
    if (lo >= 0) v = luts[lo + v];
    return (v < 0 || v >= d) ? d : v;
}

// the domain of the cell (row r, column target): the fixed-order score sums and the divisions of repair/domain.py, nothing else.
// probs_row: d_a probabilities of the cell, or null.  A row outside the table has an empty domain.
__device__ __forceinline__ DomCell cell_domain(const int32_t* __restrict__ codes, long long n, int target, int d_a, long long r,
                                               const unsigned long long* __restrict__ joint, const DomAttr* __restrict__ attrs, int k,
                                               const int32_t* __restrict__ colinfo, const long long* __restrict__ lut_off,
                                               const int32_t* __restrict__ luts, const uint8_t* __restrict__ single_ok, double beta,
                                               double row_count, double* __restrict__ probs_row) {
    const bool inside = r >= 0 && r < n;
    const unsigned long long* base[DOM_MAXK]; long long sn[DOM_MAXK], mc[DOM_MAXK];
    // the fold  IF(ISNOTNULL(domain), CONCAT(domain, d), d):  an attribute whose element list is NULL (value NULL / no group above the
    // threshold) wipes what came before it, so only the attributes after the last such one contribute
    int j0 = k;
    if (inside) {
        j0 = 0;
#pragma unroll
        for (int j = 0; j < DOM_MAXK; ++j) {
            if (j >= k) break;
            const DomAttr a = attrs[j];
            const int v = pc_bin(codes, n, a.col, r, colinfo, lut_off, luts);
            base[j] = joint + a.off + (long long)(v < a.d_c ? v : 0) * a.sv; sn[j] = a.sn; mc[j] = a.min_cnt;
            bool has = false;
            if (v < a.d_c) for (int c = 0; c < d_a; ++c) if ((long long)base[j][(long long)c * a.sn] > a.min_cnt) { has = true; break; }
            if (!has) j0 = j + 1;
        }
    }
    auto score = [&](int c) -> double {
        double s = 0.0;
        if (!single_ok[c]) return s;
#pragma unroll
        for (int j = 0; j < DOM_MAXK; ++j) {
            if (j >= k) break;
            if (j < j0) continue;
            const long long cnt = (long long)base[j][(long long)c * sn[j]];
            if (cnt > mc[j]) { const double b = fmax((double)cnt - 1.0, 0.1); s = s + b / row_count; }
        }
        return s;
    };
    double den = 0.0;
    if (j0 < k) for (int c = 0; c < d_a; ++c) den = den + score(c);          // ascending code, sequential
    double best = 0.0; int bt = -1;
    for (int c = 0; c < d_a; ++c) {
        const double p = (j0 < k && den > 0.0) ? score(c) / den : 0.0;
        if (probs_row) probs_row[c] = p;
        if (p > best) { best = p; bt = c; }                                   // first maximum: ties by ascending code
    }
    const bool valid = bt >= 0 && best > beta;
    int cur = inside ? codes[(long long)target * n + r] : -1;
    if (cur >= d_a) cur = -1;
    return DomCell{valid && cur >= 0 && cur == bt, valid ? bt : -1, valid ? best : 0.0};
}

// the RGBM_ERR_PARAM refusals that rgbm_table_cell_domains and rgbm_table_cellset_drop_weak share (thrown under `entry`'s name), and the
// attribute descriptors of the pairs `pair_idx` [k] of the table's last rgbm_table_pair_counts call
inline std::vector<DomAttr> dom_attrs(const rgbm_table& t, int32_t target_col, const int32_t* pair_idx, int32_t k, const int64_t* min_cnt,
                                      const std::string& entry) {
    if (k > DOM_MAXK) throw std::invalid_argument(entry + ": more than 8 correlated attributes");
    if (t.pc_nbins.empty()) throw std::invalid_argument(entry + ": no rgbm_table_pair_counts result on this table");
    if (t.pc_has_lut[target_col]) throw std::invalid_argument(entry + ": the target must be a discrete attribute (no LUT)");
    std::vector<DomAttr> attrs((size_t)std::max(k, 1));
    for (int j = 0; j < k; ++j) {
        const int p = pair_idx[j];
        if (p < 0 || p >= (int)t.pc_x.size()) throw std::invalid_argument(entry + ": pair index out of range");
        DomAttr a;
        a.off = t.pc_off[p]; a.min_cnt = std::max<long long>(min_cnt[j], 0);
        if (t.pc_x[p] == target_col) { a.col = t.pc_y[p]; a.d_c = t.pc_dy[p]; a.sn = (long long)t.pc_dy[p] + 1; a.sv = 1; }
        else if (t.pc_y[p] == target_col) { a.col = t.pc_x[p]; a.d_c = t.pc_dx[p]; a.sn = 1; a.sv = (long long)t.pc_dy[p] + 1; }
        else throw std::invalid_argument(entry + ": a pair does not hold the target column");
        attrs[j] = a;
    }
    return attrs;
}

}  // namespace rgh
