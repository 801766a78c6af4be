// rgbm_pmf.hip -- candidate distributions and edit distances on the HBM-resident code table (a relational step; what the steps share is
// rgbm_prep.h).  The one source that includes rgbm_cost.h, whose kernels are launched here and nowhere else:
//   repair_pmf[_weighted] candidate distributions of the NULL cells, optionally re-weighted by update costs (rgbm_cost.h)
//   edit_distance         Levenshtein matrix of two string pools (the Levenshtein update cost, rgbm_cost.h)
#include "rgbm_prep.h"
#include "rgbm_cost.h"

namespace rgh {

void edit_distance_on_device(const int32_t* a_cp, const int64_t* a_off, int64_t n_a, const int32_t* b_cp, const int64_t* b_off, int64_t n_b,
                             int32_t* d_dist, hipStream_t s) {
    const size_t na_cp = (size_t)a_off[n_a], nb_cp = (size_t)b_off[n_b];
    DevBuf<int32_t> d_a(std::max<size_t>(na_cp, 1)), d_b(std::max<size_t>(nb_cp, 1));
    DevBuf<int64_t> d_ao((size_t)n_a + 1), d_bo((size_t)n_b + 1);
    d_a.upload(a_cp, na_cp, s); d_b.upload(b_cp, nb_cp, s);
    d_ao.upload(a_off, (size_t)n_a + 1, s); d_bo.upload(b_off, (size_t)n_b + 1, s);
    const unsigned gx = nblocks(n_a, rgbm_cost::ED_BLOCK);
    for (int64_t j0 = 0; j0 < n_b; j0 += 65535) {
        const unsigned gy = (unsigned)std::min<int64_t>(n_b - j0, 65535);
        hipLaunchKernelGGL(k_edit_distance, dim3(gx, gy), dim3(rgbm_cost::ED_BLOCK), 0, s, d_a.p, d_ao.p, (long long)n_a, d_b.p, d_bo.p,
                           (long long)n_b, (long long)j0, d_dist);
    }
    // pairs with both strings longer than one 64-bit pattern word: the anti-diagonal DP, one workgroup per pair
    std::vector<int64_t> la, lb;
    for (int64_t j = 0; j < n_b; ++j) if (b_off[j + 1] - b_off[j] > rgbm_cost::ED_PAT) lb.push_back(j);
    if (!lb.empty()) for (int64_t i = 0; i < n_a; ++i) if (a_off[i + 1] - a_off[i] > rgbm_cost::ED_PAT) la.push_back(i);
    DevBuf<int64_t> d_pa, d_pb, d_so; DevBuf<int32_t> d_scr;
    if (!la.empty() && !lb.empty()) {
        std::vector<int64_t> pa, pb, so;
        int64_t tot = 0;
        for (int64_t i : la) for (int64_t j : lb) {
            pa.push_back(i); pb.push_back(j); so.push_back(tot);
            tot += 3 * (std::min(a_off[i + 1] - a_off[i], b_off[j + 1] - b_off[j]) + 2);
        }
        d_pa.alloc(pa.size()); d_pa.upload(pa.data(), pa.size(), s);
        d_pb.alloc(pb.size()); d_pb.upload(pb.data(), pb.size(), s);
        d_so.alloc(so.size()); d_so.upload(so.data(), so.size(), s);
        d_scr.alloc((size_t)tot);
        for (size_t p0 = 0; p0 < pa.size(); p0 += (1u << 30)) {
            const size_t cnt = std::min<size_t>(pa.size() - p0, 1u << 30);
            hipLaunchKernelGGL(k_edit_distance_long, dim3((unsigned)cnt), dim3(64), 0, s, d_a.p, d_ao.p, d_b.p, d_bo.p, (long long)n_b,
                               d_pa.p + p0, d_pb.p + p0, d_so.p + p0, d_scr.p, d_dist);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
}

}  // namespace rgh

namespace {

using namespace rgh;

// ---------------------------------------------------------------------------------------------
// candidate distributions (python/repair/model.py:1196-1212): per cell, classes by descending probability (ties keep
// class order), those > threshold, at most top_k -- k_weighted_pmf (rgbm_cost.h), which without a cost matrix and without renormalisation
// leaves the probabilities as they are.  The body of rgbm_table_repair_pmf (weighted = false: no costs, the caller passes cost_row, cost
// and top1_cost_out null, n_cost_rows 0, renormalise 0) and of rgbm_table_repair_pmf_weighted; the error texts carry the entry's name.
// scratch slots held together: COLS | BALLOTS BCOUNT BOFF
// ---------------------------------------------------------------------------------------------
int repair_pmf(bool weighted, rgbm_table* t, const rgbm_model* m, int32_t target_col, const int32_t* feat_cols, int32_t f, int32_t top_k, double threshold,
               const int32_t* cur_code, const int32_t* cost_row, const double* cost, int64_t n_cost_rows, double weight, int32_t renormalise, int64_t cap,
               int64_t* n_cells_out, int64_t* rows_out, int32_t* class_out, double* prob_out, double* cur_prob_out, double* top1_cost_out) {
    const char* entry = weighted ? "rgbm_table_repair_pmf_weighted" : "rgbm_table_repair_pmf";
    if (!t || !m || !feat_cols || f <= 0 || target_col < 0 || target_col >= t->c || top_k <= 0 || !n_cells_out || cap < 0 || n_cost_rows < 0 ||
        (cost_row && !cost))
        return fail(RGBM_ERR_ARG, std::string(entry) + ": bad argument");
    return guarded([&]() {
        use_device(t->device);
        check_cols(*t, feat_cols, f, entry);
        int32_t obj = 0, K = 0, F = 0;
        model_shape(m, &obj, &K, &F);
        if (obj == 2)
            throw std::invalid_argument(std::string(entry) + ": a regressor has no class distribution" + (weighted ? "" : " (model.py:1214-1221 handles continuous attributes)"));
        if (F != f) throw std::invalid_argument(std::string(entry) + ": the model was trained on a different number of features");
        if (cost && (unsigned long long)(n_cost_rows + 1) * (unsigned long long)K > (1ull << 28))
            throw std::invalid_argument(std::string(entry) + ": the cost matrix holds more than 2^28 entries");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const int32_t* d_tc = scr_upload<int32_t>(*t, SCR_COLS, &target_col, 1, s);
        const long long cells = compact<0>(*t, nullptr, d_tc, 1, false, s);      // ascending rows whose target cell is NULL
        *n_cells_out = cells;
        if (cells == 0) return RGBM_OK;
        if (cells > cap) throw std::invalid_argument(std::string(entry) + ": output capacity too small (n_cells_out holds the needed size)");
        if (!rows_out || !class_out || !prob_out) throw std::invalid_argument(std::string(entry) + ": output arrays missing");
        if (cost_row)
            for (long long i = 0; i < cells; ++i)
                if (cost_row[i] < -1 || cost_row[i] >= n_cost_rows) throw std::invalid_argument(std::string(entry) + ": cost_row out of range");
        // the cells' rows as a small code block, scored in one go
        DevBuf<int32_t> sub((size_t)cells * t->c);
        launch_gather_rows(t->codes.p, (long long)t->n, (int)t->c, sub.p, cells, t->cell_rows.p, s);
        DevBuf<int32_t> d_fc((size_t)f); d_fc.upload(feat_cols, (size_t)f, s);
        DevBuf<double> proba((size_t)cells * K);
        predict_proba_device(m, t->device, s, sub.p, cells, d_fc.p, proba.p);
        DevBuf<int32_t> d_cls((size_t)cells * top_k); DevBuf<double> d_pr((size_t)cells * top_k);
        DevBuf<int32_t> d_cur, d_row; DevBuf<double> d_cp, d_cost, d_tc1;
        if (cur_prob_out) { d_cp.alloc((size_t)cells); if (cur_code) { d_cur.alloc((size_t)cells); d_cur.upload(cur_code, (size_t)cells, s); } }
        if (cost) { d_cost.alloc((size_t)(n_cost_rows + 1) * K); d_cost.upload(cost, (size_t)(n_cost_rows + 1) * K, s); }
        if (cost_row) { d_row.alloc((size_t)cells); d_row.upload(cost_row, (size_t)cells, s); }
        if (top1_cost_out) d_tc1.alloc((size_t)cells);
        hipLaunchKernelGGL(k_weighted_pmf, dim3(nblocks(cells, 4)), dim3(256), 0, s, proba.p, cells, (int)K, (int)top_k, threshold,
                           d_cur.p, d_row.p, d_cost.p, (long long)n_cost_rows, weight, renormalise ? 1 : 0, d_cls.p, d_pr.p, d_cp.p, d_tc1.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rows_out, t->cell_rows.p, (size_t)cells * 8, hipMemcpyDeviceToHost, s));
        d_cls.download(class_out, (size_t)cells * top_k, s);
        d_pr.download(prob_out, (size_t)cells * top_k, s);
        if (cur_prob_out) d_cp.download(cur_prob_out, (size_t)cells, s);
        if (top1_cost_out) d_tc1.download(top1_cost_out, (size_t)cells, s);
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

}  // namespace

extern "C" {

RGBM_EXPORT int rgbm_table_repair_pmf(rgbm_table* t, const rgbm_model* m, int32_t target_col, const int32_t* feat_cols, int32_t f, int32_t top_k,
                                      double threshold, const int32_t* cur_code, int64_t cap, int64_t* n_cells_out, int64_t* rows_out,
                                      int32_t* class_out, double* prob_out, double* cur_prob_out) {
    return repair_pmf(false, t, m, target_col, feat_cols, f, top_k, threshold, cur_code, nullptr, nullptr, 0, 0.0, 0, cap, n_cells_out, rows_out, class_out,
                      prob_out, cur_prob_out, nullptr);
}

RGBM_EXPORT int rgbm_table_repair_pmf_weighted(rgbm_table* t, const rgbm_model* m, int32_t target_col, const int32_t* feat_cols, int32_t f,
                                               int32_t top_k, double threshold, const int32_t* cur_code, const int32_t* cost_row, const double* cost,
                                               int64_t n_cost_rows, double weight, int32_t renormalise, int64_t cap, int64_t* n_cells_out,
                                               int64_t* rows_out, int32_t* class_out, double* prob_out, double* cur_prob_out, double* top1_cost_out) {
    return repair_pmf(true, t, m, target_col, feat_cols, f, top_k, threshold, cur_code, cost_row, cost, n_cost_rows, weight, renormalise, cap, n_cells_out,
                      rows_out, class_out, prob_out, cur_prob_out, top1_cost_out);
}

RGBM_EXPORT int rgbm_edit_distance(int32_t device_id, const int32_t* a_cp, const int64_t* a_off, int64_t n_a, const int32_t* b_cp,
                                   const int64_t* b_off, int64_t n_b, int32_t* dist_out) {
    if (n_a < 0 || n_b < 0 || (n_a > 0 && !a_off) || (n_b > 0 && !b_off) || (n_a > 0 && n_b > 0 && !dist_out))
        return fail(RGBM_ERR_ARG, "rgbm_edit_distance: bad argument");
    return guarded([&]() {
        check_pool_offsets(a_off, n_a, a_cp, "rgbm_edit_distance", "a");
        check_pool_offsets(b_off, n_b, b_cp, "rgbm_edit_distance", "b");
        if (n_a == 0 || n_b == 0) return RGBM_OK;
        use_device(device_id);
        StreamGuard sg;
        DevBuf<int32_t> d_dist((size_t)n_a * n_b);
        edit_distance_on_device(a_cp, a_off, n_a, b_cp, b_off, n_b, d_dist.p, sg.s);
        d_dist.download(dist_out, (size_t)n_a * n_b, sg.s);
        HIPCHK(hipStreamSynchronize(sg.s));
        return RGBM_OK;
    });
}

}  // extern "C"
