// rgbm_domain.hip -- a relational step on the HBM-resident code table (what the steps share is rgbm_prep.h):
// =============================================================================================
// Cell-domain analysis (reference: RepairApi.scala:231-273 computeFreqStats, 479-675 computeDomainInErrorCells; the
// value-space statement is repair/domain.py, which these kernels must equal -- counts exactly, probabilities bit for bit).
//
//   pair_counts    dense joint counts of many column pairs.  The pairs are packed into GROUPS whose 32-bit histograms share one
//                  workgroup's LDS; a workgroup streams its row range once per group, stages the bins of the group's distinct
//                  columns per row tile (each column is loaded once, whatever the number of pairs that use it) and flushes
//                  with 64-bit vector atomics.  A workgroup sees at most 2^30 rows, so no 32-bit counter wraps; all sums
//                  are integers, so the result does not depend on the launch geometry.  Pairs too large for the LDS count
//                  straight into HBM.  Algorithmic bytes: 4 B per (row, distinct column of a group).
//   cell_domains   one error cell per lane: the fixed-order score sums and the divisions of repair/domain.py, nothing else.
// =============================================================================================
#include "rgbm_domain.h"

namespace {

using namespace rgh;

constexpr int PC_B = 512;                                   // threads per workgroup
constexpr int PC_MAXC = 16;                                 // distinct columns a group stages per row tile
constexpr int PC_TILE_BYTES = PC_MAXC * PC_B * 2;           // uint16 bins [PC_MAXC][PC_B]
constexpr int PC_LDS_CELLS = (160 * 1024 - 2048 - PC_TILE_BYTES) / 4;      // 32-bit counters of one group
constexpr long long PC_ROWS_PER_WG_MAX = 1ll << 30;
constexpr long long PC_MAX_CELLS_PAIR = 1ll << 24, PC_MAX_CELLS = 1ll << 25;   // dense cells of one pair / of a call

struct PcPair { int32_t sx, sy, dy1; uint32_t lds_off, cells; long long out_off; };
struct PcGroup { int32_t col_begin, ncols, pair_begin, npairs; uint32_t cells; };

__global__ __launch_bounds__(PC_B) void k_pair_counts(const int32_t* __restrict__ codes, long long n, const PcGroup* __restrict__ groups,
                                                      const int32_t* __restrict__ gcols, const PcPair* __restrict__ pairs,
                                                      const int32_t* __restrict__ colinfo, const long long* __restrict__ lut_off,
                                                      const int32_t* __restrict__ luts, long long rows_per_wg, unsigned tile_off,
                                                      unsigned long long* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* h = reinterpret_cast<unsigned*>(smem);
    unsigned short* tile = reinterpret_cast<unsigned short*>(smem + tile_off);     // [PC_MAXC][PC_B]; a lane reads back its own entries only
    const PcGroup g = groups[blockIdx.y];
    const int tid = threadIdx.x;
    for (unsigned i = tid; i < g.cells; i += PC_B) h[i] = 0;
    __syncthreads();
    const long long begin = (long long)blockIdx.x * rows_per_wg;
    const long long end = begin + rows_per_wg < n ? begin + rows_per_wg : n;
    for (long long base = begin; base < end; base += PC_B) {
        const long long r = base + tid;
        if (r < end) {
            for (int s = 0; s < g.ncols; ++s)
                tile[s * PC_B + tid] = (unsigned short)pc_bin(codes, n, gcols[g.col_begin + s], r, colinfo, lut_off, luts);
            for (int p = 0; p < g.npairs; ++p) {
                const PcPair pp = pairs[g.pair_begin + p];
                atomicAdd(&h[pp.lds_off + (unsigned)tile[pp.sx * PC_B + tid] * (unsigned)pp.dy1 + (unsigned)tile[pp.sy * PC_B + tid]], 1u);
            }
        }
    }
    __syncthreads();
    for (int p = 0; p < g.npairs; ++p) {
        const PcPair pp = pairs[g.pair_begin + p];
        for (unsigned i = tid; i < pp.cells; i += PC_B) {
            const unsigned v = h[pp.lds_off + i];
            if (v) atomicAdd(&out[pp.out_off + i], (unsigned long long)v);
        }
    }
}

// a pair whose dense table does not fit the LDS: one 64-bit atomic per row, straight into HBM
__global__ __launch_bounds__(256) void k_pair_counts_global(const int32_t* __restrict__ codes, long long n, int cx, int cy, int dy1,
                                                            const int32_t* __restrict__ colinfo, const long long* __restrict__ lut_off,
                                                            const int32_t* __restrict__ luts, unsigned long long* __restrict__ out) {
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const long long bx = pc_bin(codes, n, cx, r, colinfo, lut_off, luts), by = pc_bin(codes, n, cy, r, colinfo, lut_off, luts);
        atomicAdd(&out[bx * dy1 + by], 1ull);
    }
}

__global__ __launch_bounds__(256) void k_cell_domains(const int32_t* __restrict__ codes, long long n, int target, int d_a,
                                                      const long long* __restrict__ rows, long long m, const unsigned long long* __restrict__ joint,
                                                      const DomAttr* __restrict__ attrs, int k, const int32_t* __restrict__ colinfo,
                                                      const long long* __restrict__ lut_off, const int32_t* __restrict__ luts,
                                                      const uint8_t* __restrict__ single_ok, double beta, double row_count,
                                                      uint8_t* __restrict__ weak, int32_t* __restrict__ top, double* __restrict__ top_prob,
                                                      double* __restrict__ probs) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const DomCell d = cell_domain(codes, n, target, d_a, rows[i], joint, attrs, k, colinfo, lut_off, luts, single_ok, beta, row_count,
                                  probs ? probs + i * d_a : nullptr);
    weak[i] = (uint8_t)d.weak;
    top[i] = d.top;
    top_prob[i] = d.top_prob;
}

}  // namespace

extern "C" {

// scratch slots held together: TABLE_A (groups) TABLE_B (pairs) COLS (group columns)
RGBM_EXPORT int rgbm_table_pair_counts(rgbm_table* t, const int32_t* pair_cols, int32_t n_pairs, const int32_t* const* luts,
                                       const int32_t* n_bins, int64_t* counts_out) {
    if (!t || !pair_cols || n_pairs <= 0 || !n_bins || !counts_out) return fail(RGBM_ERR_ARG, "rgbm_table_pair_counts: bad argument");
    return guarded([&]() {
        use_device(t->device);
        check_cols(*t, pair_cols, 2 * n_pairs, "rgbm_table_pair_counts");
        const int c = t->c;
        std::vector<long long> off((size_t)n_pairs);
        long long total = 0;
        for (int p = 0; p < n_pairs; ++p) {
            const int x = pair_cols[2 * p], y = pair_cols[2 * p + 1];
            if (x == y) throw std::invalid_argument("rgbm_table_pair_counts: a pair needs two different columns");
            if (n_bins[x] < 1 || n_bins[y] < 1) throw std::invalid_argument("rgbm_table_pair_counts: n_bins must be positive");
            const long long cells = ((long long)n_bins[x] + 1) * ((long long)n_bins[y] + 1);
            if (cells > PC_MAX_CELLS_PAIR) throw std::invalid_argument("rgbm_table_pair_counts: the dense table of a pair holds more than 2^24 cells");
            off[p] = total; total += cells;
            if (total > PC_MAX_CELLS) throw std::invalid_argument("rgbm_table_pair_counts: the dense tables hold more than 2^25 cells");
        }
        // per column: {n_codes, n_bins}, LUT offset (-1 = the codes are the bins)
        std::vector<int32_t> colinfo((size_t)c * 2), flat; std::vector<long long> loff((size_t)c, -1); std::vector<uint8_t> has_lut((size_t)c, 0);
        for (int j = 0; j < c; ++j) {
            colinfo[2 * j] = t->n_codes[j]; colinfo[2 * j + 1] = std::max(n_bins[j], 1);
            if (luts && luts[j]) { loff[j] = (long long)flat.size(); flat.insert(flat.end(), luts[j], luts[j] + t->n_codes[j]); has_lut[j] = 1; }
        }
        // groups: pairs in the given order; a group is closed when its histograms or its distinct columns would not fit
        std::vector<PcGroup> groups; std::vector<PcPair> pairs; std::vector<int32_t> gcols; std::vector<int> global_pairs;
        std::vector<int32_t> plan((size_t)n_pairs * 3, -1);       // per pair {group (-1 = the HBM kernel), slot of x, slot of y}: the report
        long long plan_head[4] = {0, 0, 0, 0};                    // {groups, cells of the largest group, grid x, rows per workgroup}
        PcGroup cur{0, 0, 0, 0, 0};
        auto slot_of = [&](int col) { for (int s = 0; s < cur.ncols; ++s) if (gcols[cur.col_begin + s] == col) return s; return -1; };
        for (int p = 0; p < n_pairs; ++p) {
            const int x = pair_cols[2 * p], y = pair_cols[2 * p + 1];
            const long long cells = ((long long)n_bins[x] + 1) * ((long long)n_bins[y] + 1);
            if (cells > PC_LDS_CELLS) { global_pairs.push_back(p); continue; }
            int need = (slot_of(x) < 0) + (slot_of(y) < 0);
            if (cur.npairs > 0 && (cur.cells + cells > (long long)PC_LDS_CELLS || cur.ncols + need > PC_MAXC)) {
                groups.push_back(cur);
                cur = PcGroup{(int32_t)gcols.size(), 0, (int32_t)pairs.size(), 0, 0};
            }
            if (slot_of(x) < 0) { gcols.push_back(x); ++cur.ncols; }
            if (slot_of(y) < 0) { gcols.push_back(y); ++cur.ncols; }
            pairs.push_back(PcPair{slot_of(x), slot_of(y), n_bins[y] + 1, cur.cells, (uint32_t)cells, off[p]});
            plan[3 * (size_t)p] = (int32_t)groups.size(); plan[3 * (size_t)p + 1] = pairs.back().sx; plan[3 * (size_t)p + 2] = pairs.back().sy;
            cur.cells += (uint32_t)cells; ++cur.npairs;
        }
        if (cur.npairs > 0) groups.push_back(cur);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const long long n = t->n;
        t->pc_counts.alloc((size_t)total); t->pc_counts.zero(s);
        t->pc_bins.alloc(colinfo.size()); t->pc_bins.upload(colinfo.data(), colinfo.size(), s);
        t->pc_lut_off.alloc(loff.size()); t->pc_lut_off.upload(loff.data(), loff.size(), s);
        t->pc_luts.alloc(std::max<size_t>(flat.size(), 1)); t->pc_luts.upload(flat.data(), flat.size(), s);
        if (!groups.empty()) {
            const PcGroup* d_groups = scr_upload<PcGroup>(*t, SCR_TABLE_A, groups.data(), groups.size(), s);
            const PcPair* d_pairs = scr_upload<PcPair>(*t, SCR_TABLE_B, pairs.data(), pairs.size(), s);
            const int32_t* d_gcols = scr_upload<int32_t>(*t, SCR_COLS, gcols.data(), gcols.size(), s);
            unsigned max_cells = 0;
            for (const PcGroup& g : groups) max_cells = std::max(max_cells, g.cells);
            const unsigned tile_off = (max_cells * 4u + 15u) & ~15u;
            const size_t lds = (size_t)tile_off + PC_TILE_BYTES;
            // enough workgroups to fill the device a few times over; a workgroup never sees more than 2^30 rows
            long long chunks = std::min<long long>((n + 16 * PC_B - 1) / (16 * PC_B), std::max<long long>(1, 2048 / (long long)groups.size()));
            chunks = std::max<long long>(chunks, (n + PC_ROWS_PER_WG_MAX - 1) / PC_ROWS_PER_WG_MAX);
            chunks = std::max<long long>(chunks, 1);
            long long rows_per_wg = (n + chunks - 1) / chunks;
            rows_per_wg = (rows_per_wg + PC_B - 1) / PC_B * PC_B;
            plan_head[0] = (long long)groups.size(); plan_head[1] = max_cells; plan_head[2] = (n + rows_per_wg - 1) / rows_per_wg; plan_head[3] = rows_per_wg;
            if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_pair_counts, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_pair_counts, dim3((unsigned)((n + rows_per_wg - 1) / rows_per_wg), (unsigned)groups.size()), dim3(PC_B), lds, s,
                               t->codes.p, n, d_groups, d_gcols, d_pairs, t->pc_bins.p, t->pc_lut_off.p, t->pc_luts.p, rows_per_wg, tile_off,
                               t->pc_counts.p);
            HIPCHK(hipGetLastError());
        }
        for (int p : global_pairs) {
            const int x = pair_cols[2 * p], y = pair_cols[2 * p + 1];
            const unsigned nb = std::max(1u, std::min<unsigned>(nblocks(n, 256 * 8), 256u * 16u));
            hipLaunchKernelGGL(k_pair_counts_global, dim3(nb), dim3(256), 0, s, t->codes.p, n, x, y, n_bins[y] + 1, t->pc_bins.p, t->pc_lut_off.p,
                               t->pc_luts.p, t->pc_counts.p + off[p]);
            HIPCHK(hipGetLastError());
        }
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are 64-bit");
        HIPCHK(hipMemcpyAsync(counts_out, t->pc_counts.p, (size_t)total * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        t->pc_x.resize(n_pairs); t->pc_y.resize(n_pairs); t->pc_dx.resize(n_pairs); t->pc_dy.resize(n_pairs); t->pc_off = off;
        for (int p = 0; p < n_pairs; ++p) {
            t->pc_x[p] = pair_cols[2 * p]; t->pc_y[p] = pair_cols[2 * p + 1]; t->pc_dx[p] = n_bins[t->pc_x[p]]; t->pc_dy[p] = n_bins[t->pc_y[p]];
        }
        t->pc_nbins.assign((size_t)c, 0);
        for (int j = 0; j < c; ++j) t->pc_nbins[j] = colinfo[2 * j + 1];
        t->pc_has_lut = has_lut;
        t->pc_plan = plan; std::copy(plan_head, plan_head + 4, t->pc_plan_head);
        return RGBM_OK;
    });
}

// no device work: the plan the last successful rgbm_table_pair_counts call on the table took, and the two limits its planner works to
RGBM_EXPORT int rgbm_table_pair_counts_report(const rgbm_table* t, int64_t* head_out, int32_t* pairs_out, int32_t n_pairs) {
    if (!head_out || n_pairs < 0 || (n_pairs > 0 && (!t || !pairs_out))) return fail(RGBM_ERR_ARG, "rgbm_table_pair_counts_report: bad argument");
    for (int i = 0; i < 4; ++i) head_out[i] = 0;
    head_out[4] = PC_LDS_CELLS; head_out[5] = PC_MAXC;
    if (!t) return RGBM_OK;
    std::lock_guard<std::mutex> prep_lk(t->prep_mu);
    if ((size_t)n_pairs * 3 != t->pc_plan.size())
        return fail(RGBM_ERR_ARG, "rgbm_table_pair_counts_report: n_pairs is not the number of pairs of the table's last rgbm_table_pair_counts call");
    for (int i = 0; i < 4; ++i) head_out[i] = t->pc_plan_head[i];
    std::copy(t->pc_plan.begin(), t->pc_plan.end(), pairs_out);
    return RGBM_OK;
}

// scratch slots held together: TABLE_A (attributes) COLS (single_ok) IN_ROWS ROW_MASK (weak) IN_COLS (top) VALS (top_prob)
RGBM_EXPORT int rgbm_table_cell_domains(rgbm_table* t, int32_t target_col, const int64_t* rows, int64_t n_cells, const int32_t* pair_idx, int32_t k,
                                        const int64_t* min_cnt, const uint8_t* single_ok, double beta, int64_t row_count, uint8_t* weak_out,
                                        int32_t* top_out, double* top_prob_out, double* probs_out) {
    if (!t || target_col < 0 || target_col >= t->c || n_cells < 0 || (n_cells > 0 && (!rows || !weak_out || !top_out || !top_prob_out)) || k < 0 ||
        (k > 0 && (!pair_idx || !min_cnt)) || !single_ok || row_count <= 0)
        return fail(RGBM_ERR_ARG, "rgbm_table_cell_domains: bad argument");
    return guarded([&]() {
        use_device(t->device);
        if (k > DOM_MAXK) throw std::invalid_argument("rgbm_table_cell_domains: more than 8 correlated attributes");
        if (t->pc_nbins.empty()) throw std::invalid_argument("rgbm_table_cell_domains: no rgbm_table_pair_counts result on this table");
        if (t->pc_has_lut[target_col]) throw std::invalid_argument("rgbm_table_cell_domains: the target must be a discrete attribute (no LUT)");
        if (n_cells == 0) return RGBM_OK;
        const int d_a = t->pc_nbins[target_col];
        const std::vector<DomAttr> attrs = dom_attrs(*t, target_col, pair_idx, k, min_cnt, "rgbm_table_cell_domains");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const DomAttr* d_attrs = scr_upload<DomAttr>(*t, SCR_TABLE_A, attrs.data(), attrs.size(), s);
        const uint8_t* d_ok = scr_upload<uint8_t>(*t, SCR_COLS, single_ok, (size_t)d_a, s);
        const long long* d_rows = scr_upload<long long>(*t, SCR_IN_ROWS, reinterpret_cast<const long long*>(rows), (size_t)n_cells, s);
        uint8_t* d_weak = scr<uint8_t>(*t, SCR_ROW_MASK, (size_t)n_cells);
        int32_t* d_top = scr<int32_t>(*t, SCR_IN_COLS, (size_t)n_cells);
        double* d_tp = scr<double>(*t, SCR_VALS, (size_t)n_cells);
        DevBuf<double> d_probs;
        if (probs_out) d_probs.alloc((size_t)n_cells * d_a);
        hipLaunchKernelGGL(k_cell_domains, dim3(nblocks(n_cells, 256)), dim3(256), 0, s, t->codes.p, (long long)t->n, (int)target_col, d_a, d_rows,
                           (long long)n_cells, t->pc_counts.p, d_attrs, (int)k, t->pc_bins.p, t->pc_lut_off.p, t->pc_luts.p, d_ok, beta,
                           (double)row_count, d_weak, d_top, d_tp, d_probs.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(weak_out, d_weak, (size_t)n_cells, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(top_out, d_top, (size_t)n_cells * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(top_prob_out, d_tp, (size_t)n_cells * 8, hipMemcpyDeviceToHost, s));
        if (probs_out) d_probs.download(probs_out, (size_t)n_cells * d_a, s);
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

}  // extern "C"
