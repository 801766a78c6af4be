// rgbm.hip -- librepairgbm.so: host orchestration + C-ABI (include/rgbm.h) over the gfx950 kernels.
//
// One training call = one HIP stream; the whole leaf-wise growth of the K class trees of a
// boosting iteration runs on the device in lock step (grid.y = class tree) without any host
// round trip: the per-tree control blocks (rg::TreeState) live in HBM and every kernel of the
// fixed launch sequence
//     hist -> split_find -> tree_step -> partition -> finish_split     (num_leaves-1 times)
// reads its work description from there.  The host only enqueues.
//
// Host side of a fit, in the order of this file: the pieces both trainers share (check_fit_args, BinRecords with
// the code counts, BagState, TreeBlock), then train_core = prologue -> FitState (what both growers work on) -> LevelGrower or
// LeafwiseGrower (each owns its buffers) -> the boosting loop and the harvest, then train_batch_small on the same set-up pieces.
//
// There is NO CPU fallback in this library: without a HIP device every compute entry point
// returns RGBM_ERR_NO_DEVICE (the CPU oracle under oracle/ is test infrastructure and is never
// linked or loaded from here).
//
// The device-memory pool, the error text and the page-locked upload live in rgbm_runtime.hip, the communicator in rgbm_comm.hip; this file
// holds the trainer, the batched trainer, the predictor, model I/O and the chained repair.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <stdexcept>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "rgbm_host.h"
#include "rgbm_kernels.h"
#include "rgbm_level.h"
#include "rgbm_small.h"


namespace {
using rgh::fail; using rgh::DevBuf; using rgh::use_device; using rgh::StreamGuard; using rgh::guarded;
using rgh::AR_I64; using rgh::AR_U32; using rgh::AR_I32; using rgh::all_reduce; using rgh::all_gather_on; using rgh::stream_sync_watchdog; using rgh::comm_abort;
using rgh::comm_kind; using rgh::comm_rank; using rgh::comm_nranks; using rgh::upload_pinned;

struct Feat {
    int32_t n_codes = 0, V = 0, has_nan = 0; std::vector<int32_t> ub;
    // CATEGORICAL features only (else empty): bit c set => no training row held code c.  Such a category is MISSING for this model at
    // prediction time (it has no place in the order of the codes) -- what a per-model dictionary does with a value it does not hold.
    std::vector<uint32_t> unseen;
    bool is_unseen(int32_t c) const { return !unseen.empty() && ((unseen[(size_t)c >> 5] >> (c & 31)) & 1u); }
};
// One tree: L leaves, L - 1 internal nodes.  Its eight arrays sit in ONE block -- the tree's own, or a slice of the model's arena
// (a model is 300 x K trees: eight std::vectors a tree were 576 000 allocations for the 16 models of a default job).
struct Tree {
    int32_t L = 1;
    double *gain = nullptr, *leaf_value = nullptr;
    int32_t *feat = nullptr, *theta = nullptr, *dleft = nullptr, *left = nullptr, *right = nullptr, *leaf_count = nullptr;
    std::unique_ptr<double[]> own;
    static size_t doubles(int L) { const size_t n = (size_t)L - 1; return n + (size_t)L + (5 * n + (size_t)L + 1) / 2; }
    void place(double* p, int L_) {
        L = L_; const size_t n = (size_t)L - 1;
        gain = p; leaf_value = p + n;
        int32_t* q = reinterpret_cast<int32_t*>(p + n + L);
        feat = q; theta = q + n; dleft = q + 2 * n; left = q + 3 * n; right = q + 4 * n; leaf_count = q + 5 * n;
    }
    void alloc(int L_) { own.reset(new double[doubles(L_)]); place(own.get(), L_); }
};

struct DeviceModel {   // predictor mirror of a model on one device
    DevBuf<rg::PNode> nodes; DevBuf<double> leaf_value;
    // bit-vector scoring tables (k_predict_qs): per tree the AND-masks of every (feature, bin) and the leaf values in left-to-right order
    DevBuf<uint32_t> qs_masks, qs_used; DevBuf<double> qs_leaves; DevBuf<int32_t> qs_foff; int qs_S = 0, qs_MW = 0;   // qs_MW = 0: not built
    DevBuf<uint8_t> lut; DevBuf<long long> lut_off; DevBuf<int32_t> n_codes; DevBuf<uint8_t> miss; DevBuf<int32_t> ident;
    int node_stride = 1, leaf_stride = 1;
};

}  // namespace

struct rgbm_model {
    int32_t objective = 0, num_class = 0, K = 1, n_iter = 0, F = 0;
    std::vector<Feat> feats;
    std::vector<Tree> trees;
    std::unique_ptr<double[]> tree_arena;      // storage of the trees of a trained model (a loaded model's trees own theirs)
    std::mutex mu;
    std::map<int, DeviceModel*> dev;
    ~rgbm_model() { for (auto& kv : dev) { (void)hipSetDevice(kv.first); delete kv.second; } }
};


namespace {

// ---------------------------------------------------------------------------------------------
// Host logic: bin finding (LightGBM bin.cpp GreedyFindBin / FindBinWithZeroAsOneBin restated in
// code space; see DESIGN.md "Binning").  Input: counts per code over the training rows.
// ---------------------------------------------------------------------------------------------
// Bin upper bound between two neighbouring training codes a < b.  Codes of a NUMERIC column are ranks of its distinct values and
// LightGBM puts the bound at the midpoint of the VALUES: with the column's value dictionary (rgbm_table_set_column_values) the bound
// in code space is the largest code whose value is <= (val[a] + val[b]) / 2, so a value that only rows outside the training set
// hold falls on the side LightGBM would send it to.  Without one (categorical columns, host-array calls) the codes are the scale.
int32_t mid_code(int32_t a, int32_t b, const double* vals) {
    if (!vals) return (int32_t)(((int64_t)a + (int64_t)b) / 2);
    const double m = (vals[a] + vals[b]) / 2.0;
    int32_t lo = a, hi = b - 1;
    while (lo < hi) { const int32_t c = lo + (hi - lo + 1) / 2; if (vals[c] <= m) lo = c; else hi = c - 1; }
    return lo;
}

int greedy_find_bin(const std::vector<int32_t>& dv, const std::vector<int64_t>& cnt, int max_bin, int64_t total_cnt,
                    int min_data_in_bin, std::vector<int32_t>& ub, const double* vals) {
    const int nd = (int)dv.size();
    ub.clear();
    if (nd <= 0) return 0;
    if (nd <= max_bin) {
        int64_t cur = 0;
        for (int i = 0; i + 1 < nd; ++i) {
            cur += cnt[i];
            if (cur >= min_data_in_bin) { ub.push_back(mid_code(dv[i], dv[i + 1], vals)); cur = 0; }
        }
        ub.push_back(INT32_MAX);
        return (int)ub.size();
    }
    if (min_data_in_bin > 0) {
        max_bin = (int)std::min<int64_t>(max_bin, total_cnt / min_data_in_bin);
        max_bin = std::max(max_bin, 1);
    }
    double mean_bin_size = (double)total_cnt / max_bin;
    int rest_bin_cnt = max_bin;
    int64_t rest_sample_cnt = total_cnt;
    std::vector<char> big(nd, 0);
    for (int i = 0; i < nd; ++i)
        if ((double)cnt[i] >= mean_bin_size) { big[i] = 1; --rest_bin_cnt; rest_sample_cnt -= cnt[i]; }
    mean_bin_size = (double)rest_sample_cnt / rest_bin_cnt;
    std::vector<int32_t> upper(max_bin, INT32_MAX), lower(max_bin, INT32_MAX);
    int bin_cnt = 0;
    lower[0] = dv[0];
    int64_t cur = 0;
    for (int i = 0; i + 1 < nd; ++i) {
        if (!big[i]) rest_sample_cnt -= cnt[i];
        cur += cnt[i];
        double half = mean_bin_size * 0.5f;
        if (half < 1.0) half = 1.0;
        if (big[i] || (double)cur >= mean_bin_size || (big[i + 1] && (double)cur >= half)) {
            upper[bin_cnt] = dv[i];
            ++bin_cnt;
            lower[bin_cnt] = dv[i + 1];
            if (bin_cnt >= max_bin - 1) break;
            cur = 0;
            if (!big[i]) { --rest_bin_cnt; mean_bin_size = (double)rest_sample_cnt / (double)rest_bin_cnt; }
        }
    }
    ++bin_cnt;
    for (int i = 0; i + 1 < bin_cnt; ++i) {
        int32_t v = mid_code(upper[i], lower[i + 1], vals);
        if (ub.empty() || ub.back() != v) ub.push_back(v);
    }
    ub.push_back(INT32_MAX);
    return (int)ub.size();
}

void find_bin(const unsigned int* cnt, int32_t n_codes, int64_t n_train, const rgbm_params& p, Feat& f, const double* vals) {
    std::vector<int32_t> dv; std::vector<int64_t> dc;
    int64_t seen = 0;
    for (int32_t c = 0; c < n_codes; ++c) if (cnt[c]) { dv.push_back(c); dc.push_back(cnt[c]); seen += cnt[c]; }
    const int64_t na = n_train - seen;
    int mb = p.max_bin - (na > 0 ? 1 : 0) - 1;   // NaN bin, zero bin (FindBinWithZeroAsOneBin)
    if (mb < 1) mb = 1;
    f.n_codes = n_codes; f.has_nan = na > 0 ? 1 : 0;
    f.V = greedy_find_bin(dv, dc, mb, seen, p.min_data_in_bin, f.ub, vals);
}


// Test / experiment switches, read from the environment at the start of every training call (tests flip them between calls); none
// is needed in normal use.  Next to the fields below: RGBM_TRACE / RGBM_TRACE_K / RGBM_TRACE_ITERS (LevelTrace) and RGBM_TEST_HOOKS=1 +
// RGBM_FX_ROWS=R (fit_setup).
// Retired with their code paths; DESIGN.md ("Retired experiments") names the switches, and the parent of the commit that removed them is the
// last one where they can be rebuilt (the measurements stay in profiles/EXPERIMENTS.md):
//   lock-step of the class-tree groups of a row block                  -63 % HBM fetch, +23 % time
//   score update inside the next iteration's gradient kernel           bench step 80.8 -> 83.1 ms, the third fusion of the two that lost
//   16-bit joint codes in the root pass                                neutral
//   768-thread plain one-chunk level pass                              84.4 ms against 80.8
//   wave-specialised pass as a switch                                  one chunk: 3 % slower; two chunks: the measured default, now the only form
//   partial-T rotation (two switches)                                  81.8 -> 86.1 -> 89.6 ms
//   compile-time: rotate every level pass / 64-entry rings             loses 35-60 % at levels 1-4 / neutral
// The distinct-row view (rgbm_table_train): a table is trained through its distinct rows when they are at most
// DISTINCT_MAX_RATIO of its rows (the policy default of model.train.distinct_rows.max_ratio) and it has at least DISTINCT_MIN_ROWS rows.
// The floor is measured (profiles/EXPERIMENTS.md, "distinct-row view"): a K = 24 fit of 20 iterations on a fresh table with M = N / 4, view build
// included, parent library / this one alternating, three runs each, ms:   N = 2^18  23.8-25.4 / 23.7-29.3 (a fit that small is the latency of its
// chain of kernels);   2^20  39.8-41.5 / 28.2-31.0;   2^22  96.9-98.0 / 42.7-43.3.  2^20 is the smallest of the three N at which the slowest run
// with the view is below the fastest without.  M = N / 2 at N = 2^20: 39.0-40.2 / 33.6-34.0, so the 0.5 ratio is still ahead.
constexpr double DISTINCT_MAX_RATIO = 0.5;
constexpr long long DISTINCT_MIN_ROWS = 1ll << 20;
struct RunSwitches {
    int grower = 0;                // RGBM_GROWER=level|leafwise (1 | 2): 0 picks the level grower wherever it applies; both give the same models
    bool timing = false;           // RGBM_TIMING: host wall-clock of the phases and the launch plan, to stderr
    int lv_lds = 0;                // RGBM_LV_LDS=bytes: a smaller LDS pool for the level passes (tests: several built-slot windows per level)
    long long lv_blocks = 0;       // RGBM_LV_BLOCKS: row blocks per class tree of the root pass (0: planned)
    long long mt_blocks = 0;       // RGBM_MT_BLOCKS: row blocks per class tree of the level passes (0: planned)
    int mt_T = 0;                  // RGBM_MT_TREES: cap on the class trees per level-pass workgroup (0: none)
    int mt_rep = 8;                // RGBM_MT_REP: LDS copies of every bin the level passes are sized for
    bool joint_root = true;        // RGBM_JOINT_ROOT=0: root pass over the plain records instead of the joint-bin record
    bool mt_acc2 = true;           // RGBM_MT_ACC2=0: tables of 17..32 features take one level pass per 16-feature chunk instead of one that
                                   // accumulates both (the per-chunk form is what > 32 features and histograms too large for the LDS get)
    bool mt_sparse = true;         // RGBM_MT_SPARSE=0: class trees with < 1/MT_SPARSE_DIV live rows are walked tile by tile like the others
    int mt_rot = -1;               // RGBM_MT_ROT: feature rotation of a level pass's atomics: -1 per launch (the rule below), 0 never, 1 wherever the form exists
    int mt_rot_copies2 = 16;       // RGBM_MT_ROT_COPIES2: a launch rotates when the LDS holds fewer than this / 2 (eight) copies of its worst-case
                                   // histograms, the eight the replicated layout is sized for (profiles/r6r_*)
    int mt_rot_tmin = 2;           // RGBM_MT_ROT_TMIN: ... or when replication leaves the workgroup fewer class trees than this although one copy
                                   // holds twice as many (0 = off).  0 / 2 / 4: bench step 80.4-80.8 / 80.0-80.1 / 80.8-81.2 ms (profiles/EXPERIMENTS.md, r7m / r7n)
    bool step_readback = false;    // RGBM_STEP_READBACK=1: k_level_step scans the child histograms out of the pool, not out of LDS (tests: the path of wide tables)
    int step_threads = 0;          // RGBM_STEP_THREADS: workgroup size of k_level_step (0: LevelGrower's choice)
    int step_max_gx = 0;           // RGBM_STEP_MAX_GX: most workgroup partials per class tree k_level_step sums itself (0: LevelGrower's choice)
    bool fx_separate = false;      // RGBM_FX_MEASURE=separate: the coarse gradient sums of numerics v2.2 from a pass of their own (k_fx_measure, the
                                   // live path for K > 112) instead of out of the gradient kernels; same sums, same models
    bool distinct = true;          // RGBM_DISTINCT=0: rgbm_table_train never trains on the table's distinct-row view (the row-for-row figures)
    double distinct_max_ratio = DISTINCT_MAX_RATIO;      // RGBM_DISTINCT_MAX_RATIO
    long long distinct_min_rows = DISTINCT_MIN_ROWS;     // RGBM_DISTINCT_MIN_ROWS
};
RunSwitches read_switches() {
    RunSwitches w;
    if (const char* e = getenv("RGBM_GROWER")) w.grower = strcmp(e, "leafwise") == 0 ? 2 : (strcmp(e, "level") == 0 ? 1 : 0);
    if (const char* e = getenv("RGBM_LV_LDS")) w.lv_lds = atoi(e);
    if (const char* e = getenv("RGBM_LV_BLOCKS")) w.lv_blocks = atoll(e);
    if (const char* e = getenv("RGBM_MT_BLOCKS")) w.mt_blocks = atoll(e);
    if (const char* e = getenv("RGBM_MT_TREES")) w.mt_T = atoi(e);
    if (const char* e = getenv("RGBM_MT_REP")) w.mt_rep = atoi(e);
    if (const char* e = getenv("RGBM_JOINT_ROOT")) w.joint_root = atoi(e) != 0;
    if (const char* e = getenv("RGBM_MT_ACC2")) w.mt_acc2 = atoi(e) != 0;
    if (const char* e = getenv("RGBM_MT_SPARSE")) w.mt_sparse = atoi(e) != 0;
    if (const char* e = getenv("RGBM_STEP_READBACK")) w.step_readback = atoi(e) != 0;
    if (const char* e = getenv("RGBM_STEP_THREADS")) w.step_threads = atoi(e);
    if (const char* e = getenv("RGBM_STEP_MAX_GX")) w.step_max_gx = atoi(e);
    if (const char* e = getenv("RGBM_FX_MEASURE")) w.fx_separate = strcmp(e, "separate") == 0;
    if (const char* e = getenv("RGBM_MT_ROT")) w.mt_rot = atoi(e);
    if (const char* e = getenv("RGBM_MT_ROT_COPIES2")) w.mt_rot_copies2 = atoi(e);
    if (const char* e = getenv("RGBM_MT_ROT_TMIN")) w.mt_rot_tmin = atoi(e);
    if (const char* e = getenv("RGBM_DISTINCT")) w.distinct = atoi(e) != 0;
    if (const char* e = getenv("RGBM_DISTINCT_MAX_RATIO")) { const double r = atof(e); if (r >= 0.0 && r <= 1.0) w.distinct_max_ratio = r; }
    if (const char* e = getenv("RGBM_DISTINCT_MIN_ROWS")) w.distinct_min_rows = std::max(1ll, atoll(e));
    w.timing = getenv("RGBM_TIMING") != nullptr;
    return w;
}

// LightGBM utils/random.h (as remembered)
struct LgbRand {
    uint32_t x;
    explicit LgbRand(uint32_t seed) : x(seed) {}
    int rnd16() { x = 214013u * x + 2531011u; return (int)((x >> 16) & 0x7FFF); }
    int rnd32() { x = 214013u * x + 2531011u; return (int)(x & 0x7FFFFFFF); }
    float next_float() { return (float)rnd16() / 32768.0f; }
    int next_int(int lo, int hi) { return rnd32() % (hi - lo) + lo; }
    std::vector<int> sample(int N, int K) {
        std::vector<int> ret;
        if (K > N || K <= 0) return ret;
        if (K == N) { for (int i = 0; i < N; ++i) ret.push_back(i); return ret; }
        if (K > 1 && (double)K > ((double)N / std::log2((double)K))) {
            for (int i = 0; i < N; ++i) {
                double prob = (double)(K - (int)ret.size()) / (double)(N - i);
                if (next_float() < prob) ret.push_back(i);
            }
            return ret;
        }
        std::vector<char> in(N, 0);
        for (int r = N - K; r < N; ++r) { int v = next_int(0, r); if (in[v]) in[r] = 1; else in[v] = 1; }
        for (int i = 0; i < N; ++i) if (in[i]) ret.push_back(i);
        return ret;
    }
};


void check_params(const rgbm_params& p) {
    if (p.objective < 0 || p.objective > 2) throw std::invalid_argument("objective must be 0 (binary), 1 (multiclass) or 2 (regression)");
    if (p.max_bin < 2 || p.max_bin > 255) throw std::invalid_argument("max_bin must be in [2, 255]");
    if (p.num_leaves < 2 || p.num_leaves > 32767) throw std::invalid_argument("num_leaves must be in [2, 32767]");
    if (p.n_estimators < 1) throw std::invalid_argument("n_estimators must be positive");
    if (!(p.learning_rate > 0.0)) throw std::invalid_argument("learning_rate must be positive");
    // regression: the fixed-point grid of the histogram sums is sized for |score - y| <= (max y - min y), which a shrinkage above 1 can break
    if (p.objective == 2 && p.learning_rate > 1.0) throw std::invalid_argument("regression with learning_rate > 1 is not supported");
    if (p.objective == 1 && p.num_class < 2) throw std::invalid_argument("multiclass needs num_class >= 2");
    if (p.min_data_in_leaf < 0 || p.lambda_l1 < 0 || p.lambda_l2 < 0) throw std::invalid_argument("negative regularisation / min_data_in_leaf");
    if (p.bagging_fraction <= 0.0 || p.bagging_fraction > 1.0) throw std::invalid_argument("bagging_fraction must be in (0, 1]");
    if (p.feature_fraction <= 0.0 || p.feature_fraction > 1.0) throw std::invalid_argument("feature_fraction must be in (0, 1]");
}

struct HostLabelStats {   // row-order weight sums, only used with per-row sample weights
    bool valid = false;
    std::vector<double> tot; double suml = 0.0, w_max = 0.0;
};

// ---------------------------------------------------------------------------------------------
// What a fit derives from the code counts of its training rows before it touches row data (GBDT::Init / Dataset construction /
// BoostFromScore): bins, lookup tables, chunk layout, label statistics, initial scores, the fixed-point grid.  Shared by the
// single-fit trainer (train_core) and the batched small-table trainer (train_batch_small).
// ---------------------------------------------------------------------------------------------
struct FitHost {
    int64_t n_train = 0; int nchunk = 1; size_t lds_hist = 0;
    std::vector<int32_t> cols, ncod; std::vector<long long> cnt_off, lut_off; std::vector<unsigned int> cnt;
    std::vector<rg::FeatMeta> fmeta; std::vector<rg::ChunkMeta> cmeta; std::vector<uint8_t> lut, miss, trivial;
    std::vector<double> init, yv32; rg::TrainConst tc;
    std::unique_ptr<rgbm_model> model;
};

void fit_setup(const rgbm_table& tab, const double* y_value_in, const double* class_weight, const HostLabelStats* hls, const rgbm_params& p, int32_t F, FitHost& h) {
    using namespace rg;
    const int64_t N = tab.n;
    const int obj = p.objective;
    const std::vector<int32_t>& cols = h.cols; const std::vector<int32_t>& ncod = h.ncod; const std::vector<long long>& cnt_off = h.cnt_off;
    const std::vector<unsigned int>& cnt = h.cnt;
    const int n_y = ncod[F];
    const int K = obj == 1 ? p.num_class : 1;
    const double* y_value = nullptr;
    if (obj == 2) { h.yv32.resize(std::max(n_y, 1)); for (int c = 0; c < n_y; ++c) h.yv32[c] = (double)(float)y_value_in[c]; y_value = h.yv32.data(); }
    const unsigned int* ycnt = cnt.data() + cnt_off[F];
    int64_t& n_train = h.n_train; n_train = 0;
    for (int c = 0; c < n_y; ++c) n_train += ycnt[c];
    if (n_train <= 0) throw std::out_of_range("no training rows (every target cell is NULL)");
    if (N >= (1ll << 31) - 4096) throw std::invalid_argument("more than 2^31 rows per table are not supported");

    // ---- 2. bins
    h.model.reset(new rgbm_model());
    rgbm_model* model = h.model.get();
    model->objective = obj; model->num_class = obj == 1 ? K : (obj == 0 ? 2 : 1); model->K = K; model->F = F;
    model->feats.resize(F);
    std::vector<FeatMeta>& fmeta = h.fmeta; fmeta.assign(F, FeatMeta());
    std::vector<long long>& lut_off = h.lut_off; lut_off.assign(F + 1, 0);
    std::vector<uint8_t>& miss = h.miss; std::vector<uint8_t>& trivial = h.trivial; miss.assign(F, 0); trivial.assign(F, 0);
    int totbins = 0;
    for (int f = 0; f < F; ++f) {
        Feat& ft = model->feats[f];
        const std::vector<double>* cv = (size_t)cols[f] < tab.col_values.size() ? &tab.col_values[cols[f]] : nullptr;
        find_bin(cnt.data() + cnt_off[f], ncod[f], n_train, p, ft, (cv && (int32_t)cv->size() == ncod[f] && ncod[f] > 0) ? cv->data() : nullptr);
        if ((size_t)cols[f] < tab.col_kind.size() && tab.col_kind[cols[f]] == 1) {
            const unsigned int* cf = cnt.data() + cnt_off[f];
            bool any = false;
            for (int32_t c = 0; c < ncod[f]; ++c) any |= cf[c] == 0;
            if (any) {
                ft.unseen.assign((size_t)(ncod[f] + 31) / 32, 0u);
                for (int32_t c = 0; c < ncod[f]; ++c) if (cf[c] == 0) ft.unseen[(size_t)c >> 5] |= 1u << (c & 31);
            }
        }
        fmeta[f].V = ft.V; fmeta[f].has_nan = ft.has_nan; fmeta[f].nbins = std::max(ft.V + ft.has_nan, 1); fmeta[f].hoff = totbins;
        totbins += fmeta[f].nbins;
        trivial[f] = (ft.V + ft.has_nan <= 1) || ft.V == 0;
        miss[f] = (uint8_t)(ft.has_nan ? ft.V : 0);
        lut_off[f + 1] = lut_off[f] + std::max(ncod[f], 1);
    }
    std::vector<uint8_t>& lut = h.lut; lut.assign(lut_off[F], 0);
    for (int f = 0; f < F; ++f) {
        const Feat& ft = model->feats[f];
        int b = 0;
        for (int c = 0; c < ncod[f]; ++c) { while (b < ft.V - 1 && c > ft.ub[b]) ++b; lut[lut_off[f] + c] = (uint8_t)(ft.V > 0 ? b : 0); }
    }
    const int nchunk = (F + 15) / 16; h.nchunk = nchunk;
    std::vector<ChunkMeta>& cmeta = h.cmeta; cmeta.assign(nchunk, ChunkMeta());
    size_t& lds_hist = h.lds_hist; lds_hist = 0;
    for (int ch = 0; ch < nchunk; ++ch) {
        ChunkMeta& cm = cmeta[ch]; cm.first_feat = ch * 16; cm.nfeat = std::min(16, F - ch * 16); cm.fast_slots = 0; cm.wide_bins = 0;
        for (int j = 0; j < cm.nfeat; ++j) {
            FeatMeta& m = fmeta[ch * 16 + j];
            int sh = 0; while (sh < 5 && (m.nbins << (sh + 1)) <= 256) ++sh;
            m.rep_shift = sh; m.fast_base = cm.fast_slots; m.wide_off = cm.wide_bins;
            cm.fast_slots += m.nbins << sh; cm.wide_bins += m.nbins;
        }
        lds_hist = std::max(lds_hist, (size_t)cm.fast_slots * 16);      // leaf-wise k_hist: replicated (g, h) slots, 16 B each
    }

    // ---- 3. label statistics, init scores (BoostFromScore), quantisation scales
    const int nl = std::max({n_y, obj == 0 ? 2 : 1, obj == 1 ? K : 1});
    std::vector<double> tot(nl, 0.0);
    double w_max = 0.0;
    if (hls && hls->valid) { tot = hls->tot; tot.resize(nl, 0.0); w_max = hls->w_max; }
    else {
        for (int c = 0; c < n_y; ++c) {
            const double cw32 = class_weight ? (double)(float)class_weight[c] : 1.0;   // float32 weights (LightGBM label_t)
            tot[c] = (double)ycnt[c] * cw32;
            if (ycnt[c]) w_max = std::max(w_max, cw32);
        }
    }
    if (!(w_max > 0.0)) w_max = 1.0;
    double sumw = 0.0;
    for (int c = 0; c < nl; ++c) sumw += tot[c];
    std::vector<double>& init = h.init; init.assign(K, 0.0);
    double ymin = 0.0, ymax = 0.0;
    const double keps = k_eps();
    if (obj == 2) {
        bool first = true; double suml = 0.0;
        for (int c = 0; c < n_y; ++c) {
            if (!ycnt[c]) continue;
            if (first) { ymin = ymax = y_value[c]; first = false; }
            ymin = std::min(ymin, y_value[c]); ymax = std::max(ymax, y_value[c]);
        }
        if (hls && hls->valid) suml = hls->suml; else for (int c = 0; c < nl; ++c) suml += tot[c] * (c < n_y ? y_value[c] : 0.0);
        init[0] = suml / sumw;
    } else if (obj == 0) {
        double pavg = tot[1] / sumw;
        if (pavg > 1.0 - keps) pavg = 1.0 - keps;
        if (pavg < keps) pavg = keps;
        init[0] = std::log(pavg / (1.0 - pavg));
    } else {
        for (int k = 0; k < K; ++k) { double pr = tot[k] / sumw; init[k] = std::log(pr > keps ? pr : keps); }
    }
    const double factor = obj == 1 ? (double)K / (double)(K - 1) : 1.0;
    double bound_g, bound_h;
    if (obj == 2) { bound_g = (ymax - ymin) * w_max; if (!(bound_g > 0.0)) bound_g = 1.0; bound_h = w_max; }
    else if (obj == 0) { bound_g = w_max; bound_h = 0.25 * w_max; }
    else { bound_g = w_max; bound_h = factor * 0.25 * w_max; }
    // fixed-point grid of the histogram sums (numerics v2.2, rgbm_numerics.h).  The FLOOR of every class tree's exponent is v2.1's: |g_i| <= (bound_g / w_max) * w_i
    // and h_i <= (bound_h / w_max) * w_i hold for every row i, so with e = min(50 - ceil_log2(bound), 62 - ceil_log2(bound * sum_w / w_max)) every converted value is
    // at most 2^50 in magnitude (the range of the rint trick) and an int64 sum over all training rows (of all ranks) stays below 2^62.  The exponent a class tree
    // actually gets in an iteration comes from the measured coarse sums of its gradients (FxGrid -> k_fx_scale / k_small_tree).
    double wr = sumw / w_max;
    long long q_mult = 1;
    // TEST hook (tests/test_numerics_bound.py, tools/numerics_scale.py; the oracle reads the same pair): RGBM_TEST_HOOKS=1 + RGBM_FX_ROWS = R sizes the grid as if the
    // table held R training rows with this table's gradient distribution -- the grid a 10M / 100M-row table of this kind gets, on a table that trains in seconds.
    // It changes every model: only honoured with the explicit switch, and said on stderr.
    if (const char* th = std::getenv("RGBM_TEST_HOOKS")) if (std::atoi(th) != 0) if (const char* ev = std::getenv("RGBM_FX_ROWS")) {
        const double R = std::atof(ev);
        if (R > (double)n_train && R <= 4294967296.0 && n_train > 0) {
            wr *= R / (double)n_train; q_mult = ((long long)R + n_train - 1) / n_train;
            static std::atomic<bool> said{false};
            if (!said.exchange(true)) fprintf(stderr, "[rgbm] TEST HOOK active: RGBM_FX_ROWS=%s coarsens the fixed-point grid of every model trained by this process\n", ev);
        }
    }
    const int e_g = rg::fx_exponent(bound_g, wr), e_h = rg::fx_exponent(bound_h, wr);

    TrainConst& tc = h.tc; memset(&tc, 0, sizeof(tc));
    tc.sg = std::ldexp(1.0, e_g); tc.sh = std::ldexp(1.0, e_h); tc.inv_sg = std::ldexp(1.0, -e_g); tc.inv_sh = std::ldexp(1.0, -e_h);
    tc.l1 = p.lambda_l1; tc.l2 = p.lambda_l2; tc.min_gain_to_split = p.min_gain_to_split; tc.min_sum_hessian = p.min_sum_hessian_in_leaf;
    tc.learning_rate = p.learning_rate; tc.factor = factor; tc.min_data_in_leaf = p.min_data_in_leaf; tc.max_depth = p.max_depth;
    tc.num_leaves = p.num_leaves; tc.F = F; tc.K = K; tc.totbins = std::max(totbins, 1); tc.nchunk = nchunk; tc.objective = obj;
    tc.N = N; tc.n_train = n_train; tc.NG = N;
    tc.fx.c_g = 24 - rg::fx_ceil_log2(bound_g); tc.fx.c_h = 24 - rg::fx_ceil_log2(bound_h);
    tc.fx.e_g_min = e_g; tc.fx.e_h_min = e_h;
    tc.fx.e_g_max = 50 - rg::fx_ceil_log2(bound_g); tc.fx.e_h_max = 50 - rg::fx_ceil_log2(bound_h);
    tc.fx.q_mult = q_mult;
}

// the trees as the trainer leaves them in its flat device arrays (TreeOut), copied to the host: -> the model's tree list
struct HostTrees { const int32_t *L, *feat, *theta, *dleft, *left, *right, *cnt; const double *gain, *val; const int32_t* any; };
// two steps, so that the (many) trees of a batch of fits can be filled by several host threads: size the list, then fill ranges of it
size_t model_trees_begin(rgbm_model* model, const HostTrees& h, int NE, int K) {
    int n_iter = NE;
    for (int it = 0; it < NE; ++it) if (!h.any[it]) { n_iter = it > 0 ? it : 1; break; }   // "no more leaves that meet the split requirements"
    model->n_iter = n_iter;
    const size_t nt = (size_t)n_iter * K;
    model->trees.clear(); model->trees.resize(nt);
    size_t total = 0;
    for (size_t t = 0; t < nt; ++t) total += Tree::doubles(std::max(h.L[t], 1));
    model->tree_arena.reset(new double[std::max<size_t>(total, 1)]);
    size_t off = 0;
    for (size_t t = 0; t < nt; ++t) { const int L = std::max(h.L[t], 1); model->trees[t].place(model->tree_arena.get() + off, L); off += Tree::doubles(L); }
    return nt;
}
void model_trees_fill(rgbm_model* model, const HostTrees& h, int NL, size_t t0, size_t t1) {
    for (size_t t = t0; t < t1; ++t) {
        Tree& tr = model->trees[t];               // (placed by model_trees_begin)
        const size_t n = (size_t)tr.L - 1, nb = t * (NL - 1), lb = t * NL;
        memcpy(tr.feat, h.feat + nb, 4 * n); memcpy(tr.theta, h.theta + nb, 4 * n); memcpy(tr.dleft, h.dleft + nb, 4 * n);
        memcpy(tr.left, h.left + nb, 4 * n); memcpy(tr.right, h.right + nb, 4 * n); memcpy(tr.gain, h.gain + nb, 8 * n);
        memcpy(tr.leaf_value, h.val + lb, 8 * (size_t)tr.L); memcpy(tr.leaf_count, h.cnt + lb, 4 * (size_t)tr.L);
    }
}
void model_from_trees(rgbm_model* model, const HostTrees& h, int NE, int K, int NL) {
    const size_t n = model_trees_begin(model, h, NE, K);
    model_trees_fill(model, h, NL, 0, n);
}

// per-tree feature masks (ColSampler::ResetByTree), generated in LightGBM's draw order: [n_estimators * K][F]
std::vector<uint8_t> make_used_masks(const rgbm_params& p, size_t NT, int F, const std::vector<uint8_t>& trivial) {
    std::vector<uint8_t> used(NT * F, 0);
    LgbRand sr((uint32_t)p.seed);
    sr.rnd16(); sr.rnd16(); sr.rnd16();
    LgbRand ff((uint32_t)sr.rnd16());
    std::vector<int> valid; for (int f = 0; f < F; ++f) if (!trivial[f]) valid.push_back(f);
    for (size_t t = 0; t < NT; ++t) {
        uint8_t* u = used.data() + t * F;
        if (p.feature_fraction < 1.0) {
            int cntf = (int)std::floor((double)valid.size() * p.feature_fraction + 0.5);
            if (cntf < 1) cntf = 1;
            for (int i : ff.sample((int)valid.size(), cntf)) u[valid[i]] = 1;
        } else for (int f : valid) u[f] = 1;
    }
    return used;
}

// ---------------------------------------------------------------------------------------------
// Level grower, host side: the launch plan of the root pass and the level passes (pure arithmetic), the joint-bin packing of the
// root pass, and the table of the level-pass forms.
// ---------------------------------------------------------------------------------------------
// one k_level_mt launch of a level: (chunk, window of built slots); the first one of a level routes
struct MtLaunch { int ch, slot0, nslots, route, T, G, gx, acc2, rot; };
struct LevelPassPlan {
    int root_gx = 8;                                // row blocks per class tree of the root pass
    std::vector<std::vector<MtLaunch>> mt;          // [level] the launches of the level, levels 1 .. max_depth - 1
    std::vector<int> mt_gx;                         // [level] row blocks per class tree of the level's launches (one value per level: the partials share it)
    size_t part_items = 0;                          // nodes of the largest set of workgroup partials (root or level)
};

// What a launch of one-workgroup-per-CU passes costs, as the grid rules below see it:
//     rounds(workgroups) x (t_fix + rows per workgroup x (t_row + class trees per workgroup x t_pair)),   rounds(w) = ceil(w / 256 CUs).
// t_fix is what a workgroup does before its first row and after its last one (plan and layout look-up, route-table fill, zeroing, flush of its partials) plus
// its share of the launch; t_row the fetch of a row's record(s), once per workgroup; t_pair one (row, class tree) step of the row loop.  Calibration constants
// per form, from the per-launch intercepts and slopes of profiles/r13_step0_intercepts_parent_vs_new.md (its `new` columns; tools/level_setup_intercept.py: the same fits at two row counts
// with the row blocks pinned).  The model ranks grids of ONE launch form against each other; it is not a prediction of the step.
struct PassCost { double t_fix_us, t_row_ns, t_pair_ns; };
constexpr PassCost MT_COST_REP{14.0, 0.2, 0.75};      // k_level_mt, replicated layout
constexpr PassCost MT_COST_ROT{14.0, 1.0, 0.5};      // k_level_mt, rotated
constexpr PassCost ROOT_PASS_COST{8.0, 1.2, 0.0};        // k_level_root (one class tree per workgroup)
inline const PassCost& mt_pass_cost(bool /*acc2*/, bool rot) { return rot ? MT_COST_ROT : MT_COST_REP; }       // (the both-chunk forms: the one-chunk constants of their layout)
inline double pass_model_us(long long workgroups, double rows_per_block, int T, const PassCost& c) {
    const long long rounds = (workgroups + 255) / 256;
    return (double)rounds * (c.t_fix_us + rows_per_block * (c.t_row_ns + (double)T * c.t_pair_ns) * 1e-3);
}

// LDS bytes the level grower's passes size their histograms for (RGBM_LV_LDS, testing: a smaller pool forces several built-slot windows per level)
inline int level_lds_bytes(const RunSwitches& sw) { return (sw.lv_lds >= 65536 && sw.lv_lds <= rg::LV_LDS_BYTES) ? sw.lv_lds : rg::LV_LDS_BYTES; }

LevelPassPlan plan_level_passes(const RunSwitches& sw, const std::vector<rg::FeatMeta>& fmeta, const std::vector<rg::ChunkMeta>& cmeta,
                                long long N, int K, int max_depth, bool wm /* rows carry multiplicities */, int lds_bytes) {
    using namespace rg;
    const int nchunk = (int)cmeta.size();
    LevelPassPlan P;
    P.mt.resize(LV_MAX_DEPTH + 1); P.mt_gx.assign(LV_MAX_DEPTH + 1, 8);
    const long long ntiles = (N + LV_TILE - 1) / LV_TILE;
    // ---- root pass: one 1024-thread workgroup per CU and (class tree, row block, chunk).  Contiguous row blocks, a multiple of 8 per
    // class tree with all class trees of a row block on one XCD (k_level_root), about four rounds of 256 workgroups when the class
    // trees alone nearly fill the chip (measured at K = 64, 10M rows: 8 / 16 / 40 blocks per class tree = 23.0 / 21.0 / 23.2 ms per
    // iteration); <= 2^22 rows per workgroup.  RGBM_LV_BLOCKS overrides.
    {
        const long long cu_slots = 256, per = (long long)K * nchunk;
        const long long gmin = std::max<long long>(1, (N + (1ll << 22) - 1) >> 22);
        // Among the admitted block counts the modelled time decides (pass_model_us: a workgroup costs t_fix besides its rows), ties to the fewer workgroups.
        auto time_of = [&](long long g) { return pass_model_us(g * per, (double)N / (double)g, 1, ROOT_PASS_COST); };
        const long long gfloor = std::max<long long>(8, (gmin + 7) / 8 * 8), gcap = std::max<long long>(gfloor, std::min<long long>(512, (ntiles + 7) / 8 * 8));
        long long g2 = gfloor; double best2 = -1.0;
        for (int pass = 0; pass < 2 && best2 < 0.0; ++pass)          // (second pass: no block count inside the three-to-five-round window)
            for (long long g = gfloor; g <= gcap; g += 8) {
                if (pass == 0 && per >= 16 && (g * per < 3 * cu_slots || g * per > 5 * cu_slots)) continue;
                const double t = time_of(g);
                if (best2 < 0.0 || t < best2 * (1.0 - 1e-9)) { best2 = t; g2 = g; }
            }
        if (sw.lv_blocks >= 1) g2 = (sw.lv_blocks + 7) / 8 * 8;
        P.root_gx = (int)g2;
    }
    for (int ch = 0; ch < nchunk; ++ch)
        if ((long long)lv_slots(fmeta.data() + cmeta[ch].first_feat, cmeta[ch].nfeat, 0) * 16 + LV_ROOT_FIXED > lds_bytes)
            throw std::invalid_argument("histogram of one node exceeds LDS");
    // ---- level passes (k_level_mt).  Per chunk: how many built nodes the LDS holds next to the rings (cap), hence how many class
    // trees share a workgroup (T = cap / worst-case built nodes of the level, 2^(L-1)) or, when one class tree's nodes do not fit,
    // how many launches ("windows" of built slots) the level takes.  Every class tree group gets the same row blocks, a multiple of 8
    // (one XCD each), enough to fill the chip once (<= 2^22 rows per workgroup).
    P.part_items = (size_t)K * P.root_gx;                   // root partials: one node per (class tree, row block)
    for (int level = 1; level < max_depth; ++level) {
        const int worst = 1 << (level - 1);
        // tables of 17..32 features: ONE wave-specialised pass per level accumulates both 16-feature chunks (k_level_mt<2, ., ., MT_THREADS_ACC2, true, true>:
        // both records of a row in registers and in the ring) instead of one pass per chunk that streams every (node id, g, h) again
        bool acc2 = nchunk == 2 && sw.mt_acc2;
        if (acc2) {   // ... when one node's histograms of both chunks fit the LDS of the 768-thread workgroup (else: one pass per chunk, as for > 32 features)
            const long long nb2 = ((long long)lv_slots(fmeta.data() + cmeta[0].first_feat, cmeta[0].nfeat, 0) + lv_slots(fmeta.data() + cmeta[1].first_feat, cmeta[1].nfeat, 0)) * 16;
            if (nb2 > mt_hist_bytes(lds_bytes, MT_THREADS_ACC2, true, true, cmeta[1].nfeat > 15 || wm)) acc2 = false;
        }
        if (wm && nchunk == 2 && !acc2) throw std::invalid_argument("a two-chunk table with row multiplicities needs the one-pass level form (the multiplicity rides in the second record)");
        for (int ch = 0; ch < (acc2 ? 1 : nchunk); ++ch) {
            const FeatMeta* fm = fmeta.data() + cmeta[ch].first_feat;
            long long node_bytes = (long long)lv_slots(fm, cmeta[ch].nfeat, 0) * 16;
            if (acc2) node_bytes += (long long)lv_slots(fmeta.data() + cmeta[1].first_feat, cmeta[1].nfeat, 0) * 16;
            const int mt_thr = acc2 ? MT_THREADS_ACC2 : LV_THREADS;
            const bool li_arr = cmeta[acc2 ? 1 : ch].nfeat > 15 || wm;          // the ring needs a slot array (k_level_mt: !li_in_rec)
            const long long hist_room = mt_hist_bytes(lds_bytes, mt_thr, acc2, acc2 /* the both-chunk pass is the wave-specialised one */, li_arr);
            long long cap = hist_room / std::max<long long>(node_bytes, 1);
            cap = std::min<long long>(cap, MT_MAX_NODES);
            if (cap < 1) throw std::invalid_argument("histogram of one node exceeds LDS");
            const int win = (int)std::min<long long>(worst, cap);                    // built slots per launch
            // LDS left over after the T class trees' nodes becomes replication (2^s copies of every bin).  A batch of 64 built rows comes from
            // one or two class trees (a wave walks them one after another) and, at the shallow levels, from one or two nodes: without
            // replication its lanes pile up on a handful of addresses (measured at K = 64: 23-31 cycles per atomic instruction at
            // replication 1 against 12.8 in the root pass).  So T is sized for `mt_rep` copies first; the records the extra workgroups
            // re-read come out of the XCD's L2 (all class tree groups of a row block run on one XCD at the same time).
            const long long rep_target = std::max(1, sw.mt_rep);
            const long long t_nodes = std::max<long long>(win, cap / rep_target);
            int T = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(t_nodes / win, MT_MAX_T), std::min<long long>(K, MT_RT_BUDGET / (2 * worst))));
            if (sw.mt_T >= 1) T = std::max(1, std::min(T, sw.mt_T));
            // Feature rotation of the histogram updates (rgbm_level.h, "FEATURE ROTATION") for the launches whose LDS holds fewer than eight copies (RGBM_MT_ROT_COPIES2 / 2) of their
            // worst-case histograms -- the deepest dense levels, where rows of one cluster pile up on one address per feature: measured -11 % at
            // level 5 of the K = 64 target and +35-60 % where there IS room for replicas (profiles/r5c_*), hence per launch.
            const bool plain1 = nchunk == 1 || acc2;      // the two forms that exist with rotation (RGBM_MT_FORMS)
            // (a rotated step works on sixteen feature slots per chunk whatever the chunk holds: with few features most lanes of a step idle -- rotate only chunks
            // that fill at least three quarters of them)
            const bool rot_full = cmeta[ch].nfeat >= 12 && (!acc2 || cmeta[1].nfeat >= 12);
            // ... and (round 6) where the replicated layout would leave the workgroup fewer than RGBM_MT_ROT_TMIN (2: a single one) class trees although one copy holds at least twice
            // as many: every doubling of the class trees per workgroup is ~5 % of a deep level (the records are read once per T steps), which eight copies do not buy back
            const long long rot_node_bytes = node_bytes + mt_rot_dummy(true) * 16;
            const long long cap_rot = std::min<long long>(hist_room / rot_node_bytes, MT_MAX_NODES);
            const long long T_rot = std::min<long long>(std::min<long long>(cap_rot / win, MT_MAX_T), std::min<long long>(K, MT_RT_BUDGET / (2 * worst)));
            const bool few_trees = T < sw.mt_rot_tmin && T_rot >= 2 * (long long)T;
            const bool rot = plain1 && (sw.mt_rot == 1 || (sw.mt_rot < 0 && rot_full && (cap * 2 < (long long)sw.mt_rot_copies2 * T * win || few_trees))) &&
                             (long long)T * win * rot_node_bytes <= hist_room;
            // a rotated launch needs ONE copy: as many class trees per workgroup as the LDS holds
            if (rot && sw.mt_T < 1) T = (int)std::max<long long>(T, T_rot);
            const int G = (K + T - 1) / T;
            for (int s0 = 0; s0 < worst; s0 += win)
                P.mt[level].push_back(MtLaunch{ch, s0, win, (ch == 0 && s0 == 0) ? 1 : 0, T, G, 0, acc2 ? 1 : 0, rot ? 1 : 0});
        }
        const long long gmin = std::max<long long>(1, (N + (1ll << 22) - 1) >> 22);
        // row blocks per class tree: a multiple of 8 (one XCD each); G * gx workgroups should fill whole rounds of 256 CUs (G = 24: 8 row
        // blocks leave a quarter of the chip idle, 32 make three full rounds) without cutting the table into slivers
        const long long nwt = (N + MT_WT_ROWS - 1) / MT_WT_ROWS;
        const long long gx_lo = std::max<long long>(8, (gmin + 7) / 8 * 8), gx_hi = std::max<long long>(gx_lo, std::min<long long>(512, (nwt / (4 * (LV_THREADS / 64)) + 7) / 8 * 8));
        // ... chosen by the modelled time of the level's launches (pass_model_us): a workgroup costs t_fix before its first row, so 1496 workgroups of
        // 18 k rows (G = 11: six rounds filled to 97 %, what filling whole rounds alone picks) lose to 440 of 62 k rows (two rounds filled to 86 %).
        // Ties go to the fewer workgroups.
        long long gx = gx_lo; double best = 0.0;
        for (long long g = gx_lo; g <= gx_hi; g += 8) {
            double t = 0.0;
            for (const auto& L : P.mt[level]) t += pass_model_us((long long)L.G * g, (double)N / (double)g, std::min(L.T, K), mt_pass_cost(L.acc2 != 0, L.rot != 0));
            if (g == gx_lo || t < best * (1.0 - 1e-9)) { best = t; gx = g; }
        }
        if (sw.mt_blocks >= 1) gx = (sw.mt_blocks + 7) / 8 * 8;
        P.mt_gx[level] = (int)gx;
        for (auto& L : P.mt[level]) L.gx = (int)gx;
        P.part_items = std::max(P.part_items, (size_t)K * (size_t)gx * (size_t)worst);
    }
    return P;
}

// Joint bins for the root pass, host half: best-fit-decreasing packing of the features into groups whose bin counts multiply to <= 256;
// worth it when it saves at least two atomics per row, the groups fit one 16-byte record (15 bytes when byte 15 carries the row's
// multiplicity) and their histograms fit the LDS.  on == false: the root pass keeps the plain records.
struct JointRootPlan {
    bool on = false;
    std::vector<std::vector<int>> groups;           // features of every group
    std::vector<rg::FeatMeta> vfm; rg::ChunkMeta vcm;   // the groups as the features of ONE virtual chunk
    std::vector<rg::JointFeat> jf;                  // [F] where a feature sits in its group's joint code
    std::vector<int16_t> binfeat;                   // [totbins] bin -> feature
};
JointRootPlan plan_joint_root(const std::vector<rg::FeatMeta>& fmeta, int totbins, bool wm, int lds_bytes) {
    using namespace rg;
    const int F = (int)fmeta.size();
    JointRootPlan J;
    std::vector<int> order(F); for (int f = 0; f < F; ++f) order[f] = f;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return fmeta[a].nbins > fmeta[b].nbins; });
    std::vector<int> prod;
    for (int f : order) {
        int best = -1;
        for (size_t g = 0; g < J.groups.size(); ++g)
            if ((long long)prod[g] * fmeta[f].nbins <= 256 && (best < 0 || prod[g] > prod[best])) best = (int)g;
        if (best < 0) { J.groups.emplace_back(); prod.push_back(1); best = (int)J.groups.size() - 1; }
        J.groups[best].push_back(f); prod[best] *= fmeta[f].nbins;
    }
    const int VF = (int)J.groups.size();
    if (VF > (wm ? 15 : 16) || VF > F - 2) return J;
    J.vfm.resize(VF); J.jf.resize(F); J.binfeat.assign(totbins, 0);
    ChunkMeta& vcm = J.vcm; vcm.first_feat = 0; vcm.nfeat = VF; vcm.fast_slots = 0; vcm.wide_bins = 0;
    for (int v = 0; v < VF; ++v) {
        FeatMeta& m = J.vfm[v]; memset(&m, 0, sizeof(m));
        m.V = prod[v]; m.has_nan = 0; m.nbins = prod[v]; m.hoff = vcm.wide_bins; m.wide_off = vcm.wide_bins;
        int sh = 0; while (sh < 5 && (m.nbins << (sh + 1)) <= 256) ++sh;
        m.rep_shift = sh; m.fast_base = vcm.fast_slots; vcm.fast_slots += m.nbins << sh; vcm.wide_bins += m.nbins;
        int stride = 1;
        for (int f : J.groups[v]) {
            JointFeat& j = J.jf[f]; memset(&j, 0, sizeof(j));
            j.voff = m.hoff; j.stride = stride; j.nbins = fmeta[f].nbins; j.nbv = prod[v]; j.hoff = fmeta[f].hoff; j.vbyte = v;
            stride *= fmeta[f].nbins;
            for (int b = 0; b < fmeta[f].nbins; ++b) J.binfeat[fmeta[f].hoff + b] = (int16_t)f;
        }
    }
    J.on = (long long)lv_slots(J.vfm.data(), VF, 0) * 16 + LV_ROOT_FIXED <= lds_bytes;
    return J;
}

// The forms of the level pass that exist, (NCHR, THREADS, ACC2, SPEC, ROTP), each for BAG x ROUTE: the ONE list behind the LDS attribute
// and the launch, so a form cannot be launched without its attribute.  k_level_mt's static_assert admits the same six.
#define RGBM_MT_FORMS(X) \
    X(0, rg::LV_THREADS, false, false, false) /* any number of chunks: the split byte is gathered */ \
    X(1, rg::LV_THREADS, false, false, false) /* one chunk */ \
    X(1, rg::LV_THREADS, false, false, true)  /* one chunk, rotated */ \
    X(2, rg::LV_THREADS, false, false, false) /* two chunks, one pass per chunk */ \
    X(2, rg::MT_THREADS_ACC2, true, true, false) /* two chunks in one wave-specialised pass */ \
    X(2, rg::MT_THREADS_ACC2, true, true, true)  /* ... rotated */
struct MtForm { int nchr, threads; bool acc2, spec, rot; };
constexpr MtForm MT_FORMS[] = {
#define RGBM_MT_FORM_ENTRY(NCHR, THR, ACC, SPEC, ROT) {NCHR, THR, ACC, SPEC, ROT},
    RGBM_MT_FORMS(RGBM_MT_FORM_ENTRY)
#undef RGBM_MT_FORM_ENTRY
};
using MtKernel = decltype(&rg::k_level_mt<1, false, true, rg::LV_THREADS, false, false, false>);      // (every instantiation has this signature)
MtKernel mt_kernel(const MtForm& f, bool bag, bool route) {
#define RGBM_MT_FORM_KERNEL(NCHR, THR, ACC, SPEC, ROT) \
    if (f.nchr == NCHR && f.threads == THR && f.acc2 == ACC && f.spec == SPEC && f.rot == ROT) \
        return bag ? (route ? rg::k_level_mt<NCHR, true, true, THR, ACC, SPEC, ROT> : rg::k_level_mt<NCHR, true, false, THR, ACC, SPEC, ROT>) \
                   : (route ? rg::k_level_mt<NCHR, false, true, THR, ACC, SPEC, ROT> : rg::k_level_mt<NCHR, false, false, THR, ACC, SPEC, ROT>);
    RGBM_MT_FORMS(RGBM_MT_FORM_KERNEL)
#undef RGBM_MT_FORM_KERNEL
    throw std::logic_error("level pass: no such launch form");
}
// (the parameter list is k_level_mt's own)
void launch_level_mt(const MtForm& f, bool bag, bool route, dim3 grid, hipStream_t s, const uint4* rec, const float2* gh, uint8_t* node, const uint8_t* inbag,
                     const rg::LvPlan* plan, rg::HistBin* part, int32_t* count, const rg::FeatMeta* fmeta, const rg::ChunkMeta* cmeta, int32_t* err_flag,
                     const rg::FxScale* fxs, const rg::LevelConst& c) {
    // (always the CU's whole LDS: the hessian sums sit a compile-time distance behind the gradient sums; LevelConst::lds_bytes, the test hook, only sizes the histograms)
    hipLaunchKernelGGL(mt_kernel(f, bag, route), grid, dim3(f.threads), rg::LV_LDS_BYTES, s, rec, gh, node, inbag, plan, part, count, fmeta, cmeta, err_flag, fxs, c);
}
// HIP events around every histogram launch of a training call, on the stream it is launched on; only when stats are requested
struct HistTimers {
    bool on; hipStream_t s;
    std::deque<rgh::Event> ev; std::vector<char> root;      // launch i: events 2i (before) and 2i + 1 (after)
    template <typename Fn> void timed(bool is_root, Fn&& fn) {
        if (!on) { fn(); return; }
        HIPCHK(hipEventRecord(ev.emplace_back().e, s));
        fn();
        HIPCHK(hipEventRecord(ev.emplace_back().e, s));
        root.push_back(is_root ? 1 : 0);
    }
};

// RGBM_TRACE=<dir> (debugging; with RGBM_TRACE_K=<class trees> and RGBM_TRACE_ITERS=lo:hi): snapshots of the level grower's state after every
// level of the iterations lo..hi and a checksum of (score, g/h, node ids) after every iteration, written to <dir>/target<col>.{bin,idx}
struct LevelTrace {
    struct Rec { std::string name; int it, level; size_t off, bytes; };
    const char* dir; bool on; hipStream_t s;
    int lo = 44, hi = 44, cur_it = 0;
    std::vector<Rec> idx; size_t used = 0;
    DevBuf<unsigned char> buf;              // sized by the caller when `on`
    LevelTrace(bool level_mode, int K, hipStream_t stream) : dir(getenv("RGBM_TRACE")), s(stream) {
        on = dir && level_mode && (!getenv("RGBM_TRACE_K") || atoi(getenv("RGBM_TRACE_K")) == K);
        if (on && getenv("RGBM_TRACE_ITERS")) sscanf(getenv("RGBM_TRACE_ITERS"), "%d:%d", &lo, &hi);
    }
    void copy(const char* name, int level, const void* src, size_t bytes) {
        if (!on || cur_it < lo || cur_it > hi) return;
        if (used + bytes > buf.n) return;
        HIPCHK(hipMemcpyAsync(buf.p + used, src, bytes, hipMemcpyDeviceToDevice, s));
        idx.push_back({name, cur_it, level, used, bytes}); used += (bytes + 15) & ~(size_t)15;
    }
    void sum(const char* name, const void* src, size_t bytes) {
        if (!on || used + 16 > buf.n) return;
        HIPCHK(hipMemsetAsync(buf.p + used, 0, 8, s));
        rgh::trace_sum(src, bytes, (unsigned long long*)(buf.p + used), s);
        idx.push_back({name, cur_it, -1, used, 8}); used += 16;
    }
    void write(int target_col) {            // (after the stream has drained)
        if (!on || !used) return;
        std::vector<unsigned char> h(used);
        HIPCHK(hipMemcpy(h.data(), buf.p, used, hipMemcpyDeviceToHost));
        char path[512];
        snprintf(path, sizeof(path), "%s/target%d.bin", dir, target_col);
        if (FILE* f = fopen(path, "wb")) { fwrite(h.data(), 1, h.size(), f); fclose(f); }
        snprintf(path, sizeof(path), "%s/target%d.idx", dir, target_col);
        if (FILE* f = fopen(path, "w")) { for (const auto& r : idx) fprintf(f, "%s %d %d %zu %zu\n", r.name.c_str(), r.it, r.level, r.off, r.bytes); fclose(f); }
    }
};

// rgbm_train_stats of a finished training call
void fill_train_stats(rgbm_train_stats* stats, float total_ms, const HistTimers& timers, const HostTrees& h, const rgbm_params& p, bool level_mode, bool use_bagging,
                      int nranks /* row-sharded: the ranks that share the table */, int64_t N, int64_t n_train, int F, int root_feats /* feature groups of the root pass */,
                      int K, unsigned long long statrows) {
    const int NE = p.n_estimators, NL = p.num_leaves;
    memset(stats, 0, sizeof(*stats));
    stats->total_ms = total_ms;
    stats->hist_launches = (int64_t)timers.root.size();
    for (size_t i = 0; i < timers.root.size(); ++i) {
        float m2 = 0.f; HIPCHK(hipEventElapsedTime(&m2, timers.ev[2 * i].e, timers.ev[2 * i + 1].e));
        stats->hist_ms += m2; if (timers.root[i]) stats->root_ms += m2;
    }
    stats->trees = (int64_t)NE * K;
    const bool root_done = n_train >= (int64_t)p.min_data_in_leaf * 2;
    if (level_mode) {
        // rows whose (g,h) were accumulated: counted on the device (k_level_step); root passes = trees with a searched root
        // (bag sizes vary: not tracked separately).  Row-sharded: the device counter sums GLOBAL child counts on every rank; report this rank's share
        const int64_t root_rows = (root_done && !use_bagging) ? (int64_t)NE * K * n_train : 0;
        const int64_t rows_acc = (int64_t)(statrows / (unsigned long long)nranks);
        stats->hist_rows = rows_acc; stats->root_rows = root_rows / nranks;
        stats->root_atomics_per_row = 2 * (int64_t)root_feats; stats->level_atomics_per_row = 2 * (int64_t)F;
        // algorithmic bytes: F bin bytes + 8 B (g,h) per accumulated row
        stats->hist_bytes = rows_acc * ((int64_t)F + 8);
        return;
    }
    // rows scanned: root = N per class tree; otherwise the smaller child of every split, which the
    // trees record (leaf_count of both children is known at the end only for final leaves), so
    // replay the growth order on the host from the stored counts.
    int64_t rows = 0, root_rows = 0;
    for (size_t t = 0; t < (size_t)NE * K; ++t) {
        const int L = h.L[t];
        const int32_t* left = h.left + t * (NL - 1); const int32_t* right = h.right + t * (NL - 1);
        if (root_done) { rows += N; root_rows += N; }
        // final leaf counts -> internal counts: node j created leaf j+1 from some leaf; recover via children links
        std::vector<int64_t> fin(h.cnt + t * NL, h.cnt + t * NL + NL);
        std::vector<int64_t> nodecnt(std::max(L - 1, 1), 0);
        auto sub = [&](int ch) -> int64_t { return ch < 0 ? fin[~ch] : nodecnt[ch]; };
        for (int j = L - 2; j >= 0; --j) nodecnt[j] = sub(left[j]) + sub(right[j]);
        std::vector<int> node_depth(std::max(L - 1, 1), 0);
        for (int j = 0; j < L - 1; ++j) {
            const int lc = left[j], rc = right[j];
            if (lc >= 0) node_depth[lc] = node_depth[j] + 1;
            if (rc >= 0) node_depth[rc] = node_depth[j] + 1;
            const int64_t a = sub(lc), b = sub(rc);
            bool go = j + 2 < NL;
            if (p.max_depth > 0 && node_depth[j] + 1 >= p.max_depth) go = false;
            if (a < (int64_t)p.min_data_in_leaf * 2 && b < (int64_t)p.min_data_in_leaf * 2) go = false;
            if (go) rows += std::min(a, b);
        }
    }
    stats->hist_rows = rows; stats->root_rows = root_rows;
    // algorithmic bytes use the USEFUL feature bytes (F), not the padded record
    stats->hist_bytes = rows * ((int64_t)F + 8) + (rows - root_rows) * 4;
}

// ---------------------------------------------------------------------------------------------
// Set-up that the single-fit trainer (train_core) and the batched small-table trainer (train_batch_small) share: the argument
// checks of a fit, its code counts, its bin records, its bagging state and the block of arrays its trees are written to.
// ---------------------------------------------------------------------------------------------
void check_fit_args(const rgbm_table& tab, int32_t target_col, const int32_t* feat_cols, int32_t F, const double* y_value, const rgbm_params& p) {
    check_params(p);
    if (F <= 0) throw std::invalid_argument("no feature columns");
    if (target_col < 0 || target_col >= tab.c) throw std::invalid_argument("target column out of range");
    for (int f = 0; f < F; ++f) if (feat_cols[f] < 0 || feat_cols[f] >= tab.c) throw std::invalid_argument("feature column out of range");
    const int obj = p.objective, n_y = tab.n_codes[target_col];
    if (obj == 1 && n_y > p.num_class) throw std::out_of_range("target has more label codes than num_class");
    if (obj == 0 && n_y > 2) throw std::out_of_range("binary objective with more than 2 label codes");
    if (obj == 2 && !y_value) throw std::out_of_range("regression needs the y_value dictionary");
}

// The bin tables of a fit on the device and the records of its rows: [nchunk][N] x 16 bytes, one byte per feature.  First the device side
// of FitHost's cols / ncod / cnt_off / cnt: the fit's columns (the features, then the target), their dictionary sizes, the code counts.
struct BinRecords {
    DevBuf<int32_t> cols, ncod; DevBuf<long long> cnt_off; DevBuf<unsigned int> cnt;
    DevBuf<rg::FeatMeta> fmeta; DevBuf<rg::ChunkMeta> cmeta; DevBuf<long long> lut_off; DevBuf<uint8_t> lut, miss; DevBuf<uint4> rec;
    // Code frequencies of the training rows (features + the target itself).  Enqueue only: download_counts brings them to h.cnt, and the
    // caller synchronises before it reads them (a batch once for all its fits).
    void count_codes(const rgbm_table& tab, int32_t target_col, const int32_t* feat_cols, int32_t F, FitHost& h, hipStream_t s) {
        h.cols.assign(feat_cols, feat_cols + F); h.cols.push_back(target_col);
        h.ncod.resize(F + 1); h.cnt_off.assign(F + 2, 0);
        for (int f = 0; f <= F; ++f) { h.ncod[f] = tab.n_codes[h.cols[f]]; h.cnt_off[f + 1] = h.cnt_off[f] + std::max(h.ncod[f], 1); }
        cols.alloc(F + 1); ncod.alloc(F + 1); cnt_off.alloc(F + 2); cnt.alloc(h.cnt_off[F + 1]);
        cols.upload(h.cols.data(), F + 1, s); ncod.upload(h.ncod.data(), F + 1, s); cnt_off.upload(h.cnt_off.data(), F + 2, s); cnt.zero(s);
        const int gx = (int)std::min<int64_t>((tab.n + 255) / 256, 1024);
        hipLaunchKernelGGL(rg::k_count_codes, dim3(gx, F + 1), dim3(256), 0, s, tab.codes.p, (long long)tab.n, tab.codes.p + (long long)target_col * tab.n, cols.p, ncod.p,
                           cnt_off.p, cnt.p, tab.has_mult ? tab.mult.p : (const uint8_t*)nullptr);
    }
    void download_counts(FitHost& h, hipStream_t s) const { h.cnt.resize(cnt.n); cnt.download(h.cnt.data(), cnt.n, s); }
    void fill(const FitHost& h, long long N, hipStream_t s) {
        const int F = h.tc.F;
        fmeta.alloc(F); cmeta.alloc(h.nchunk); lut_off.alloc(F + 1); lut.alloc(h.lut.size()); miss.alloc(F);
        fmeta.upload(h.fmeta.data(), F, s); cmeta.upload(h.cmeta.data(), h.nchunk, s); lut_off.upload(h.lut_off.data(), F + 1, s);
        lut.upload(h.lut.data(), h.lut.size(), s); miss.upload(h.miss.data(), F, s);
        rec.alloc((size_t)h.nchunk * N);
    }
    // bin records of the rows of `t` (the fit's table, or a table with the same columns) through a lookup table of the fit
    void pack(const rgbm_table& t, const uint8_t* lut_, const uint8_t* miss_, uint4* out, const uint8_t* mult, hipStream_t s) const {
        hipLaunchKernelGGL(rg::k_pack_bins, dim3((unsigned)((t.n + 255) / 256)), dim3(256), 0, s, t.codes.p, (long long)t.n, 0ll, (long long)t.n, cols.p, ncod.p,
                           lut_off.p, lut_, miss_, (int)fmeta.n, (int)cmeta.n, out, mult);
    }
    void pack(const rgbm_table& tab, hipStream_t s) { pack(tab, lut.p, miss.p, rec.p, tab.has_mult ? tab.mult.p : (const uint8_t*)nullptr, s); }
};

// bagging state (GBDT::Bagging): stable training-row order, one LCG per 1024 positions
struct BagState {
    DevBuf<unsigned int> blk, rand, bagcnt; DevBuf<int32_t> sorted_rows, oob; DevBuf<uint8_t> inbag;      // (inbag.p stays null without bagging: the kernels' "every row")
    std::vector<unsigned int> seeds;       // host source of an asynchronous upload: alive until the stream has drained
    long long off = 0, local = 0, nrb = 1;
    void order_rows(const int32_t* d_ycol, long long N, long long n_train, hipStream_t s) {
        const long long nblk = (N + 1023) / 1024;
        blk.alloc(nblk); sorted_rows.alloc(n_train); oob.alloc(n_train); inbag.alloc(N); bagcnt.alloc(2);
        hipLaunchKernelGGL(rg::k_block_count, dim3((unsigned)nblk), dim3(256), 0, s, d_ycol, N, blk.p);
        hipLaunchKernelGGL(rg::k_block_scan, dim3(1), dim3(1024), 0, s, blk.p, nblk);
        hipLaunchKernelGGL(rg::k_stable_compact, dim3((unsigned)nblk), dim3(256), 0, s, d_ycol, N, blk.p, sorted_rows.p);
    }
    // the draws go per training-row POSITION: this table's rows hold the positions [bag_off, bag_off + bag_local) of n_train (a row shard: a part of them)
    void seed(const rgbm_params& p, long long bag_off, long long bag_local, hipStream_t s) {
        off = bag_off; local = bag_local;
        nrb = std::max<long long>(1, (off + local + 1023) / 1024 - off / 1024);
        LgbRand sr2((uint32_t)p.seed); sr2.rnd16();
        const int bagging_seed = sr2.rnd16();
        seeds.resize(nrb);
        for (long long b = 0; b < nrb; ++b) seeds[b] = (unsigned int)(bagging_seed + off / 1024 + b);
        rand.alloc(nrb); rand.upload(seeds.data(), nrb, s);
    }
};

// The trees of a fit as the trainer's kernels write them (rg::TreeOut) plus `any` (per iteration: did any class tree split), and their
// way to the host: ONE block with the ten arrays at 64-byte boundaries, whoever owns it (a vector, a slice of the page-locked arena).
struct TreeBlock {
    DevBuf<int32_t> L, feat, theta, dleft, left, right, cnt, any; DevBuf<double> gain, val;
    void alloc(size_t NT, int NL, int NE, hipStream_t s) {
        const size_t nn = NT * (size_t)(NL - 1), nl = NT * (size_t)NL;
        any.alloc(NE); any.zero(s);
        L.alloc(NT); feat.alloc(nn); theta.alloc(nn); dleft.alloc(nn); left.alloc(nn); right.alloc(nn); cnt.alloc(nl); gain.alloc(nn); val.alloc(nl);
        cnt.zero(s); val.zero(s);
    }
    rg::TreeOut out() const { return rg::TreeOut{L.p, feat.p, theta.p, dleft.p, left.p, right.p, gain.p, val.p, cnt.p}; }
    // The host layout: byte offsets of L, feat, theta, dleft, left, right, cnt, gain, val, any, each at a 64-byte boundary; [10] = the block's size
    void host_layout(size_t (&off)[11]) const {
        const size_t bytes[10] = {L.n * 4, feat.n * 4, theta.n * 4, dleft.n * 4, left.n * 4, right.n * 4, cnt.n * 4, gain.n * 8, val.n * 8, any.n * 4};
        off[0] = 0;
        for (int i = 0; i < 10; ++i) off[i + 1] = off[i] + ((bytes[i] + 63) & ~(size_t)63);
    }
    size_t host_bytes() const { size_t off[11]; host_layout(off); return off[10]; }
    // enqueues the copies into a host block of host_bytes() bytes and returns the view of it (valid once the stream has drained)
    HostTrees download(char* base, hipStream_t s) const {
        size_t off[11]; host_layout(off);
        auto get = [&](const auto& buf, int i) { auto* h = reinterpret_cast<decltype(buf.p)>(base + off[i]); buf.download(h, buf.n, s); return h; };
        return HostTrees{get(L, 0), get(feat, 1), get(theta, 2), get(dleft, 3), get(left, 4), get(right, 5), get(cnt, 6), get(gain, 7), get(val, 8), get(any, 9)};
    }
};

// ---------------------------------------------------------------------------------------------
// The trainer (GBDT::Train) on a resident table: train_core = prologue (checks, code counts, bins, records) -> the state both growers
// work on (FitState) -> one grower (LevelGrower wherever it applies, else LeafwiseGrower; both are HIP and give the same models) ->
// the boosting loop and the harvest.
// ---------------------------------------------------------------------------------------------
// What a boosting iteration works on whichever grower builds the trees.  The growers keep a reference to it and only READ it, when they
// enqueue: train_core fills the members from the weights on AFTER it has built the grower (the order the work goes on the stream).
struct FitState {
    const rgbm_table& tab; const rgbm_params& p; hipStream_t s; const int32_t F;
    const RunSwitches sw = read_switches();
    const int K = p.objective == 1 ? p.num_class : 1, NL = p.num_leaves, NE = p.n_estimators; const int64_t N = tab.n;
    const bool use_bagging = p.bagging_freq > 0 && p.bagging_fraction < 1.0;
    // grower choice: the level-synchronous streaming grower (rgbm_level.h) whenever it applies; RGBM_GROWER=leafwise forces the index-list grower
    const bool level_mode = p.max_depth >= 1 && p.max_depth <= rg::LV_MAX_DEPTH && F <= 255 && sw.grower != 2;
    const bool dp = (p.reserved & RGBM_FLAG_ROW_SHARDED) != 0;     // the table is one rank's row shard (rgbm_params.reserved bit 0)
    const int32_t* d_ycol; const uint8_t* d_mult = tab.has_mult ? tab.mult.p : (const uint8_t*)nullptr;
    FitHost h; BinRecords bins;
    DevBuf<int32_t> base;              // the training rows in ascending order (the leaf-wise grower's root list, the bag lists' source)
    DevBuf<unsigned int> counter;      // ... and how many they are
    DevBuf<float2> gh;                 // float32 (g, h) of every (row, class tree); non-training rows stay (0, 0)
    DevBuf<double> score, init;
    DevBuf<unsigned long long> fxq;    // numerics v2.2: coarse gradient sums of the iteration's class trees (k_fx_scale zeroes them again)
    DevBuf<rg::FxScale> fxs;           // ... and the grid they give every class tree
    DevBuf<unsigned long long> qpart; long long fx_parts = 0; bool fx_fused = false;      // the gradient kernels measure the coarse sums themselves (qpart.p is null otherwise)
    TreeBlock trees;
    DevBuf<double> cw, yv, sw_rows; DevBuf<uint8_t> used;
    BagState bag; DevBuf<unsigned int> bagcnt_g;
    const unsigned int* n_in_ptr = nullptr;          // rows in the bag of the current iteration, over ALL ranks when row-sharded (the root count of every tree)
    DevBuf<int32_t> it;                // device-side iteration counter of the level grower (k_level_init)
    HistTimers timers;

    FitState(const rgbm_table& tab_, int32_t target_col, int32_t F_, const rgbm_params& p_, bool timed, hipStream_t s_)
        : tab(tab_), p(p_), s(s_), F(F_), d_ycol(tab_.codes.p + (long long)target_col * tab_.n), timers{timed, s_} {}

    // numerics v2.2: every class tree of an iteration gets its own fixed-point grid from the coarse sums Q_g, Q_h of its (g, h) (rgbm_numerics.h).  The
    // gradient kernels leave the sums per workgroup / wave (qpart [parts][K][2]: plain stores, no atomics), k_fx_reduce adds them up into fxq [K][2];
    // k_grad<1> (softmax with K > 112) and RGBM_FX_MEASURE=separate take them from a pass of their own over the (g, h) array (k_fx_measure).  Row-sharded:
    // ONE more integer all-reduce per iteration (2 K words).  k_fx_scale turns the sums into the FxScale table every accumulating / searching kernel reads.
    int grad_gx() const { return (int)std::min<long long>((N + 255) / 256, 4096); }
    bool mc_tile() const { return p.objective == 1 && K >= 16 && K <= 112; }
    bool mc_rows() const { return p.objective == 1 && K < 16; }
    void alloc_fx_parts() {
        if (sw.fx_separate || (p.objective == 1 && !mc_tile() && !mc_rows())) return;
        fx_fused = true; fx_parts = mc_tile() ? (N + 63) / 64 : (mc_rows() ? ((N + 255) / 256) * 4 : (long long)grad_gx());
        qpart.alloc((size_t)fx_parts * K * 2);
    }
    // the gradients of an iteration and the grid they give its class trees; node0 [K][NS]: the level grower's node ids (every training row goes back to the root)
    void enqueue_grad(uint8_t* node0, long long NS);
    void enqueue_bagging();    // the bag of the iterations from this one on
};

// The two ways of growing the K class trees of a boosting iteration.  Each is built from the fit's common state (which it reads, never writes),
// allocates its own buffers and enqueues its set-up; enqueue_iteration(it) follows the gradients of iteration `it`: its trees and the score update.
// The level-synchronous grower (rgbm_level.h): max_depth passes over the rows per iteration, every class tree's open nodes at once.
struct LevelGrower {
    FitState& st; hipStream_t s;
    int root_feats;                         // feature groups the root pass accumulates per row (statistics)
    unsigned long long statrows = 0;        // rows whose (g, h) were accumulated, counted on the device (statistics)
    rg::LevelConst lc, lcj; LevelPassPlan passes;
    const int n_hnodes = (1 << st.p.max_depth) - 1;
    bool use_reduce = false;   // root pass: sum the per-workgroup partials in a separate kernel (many workgroups per class tree, joint bins, or row-sharded)
    // joint bins for the root pass (rgbm_level.h, k_pack_joint): a second record whose bytes hold GROUPS of low-cardinality features
    bool joint_root = false; int vtotbins = 0;
    DevBuf<rg::FeatMeta> vfmeta; DevBuf<rg::ChunkMeta> vcmeta; DevBuf<uint4> rec_j; DevBuf<rg::HistBin> part_j, red_j; DevBuf<rg::JointFeat> jf; DevBuf<int16_t> binfeat;
    DevBuf<uint8_t> node; DevBuf<rg::LvPlan> plan; DevBuf<rg::SNode> snodes;
    // k_level_step: lane map of its packed threshold scan, waves a child needs, whether the two child histograms live in LDS, workgroup size, and the most
    // workgroup partials per class tree it sums itself (more: k_level_reduce runs in front).  Threads and threshold: profiles/EXPERIMENTS.md, round 14.
    DevBuf<rg::ScanLane> scan_map; std::vector<rg::ScanLane> h_scan; int scan_waves = 0; bool step_hist_lds = true;
    int step_threads = 512, step_max_gx = 256;
    DevBuf<rg::HistBin> part, lpool, part_red; DevBuf<int32_t> count, count_g, err, leafnode; DevBuf<double> ndelta; DevBuf<unsigned long long> d_statrows;
    const int score_gx = (int)std::max<long long>(1, std::min<long long>((st.N + 1023) / 1024, (2048 + st.K - 1) / st.K));
    LevelTrace trace;
    int32_t h_err = 0;
    // layout tables of the root pass and of the level passes (the host copies live as long as the uploads may be in flight)
    std::vector<rg::RootLayout> h_root_lay; std::vector<rg::MtLayout> h_mt_lay; std::vector<int> mt_lay_keys;
    DevBuf<rg::RootLayout> root_lay; DevBuf<rg::MtLayout> mt_lay;
    static int mt_lay_key(const MtLaunch& L) { return L.ch * 4 + (L.acc2 ? 2 : 0) + (L.rot ? 1 : 0); }
    int mt_lay_index(const MtLaunch& L) const {
        for (size_t i = 0; i < mt_lay_keys.size(); ++i) if (mt_lay_keys[i] == mt_lay_key(L)) return (int)i;
        return -1;
    }

    explicit LevelGrower(FitState& st_) : st(st_), s(st_.s), root_feats(st_.F), trace(true, st_.K, st_.s) {
        using namespace rg;
        memset(&lc, 0, sizeof(lc)); memset(&lcj, 0, sizeof(lcj));
        lc.lds_bytes = level_lds_bytes(st.sw);
        lc.nchunk = st.h.nchunk; lc.K = st.K; lc.F = st.F; lc.totbins = st.h.tc.totbins;
        lc.num_leaves = st.NL; lc.max_depth = st.p.max_depth; lc.min_data_in_leaf = st.p.min_data_in_leaf; lc.N = st.N; lc.NS = (st.N + 255) & ~255ll; lc.NG = lc.NS;
        lc.sib_local = (st.dp && comm_rank() == 0) ? 1 : 0;
        lc.has_mult = st.tab.has_mult ? 1u : 0u;
        passes = plan_level_passes(st.sw, st.h.fmeta, st.h.cmeta, st.N, st.K, st.p.max_depth, st.tab.has_mult, lc.lds_bytes);
        lc.gx = passes.root_gx; lc.xcd_blocks = 1; lc.max_built = 1;
        node.alloc((size_t)st.K * lc.NS);
        // the padding rows [N, NS) of every class tree stay LV_INACTIVE for the whole fit (the gradient kernels reset rows < N only): the level pass
        // routes rows by their id alone, and an id past the end of a class tree's table takes the dummy entry
        HIPCHK(hipMemsetAsync(node.p, 0xFF, (size_t)st.K * lc.NS, s));
        plan.alloc(st.K); snodes.alloc((size_t)st.K * 256);
        part.alloc(passes.part_items * st.h.tc.totbins); lpool.alloc((size_t)st.K * n_hnodes * st.h.tc.totbins);
        scan_waves = scan_lane_map(st.h.fmeta.data(), st.F, h_scan);
        scan_map.alloc(h_scan.size()); scan_map.upload(h_scan.data(), h_scan.size(), s);
        step_hist_lds = ls_hist_in_lds(st.h.tc.totbins, st.F) && !st.sw.step_readback;
        if (st.sw.step_threads >= 128 && st.sw.step_threads <= LS_MAX_THREADS && st.sw.step_threads % 64 == 0) step_threads = st.sw.step_threads;
        if (st.sw.step_max_gx >= 1) step_max_gx = st.sw.step_max_gx;
        count.alloc((size_t)st.K * 256); use_reduce = st.dp || lc.gx > step_max_gx;
        if (st.dp) count_g.alloc((size_t)st.K * 256);
        const int max_built_all = 1 << std::max(0, st.p.max_depth - 2);
        part_red.alloc((size_t)st.K * max_built_all * st.h.tc.totbins + (size_t)st.K * 128 /* K*256 int64 counts */);
        leafnode.alloc((size_t)st.K * LV_MAX_LEAVES); err.alloc(1); err.zero(s); ndelta.alloc((size_t)st.K * 256); d_statrows.alloc(1); d_statrows.zero(s);
        // Joint bins for the root pass (the tables where the root pass runs at the LDS-atomic rate); RGBM_JOINT_ROOT=0 disables it (same
        // models either way: the sums are exact integers)
        if (st.sw.joint_root && ((long long)st.K * st.N >= (1ll << 21) || (st.tab.has_mult && st.h.nchunk == 2))) {
            const JointRootPlan jp = plan_joint_root(st.h.fmeta, st.h.tc.totbins, st.tab.has_mult, lc.lds_bytes);
            if (jp.on) {
                const int VF = (int)jp.vfm.size();
                joint_root = true; vtotbins = jp.vcm.wide_bins;
                vfmeta.alloc(VF); vfmeta.upload(jp.vfm.data(), VF, s); vcmeta.alloc(1); vcmeta.upload(&jp.vcm, 1, s);
                jf.alloc(st.F); jf.upload(jp.jf.data(), st.F, s); binfeat.alloc(jp.binfeat.size()); binfeat.upload(jp.binfeat.data(), jp.binfeat.size(), s);
                rec_j.alloc((size_t)st.N);
                hipLaunchKernelGGL(k_pack_joint, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, s, st.bins.rec.p, (long long)st.N, st.F, jf.p, rec_j.p, st.tab.has_mult ? st.h.nchunk - 1 : -1);
                part_j.alloc((size_t)st.K * lc.gx * vtotbins); red_j.alloc((size_t)st.K * vtotbins + (size_t)st.K * 128 /* k_level_reduce parks the counts behind the bins */);
                lcj = lc; lcj.nchunk = 1; lcj.F = VF; lcj.totbins = vtotbins; lcj.max_built = 1;
                h_root_lay.resize(1); root_layout_fill(h_root_lay[0], jp.vfm.data(), VF, lc.lds_bytes);
                use_reduce = true; root_feats = VF;
                HIPCHK(hipStreamSynchronize(s));   // jp's vectors are locals
            }
        }
        if (st.tab.has_mult && st.h.nchunk == 2 && !joint_root)
            throw std::invalid_argument("a two-chunk table with row multiplicities needs the joint-bin root pass (its record carries the multiplicity); this feature set does not pack into 15 groups");
        // layout tables (rgbm_level.h, "LAYOUT TABLES"): one per chunk of the root pass, one per (chunk, form) of the level passes
        if (!joint_root) {
            h_root_lay.resize(st.h.nchunk);
            for (int ch = 0; ch < st.h.nchunk; ++ch) root_layout_fill(h_root_lay[ch], st.h.fmeta.data() + st.h.cmeta[ch].first_feat, st.h.cmeta[ch].nfeat, lc.lds_bytes);
        }
        root_lay.alloc(h_root_lay.size()); root_lay.upload(h_root_lay.data(), h_root_lay.size(), s);
        lc.root_lay = root_lay.p; lcj.root_lay = root_lay.p;
        for (int level = 1; level < st.p.max_depth; ++level) for (const auto& L : passes.mt[level]) if (mt_lay_index(L) < 0) {
            const bool acc2 = L.acc2 != 0;
            const ChunkMeta& cm = st.h.cmeta[L.ch];
            const int nf_last = acc2 ? st.h.cmeta[1].nfeat : cm.nfeat;
            const bool li_in_rec = nf_last <= 15 && !st.tab.has_mult;               // (as k_level_mt decides it)
            mt_lay_keys.push_back(mt_lay_key(L)); h_mt_lay.emplace_back();
            mt_layout_fill(h_mt_lay.back(), st.h.fmeta.data() + cm.first_feat, cm.nfeat, acc2 ? st.h.fmeta.data() + st.h.cmeta[1].first_feat : nullptr, acc2 ? st.h.cmeta[1].nfeat : 0,
                           cm.wide_bins, L.rot != 0, mt_hist_bytes(lc.lds_bytes, acc2 ? MT_THREADS_ACC2 : LV_THREADS, acc2, acc2, !li_in_rec));
        }
        if (!h_mt_lay.empty()) { mt_lay.alloc(h_mt_lay.size()); mt_lay.upload(h_mt_lay.data(), h_mt_lay.size(), s); }
        if (st.sw.timing) {
            fprintf(stderr, "[rgbm] root: gx %d joint %d groups %d\n", lc.gx, joint_root ? 1 : 0, joint_root ? lcj.F : 0);
            for (int level = 1; level < st.p.max_depth; ++level) for (const auto& L : passes.mt[level])
                fprintf(stderr, "[rgbm] level %d launch: chunk %d slots %d..%d route %d T %d G %d gx %d acc2 %d rot %d\n", level, L.ch, L.slot0, L.slot0 + L.nslots - 1, L.route, L.T, L.G, L.gx, L.acc2, L.rot);
        }
        rgh::once_per_device(st.tab.device, rgh::ONCE_LEVEL_LDS, [] {      // the level grower's kernels may use the CU's whole LDS
            HIPCHK(hipFuncSetAttribute((const void*)rg::k_level_root, hipFuncAttributeMaxDynamicSharedMemorySize, rg::LV_LDS_BYTES));
            for (const MtForm& f : MT_FORMS) for (int bag = 0; bag < 2; ++bag) for (int route = 0; route < 2; ++route)
                HIPCHK(hipFuncSetAttribute((const void*)mt_kernel(f, bag != 0, route != 0), hipFuncAttributeMaxDynamicSharedMemorySize, rg::LV_LDS_BYTES));
        });
        if (trace.on) trace.buf.alloc(((size_t)st.K * n_hnodes * st.h.tc.totbins * 16 + (size_t)st.K * 256 * (sizeof(SNode) + 4) + (size_t)st.K * sizeof(LvPlan) + 4096) * (size_t)(st.p.max_depth + 1) * (size_t)(trace.hi - trace.lo + 1) + (size_t)st.NE * 64 + 4096);
    }

    void trace_level(int level) {
        trace.copy("count", level, count.p, (size_t)st.K * 256 * 4);
        trace.copy("plan", level, plan.p, (size_t)st.K * sizeof(rg::LvPlan));
        trace.copy("snodes", level, snodes.p, (size_t)st.K * 256 * sizeof(rg::SNode));
        trace.copy("lpool", level, lpool.p, (size_t)st.K * n_hnodes * st.h.tc.totbins * 16);
    }
    // partials of this rank -> compact buffer (-> integer all-reduce when row-sharded); the step kernel then sees ONE partial.  On one rank the step
    // kernel sums up to step_max_gx partials itself (the root: use_reduce, which the joint-bin root pass also sets).
    std::pair<const rg::HistBin*, rg::LevelConst> exchange(bool root, int nb, const rg::LevelConst& lp) {
        using namespace rg;
        if (root ? !use_reduce : (!st.dp && lp.gx <= step_max_gx)) return {part.p, lp};
        if (root && joint_root) {   // partials -> one joint histogram per class tree (k_level_reduce in the joint bin space) -> marginals of the real features
            hipLaunchKernelGGL(k_level_reduce, dim3((vtotbins + 63) / 64, 1, st.K), dim3(256), 0, s, part_j.p, red_j.p, plan.p, count.p, 1, 1, lcj);
            hipLaunchKernelGGL(k_level_marginal, dim3((st.h.tc.totbins + 255) / 256, st.K), dim3(256), 0, s, red_j.p, part_red.p, plan.p, count.p, jf.p, binfeat.p, vtotbins, lc);
        } else
            hipLaunchKernelGGL(k_level_reduce, dim3((st.h.tc.totbins + 63) / 64, nb, st.K), dim3(256), 0, s, part.p, part_red.p, plan.p, count.p, root ? 1 : 0, nb, lp);
        if (st.dp) {
            const size_t nh = (size_t)st.K * nb * st.h.tc.totbins * 2;          // int64 words of histograms, then K*256 child counts
            all_reduce(part_red.p, nh + (size_t)st.K * 256, AR_I64, s);
            hipLaunchKernelGGL(k_counts_unpack, dim3(st.K), dim3(256), 0, s, reinterpret_cast<const long long*>(part_red.p) + nh, count_g.p);
        }
        LevelConst r = lp; r.gx = 1; r.max_built = nb;
        return {part_red.p, r};
    }
    // one boosting iteration of the level grower after the gradients: an iteration-invariant launch sequence
    void enqueue_iteration(int it) {
        using namespace rg;
        const TreeOut to = st.trees.out();
        trace.cur_it = it;
        trace.sum("gh", st.gh.p, (size_t)st.K * st.h.tc.NG * 8);
        hipLaunchKernelGGL(k_level_init, dim3(st.K), dim3(64), 0, s, plan.p, snodes.p, count.p, st.n_in_ptr, (long long)st.h.n_train, st.fxq.p, st.h.tc.fx, st.fxs.p, st.it.p, lc);
        const size_t step_lds = ls_lds_bytes(st.h.tc.totbins, st.F, step_hist_lds);
        int32_t* cntg = st.dp ? count_g.p : count.p;      // child row counts seen by split / leaf-count (global when row-sharded)
        st.timers.timed(true, [&]() {
            if (joint_root)   // the root pass over the joint record: one pair of atomics per feature GROUP and row
                hipLaunchKernelGGL(k_level_root, dim3((unsigned)lc.gx * (unsigned)st.K, 1, 1), dim3(LV_THREADS), lc.lds_bytes, s, rec_j.p, st.gh.p, node.p, plan.p, part_j.p,
                                   vfmeta.p, vcmeta.p, st.fxs.p, lcj);
            else
                hipLaunchKernelGGL(k_level_root, dim3((unsigned)lc.gx * (unsigned)st.K, 1, st.h.nchunk), dim3(LV_THREADS), lc.lds_bytes, s, st.bins.rec.p, st.gh.p, node.p, plan.p, part.p,
                                   st.bins.fmeta.p, st.bins.cmeta.p, st.fxs.p, lc);
        });
        {
            auto ex = exchange(true, 1, lc);
            hipLaunchKernelGGL(k_level_step<true>, dim3(1, st.K), dim3(step_threads), step_lds, s, ex.first, lpool.p, plan.p, snodes.p, cntg, count.p, st.bins.fmeta.p,
                               st.used.p, scan_map.p, scan_waves, step_hist_lds ? 1 : 0, d_statrows.p, st.it.p, n_hnodes, st.fxs.p, st.h.tc, ex.second);
            trace_level(0);
        }
        for (int level = 1; level < st.p.max_depth; ++level) {
            hipLaunchKernelGGL(k_level_plan, dim3(st.K), dim3(64), 0, s, plan.p, snodes.p, st.bins.fmeta.p, level, st.h.tc, lc);
            // the k_level_mt launches of the level; lp describes the partials they write
            LevelConst lp = lc;
            lp.xcd_blocks = 0; lp.gx = passes.mt_gx[level]; lp.max_built = 1 << (level - 1);
            for (const MtLaunch& L : passes.mt[level]) {
                LevelConst l1 = lp;
                l1.mt_T = L.T; l1.mt_G = L.G; l1.mt_ch = L.ch; l1.mt_slot0 = L.slot0; l1.mt_nslots = L.nslots; l1.mt_route = L.route; l1.mt_sparse = st.sw.mt_sparse ? 1 : 0;
                l1.mt_lay = mt_lay.p + mt_lay_index(L);
                const bool acc2 = L.acc2 != 0;
                const MtForm form{acc2 ? 2 : (st.h.nchunk <= 2 ? st.h.nchunk : 0), acc2 ? MT_THREADS_ACC2 : LV_THREADS, acc2, acc2, L.rot != 0};
                st.timers.timed(false, [&]() {
                    launch_level_mt(form, st.use_bagging, L.route != 0, dim3((unsigned)L.G * (unsigned)L.gx), s, st.bins.rec.p, st.gh.p, node.p, st.bag.inbag.p,
                                    plan.p, part.p, count.p, st.bins.fmeta.p, st.bins.cmeta.p, err.p, st.fxs.p, l1);
                });
            }
            auto ex = exchange(false, 1 << (level - 1), lp);
            hipLaunchKernelGGL(k_level_step<false>, dim3(1 << (level - 1), st.K), dim3(step_threads), step_lds, s, ex.first, lpool.p, plan.p, snodes.p,
                               cntg, count.p, st.bins.fmeta.p, st.used.p, scan_map.p, scan_waves, step_hist_lds ? 1 : 0, d_statrows.p, st.it.p, n_hnodes, st.fxs.p, st.h.tc, ex.second);
            trace_level(level);
        }
        // last level: plan -> replay (leaf values never depend on the deepest counts) -> route + count + score in one pass
        hipLaunchKernelGGL(k_level_plan, dim3(st.K), dim3(64), 0, s, plan.p, snodes.p, st.bins.fmeta.p, st.p.max_depth, st.h.tc, lc);
        hipLaunchKernelGGL(k_level_replay, dim3(st.K), dim3(64), 0, s, plan.p, snodes.p, cntg, to, st.init.p, ndelta.p, leafnode.p, st.trees.any.p, err.p, st.it.p, st.h.tc);
        // AddScore: the pass that routes, counts and adds in one
        hipLaunchKernelGGL(k_level_final, dim3(score_gx, st.K), dim3(256), 0, s, st.bins.rec.p, node.p, st.bag.inbag.p, plan.p, to, ndelta.p, st.score.p, count.p, st.it.p, lc);
        if (st.dp) { hipLaunchKernelGGL(k_copy_i32, dim3(st.K), dim3(256), 0, s, count.p, count_g.p, (long long)st.K * 256); all_reduce(count_g.p, (size_t)st.K * 256, AR_I32, s); }
        hipLaunchKernelGGL(k_level_leafcount, dim3(st.K), dim3(LV_MAX_LEAVES), 0, s, plan.p, cntg, leafnode.p, to, st.it.p, st.h.tc);
        trace_level(st.p.max_depth);
        trace.sum("score", st.score.p, (size_t)st.K * st.N * 8); trace.sum("node", node.p, (size_t)st.K * lc.NS);
    }
    // behind the last iteration: what report() needs on the host; report() runs after the stream has drained and raises what the device flagged
    void enqueue_report() { err.download(&h_err, 1, s); d_statrows.download(&statrows, 1, s); }
    void report(int32_t target_col) {
        trace.write(target_col);
        if (h_err & 2) throw std::runtime_error("level grower: a level pass was launched with more built nodes / route entries than its workgroup tables hold (sizing violated)");
        if (h_err) throw std::runtime_error("level grower: a node outside the speculative expansion was selected (expansion bound violated)");
    }
};

// The index-list grower (rgbm_kernels.h): leaf-wise, num_leaves - 1 rounds of hist -> split_find -> tree_step -> partition -> finish_split.
struct LeafwiseGrower {
    FitState& st; hipStream_t s;
    DevBuf<int32_t> idx0, idx1, sorted; DevBuf<rg::HistBin> pool; DevBuf<rg::TreeState> state; DevBuf<rg::Leaf> leaves; DevBuf<rg::Cand> cand; DevBuf<double> upd;
    const long long root_tiles = (st.N + rg::TILE_ROWS - 1) / rg::TILE_ROWS;
    const int hist_gx = (int)std::max<long long>(1, std::min<long long>(root_tiles, (1536 + (long long)st.K * st.h.nchunk - 1) / ((long long)st.K * st.h.nchunk)));
    const int part_gx = (int)std::max<long long>(1, std::min<long long>((st.h.n_train + 1023) / 1024, (1024 + st.K - 1) / st.K));
    const int upd_gx = (int)std::max<long long>(1, std::min<long long>((st.h.n_train + 255) / 256, (2048 + st.K - 1) / st.K));
    const size_t upd_lds = (size_t)(3 * st.NL + (st.NL & 1)) * 4 + (size_t)st.NL * 8;

    explicit LeafwiseGrower(FitState& st_) : st(st_), s(st_.s) {
        idx0.alloc((size_t)st.K * st.h.n_train); idx1.alloc((size_t)st.K * st.h.n_train);
        pool.alloc((size_t)st.K * st.NL * st.h.tc.totbins);
        state.alloc(st.K); leaves.alloc((size_t)st.K * st.NL); cand.alloc((size_t)st.K * 2 * st.F);
        upd.alloc((size_t)st.K * st.NL); sorted.alloc((size_t)st.K * st.NL * 3);
        if (st.h.lds_hist > 64 * 1024)
            rgh::once_per_device(st.tab.device, rgh::ONCE_HIST_LDS, [] { HIPCHK(hipFuncSetAttribute((const void*)rg::k_hist, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); });
        if (st.h.lds_hist > 160 * 1024) throw std::invalid_argument("histogram working set exceeds LDS");
    }
    void enqueue_iteration(int it) {
        using namespace rg;
        const TreeOut to = st.trees.out();
        const uint8_t* usedp = st.used.p + (size_t)it * st.K * st.F;
        hipLaunchKernelGGL(k_init_iter, dim3(st.K), dim3(64), 0, s, state.p, leaves.p, pool.p, to, st.n_in_ptr, it, st.h.tc);
        for (int step = 0; step < st.NL - 1; ++step) {
            st.timers.timed(step == 0, [&]() {
                hipLaunchKernelGGL(k_hist, dim3(hist_gx, st.K, st.h.nchunk), dim3(256), st.h.lds_hist, s, st.bins.rec.p, st.gh.p, idx0.p, idx1.p, st.base.p,
                                   state.p, pool.p, st.bins.fmeta.p, st.bins.cmeta.p, st.fxs.p, st.h.tc);
            });
            hipLaunchKernelGGL(k_split_find, dim3((st.F + 3) / 4, st.K), dim3(256), 0, s, pool.p, state.p, leaves.p, st.bins.fmeta.p, usedp, cand.p, st.fxs.p, st.h.tc);
            hipLaunchKernelGGL(k_tree_step, dim3(st.K), dim3(64), 0, s, state.p, leaves.p, cand.p, pool.p, st.bins.fmeta.p, to, it, st.h.tc);
            hipLaunchKernelGGL(k_partition, dim3(part_gx, st.K), dim3(256), 0, s, reinterpret_cast<const uint8_t*>(st.bins.rec.p), idx0.p, idx1.p, st.base.p, state.p, st.h.tc);
            hipLaunchKernelGGL(k_finish_split, dim3(st.K), dim3(64), 0, s, state.p, leaves.p, to, it, st.h.tc);
        }
        hipLaunchKernelGGL(k_finalize_tree, dim3(st.K), dim3(64), 0, s, state.p, leaves.p, to, st.init.p, upd.p, sorted.p, st.trees.any.p, it, st.h.tc);
        hipLaunchKernelGGL(k_score_update, dim3(upd_gx, st.K), dim3(256), upd_lds, s, state.p, leaves.p, sorted.p, upd.p, idx0.p, idx1.p, st.base.p, st.score.p, st.n_in_ptr, st.h.tc);
        if (st.use_bagging)
            hipLaunchKernelGGL(k_score_update_oob, dim3(upd_gx, st.K), dim3(256), 0, s, reinterpret_cast<const uint8_t*>(st.bins.rec.p), st.bag.oob.p, st.bag.bagcnt.p,
                               state.p, to, st.bins.fmeta.p, upd.p, st.score.p, it, st.h.tc);
    }
};

// ---- what an iteration enqueues before its grower
void FitState::enqueue_grad(uint8_t* node0, long long NS) {
    using namespace rg;
    if (p.objective == 0) hipLaunchKernelGGL(k_grad<0>, dim3(grad_gx()), dim3(256), 0, s, score.p, d_ycol, yv.p, cw.p, sw_rows.p, bag.inbag.p, gh.p, node0, NS, qpart.p, d_mult, h.tc);
    else if (mc_rows())
        hipLaunchKernelGGL(k_grad_mc_rows<256>, dim3((unsigned)((N + 255) / 256)), dim3(256), (size_t)K * 256 * 8, s, score.p, d_ycol, cw.p, sw_rows.p, bag.inbag.p, gh.p, node0, NS, qpart.p, d_mult, h.tc);
    else if (mc_tile())
        hipLaunchKernelGGL(k_grad_mc, dim3((unsigned)((N + 63) / 64)), dim3(256), (size_t)(K * 64 + 320) * 8, s, score.p, d_ycol, cw.p, sw_rows.p, bag.inbag.p, gh.p, node0, NS, qpart.p, d_mult, h.tc);
    else if (p.objective == 1) hipLaunchKernelGGL(k_grad<1>, dim3(grad_gx()), dim3(256), 0, s, score.p, d_ycol, yv.p, cw.p, sw_rows.p, bag.inbag.p, gh.p, node0, NS, (unsigned long long*)nullptr, d_mult, h.tc);
    else hipLaunchKernelGGL(k_grad<2>, dim3(grad_gx()), dim3(256), 0, s, score.p, d_ycol, yv.p, cw.p, sw_rows.p, bag.inbag.p, gh.p, node0, NS, qpart.p, d_mult, h.tc);
    if (fx_fused) {
        const long long total = fx_parts * K * 2;
        const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>(256, (total + 8191) / 8192));
        hipLaunchKernelGGL(k_fx_reduce, dim3(gx), dim3(256), (size_t)K * 2 * 8, s, qpart.p, fx_parts, 2 * K, fxq.p);
    } else {
        const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>(128, (N + 4095) / 4096));
        hipLaunchKernelGGL(k_fx_measure, dim3(gx, K), dim3(256), 0, s, gh.p, (long long)N, (long long)h.tc.NG, h.tc.fx, fxq.p, d_mult);
    }
    if (dp) all_reduce(fxq.p, (size_t)K * 2, AR_I64, s);
    if (!level_mode) hipLaunchKernelGGL(k_fx_scale, dim3(1), dim3(256), 0, s, fxq.p, K, h.tc.fx, fxs.p);      // (level grower: k_level_init does it)
}
void FitState::enqueue_bagging() {
    using namespace rg;
    hipLaunchKernelGGL(k_bagging, dim3((unsigned)((bag.nrb + 63) / 64)), dim3(64), 0, s, bag.rand.p, bag.local, p.bagging_fraction, bag.sorted_rows.p, bag.inbag.p, bag.bagcnt.p,
                       bag.off, (long long)h.n_train);
    hipLaunchKernelGGL(k_bag_lists, dim3((unsigned)((std::max<long long>(bag.local, 1) + 255) / 256)), dim3(256), 0, s, bag.sorted_rows.p, bag.local, bag.inbag.p, base.p, bag.oob.p, bag.bagcnt.p);
    if (dp) {
        hipLaunchKernelGGL(k_copy_i32, dim3(1), dim3(256), 0, s, reinterpret_cast<const int32_t*>(bag.bagcnt.p), reinterpret_cast<int32_t*>(bagcnt_g.p), 2ll);
        all_reduce(bagcnt_g.p, 2, AR_U32, s);
    }
}

rgbm_model* train_core(const rgbm_table& tab, int32_t target_col, const int32_t* feat_cols, int32_t F,
                       const double* y_value, const double* class_weight, const double* sample_weight_host,
                       const HostLabelStats* hls, const rgbm_params& p, rgbm_train_stats* stats, bool view_stats = false) {
    using namespace rg;
    check_fit_args(tab, target_col, feat_cols, F, y_value, p);
    if (F > 65535) throw std::invalid_argument("more than 65535 feature columns");
    StreamGuard sg_; hipStream_t s = sg_.s;
    rgh::Event ev_begin, ev_end;
    HIPCHK(hipEventRecord(ev_begin.e, s));

    FitState st(tab, target_col, F, p, stats != nullptr, s);
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = now();
    // ---- 1. prologue: code frequencies of the training rows -> bins, tables, label statistics (fit_setup) -> bin records
    st.bins.count_codes(tab, target_col, feat_cols, F, st.h, s);
    if (st.dp) {   // the table is one rank's row shard: the counts are summed over the ranks
        if (comm_kind() == 0) throw std::invalid_argument("row-sharded training requested but this thread has no communicator (rgbm_comm_init)");
        all_reduce(st.bins.cnt.p, st.bins.cnt.n, AR_U32, s);
    }
    st.bins.download_counts(st.h, s);
    if (st.dp) stream_sync_watchdog(s); else HIPCHK(hipStreamSynchronize(s));
    fit_setup(tab, y_value, class_weight, hls, p, F, st.h);
    if (p.objective == 2) y_value = st.h.yv32.data();          // LightGBM keeps labels as float32: the dictionary rounded once
    const int n_y = st.h.ncod[F];

    const double t_bins = now();
    st.bins.fill(st.h, st.N, s);
    // rows with multiplicities (rgbm_table_set_row_multiplicity): the multiplicity rides in byte 15 of the row's LAST bin record, so that chunk
    // must leave the byte free; the level grower only (one chunk, or two chunks in one pass), no bagging (LightGBM draws per ORIGINAL row), no per-row weights
    if (tab.has_mult && (!st.level_mode || st.h.nchunk > 2 || (F % 16) == 0 || sample_weight_host || st.use_bagging))
        throw std::invalid_argument("a table with row multiplicities trains with the level grower (1 <= max_depth <= 7), at most 32 features of which the last 16-feature "
                                    "chunk holds at most 15, without bagging and without per-row weights");
    st.bins.pack(tab, s);
    if (st.dp && (!st.level_mode || sample_weight_host))
        throw std::invalid_argument("row-sharded training supports the level grower (1 <= max_depth <= 7) without per-row weights");
    // ---- 2. the state both growers work on, up to the trees; then the grower with its own buffers and set-up
    st.counter.alloc(1); st.counter.zero(s);
    if (!st.level_mode || st.use_bagging) {
        st.base.alloc(st.h.n_train);
        hipLaunchKernelGGL(k_iota_train, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, s, st.d_ycol, (long long)st.N, st.base.p, st.counter.p);
    }
    if (st.level_mode) st.h.tc.NG = (st.N + 255) & ~255ll;            // level grower: every wave tile of a class tree's (g, h) row is in bounds and 32-byte aligned
    st.gh.alloc((size_t)st.K * st.h.tc.NG); st.gh.zero(s);
    st.score.alloc((size_t)st.K * st.N); st.init.alloc(st.K);
    st.init.upload(st.h.init.data(), st.K, s);
    st.fxq.alloc((size_t)st.K * 2); st.fxq.zero(s);
    st.fxs.alloc(st.K);
    hipLaunchKernelGGL(k_init_score, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, s, st.score.p, (long long)st.N, st.K, st.init.p);
    const size_t NT = (size_t)st.NE * st.K;
    st.trees.alloc(NT, st.NL, st.NE, s);
    std::unique_ptr<LevelGrower> lg; std::unique_ptr<LeafwiseGrower> lw;
    if (st.level_mode) lg.reset(new LevelGrower(st)); else lw.reset(new LeafwiseGrower(st));
    // ---- 3. the rest of the common state: weights, feature masks, bagging
    if (class_weight) { st.cw.alloc(n_y); st.cw.upload(class_weight, n_y, s); }
    if (y_value) { st.yv.alloc(n_y); st.yv.upload(y_value, n_y, s); }
    if (sample_weight_host) { st.sw_rows.alloc(st.N); st.sw_rows.upload(sample_weight_host, st.N, s); }

    const std::vector<uint8_t> used = make_used_masks(p, NT, F, st.h.trivial);
    st.used.alloc(used.size()); st.used.upload(used.data(), used.size(), s);

    if (st.use_bagging) {
        st.bag.order_rows(st.d_ycol, st.N, st.h.n_train, s);
        long long bag_off = 0, bag_local = st.h.n_train;
        if (st.dp) {
            // GBDT::Bagging draws per training-row POSITION (ascending row order over the whole table): this rank's rows hold the positions
            // [bag_off, bag_off + bag_local), bag_off = training rows of the ranks before it (one all-reduce of a per-rank count vector)
            unsigned int h_local = 0; st.counter.download(&h_local, 1, s); stream_sync_watchdog(s);
            bag_local = (long long)h_local;
            std::vector<long long> rc((size_t)comm_nranks(), 0); rc[(size_t)comm_rank()] = bag_local;
            DevBuf<long long> d_rc(rc.size()); d_rc.upload(rc.data(), rc.size(), s);
            all_reduce(d_rc.p, rc.size(), AR_I64, s);
            d_rc.download(rc.data(), rc.size(), s); stream_sync_watchdog(s);
            long long tot = 0;
            for (int r = 0; r < comm_nranks(); ++r) { if (r < comm_rank()) bag_off += rc[(size_t)r]; tot += rc[(size_t)r]; }
            if (tot != st.h.n_train) throw std::runtime_error("row-sharded bagging: the ranks' training-row counts do not add up");
            st.bagcnt_g.alloc(2);
        }
        st.bag.seed(p, bag_off, bag_local, s);
        HIPCHK(hipStreamSynchronize(s));
        st.n_in_ptr = st.dp ? st.bagcnt_g.p : st.bag.bagcnt.p;
    }
    st.it.alloc(1); HIPCHK(hipMemsetAsync(st.it.p, 0xFF, sizeof(int32_t), s));      // -1: k_level_init advances it at the start of every iteration
    st.alloc_fx_parts();
    // the distinct-row view: the statistics count the rows the kernels stream, so the view's own training rows are counted once
    unsigned int view_train_rows = 0;
    if (view_stats && stats) {
        hipLaunchKernelGGL(k_count_train, dim3((unsigned)((st.N + 255) / 256)), dim3(256), 0, s, st.d_ycol, (long long)st.N, st.counter.p);
        st.counter.download(&view_train_rows, 1, s);      // (read after the final synchronise; the level grower does not use the counter)
    }

    if (st.sw.timing) HIPCHK(hipStreamSynchronize(s));
    const double t_setup = now();
    // ---- 4. boosting iterations: everything below is enqueue-only.
    // hipGraph replay of an iteration was built and measured twice (rounds 1 and 2, MI355X / ROCm 7.2) and removed: a 10 000-row fit
    // takes the same time either way (the chain of ~30 small dependent kernels per iteration is bound by GPU-side latency, not by
    // the host launches), 24 concurrent host threads gain nothing (8.8 vs 9.2 ms per 60-iteration fit), and captures made while
    // other threads train fail or replay wrongly (20 bad models in 150) even with every graph call behind one mutex.
    for (int it = 0; it < st.NE; ++it) {
        if (st.use_bagging && it % p.bagging_freq == 0) st.enqueue_bagging();
        st.enqueue_grad(lg ? lg->node.p : nullptr, lg ? lg->lc.NS : 0);
        if (lg) lg->enqueue_iteration(it); else lw->enqueue_iteration(it);
    }
    HIPCHK(hipGetLastError());

    const double t_enq = now();
    // ---- 5. trees back to the host
    std::vector<char> host_trees(st.trees.host_bytes());
    const HostTrees ht = st.trees.download(host_trees.data(), s);
    if (lg) lg->enqueue_report();
    HIPCHK(hipEventRecord(ev_end.e, s));
    if (st.dp) stream_sync_watchdog(s); else HIPCHK(hipStreamSynchronize(s));
    if (st.sw.timing) fprintf(stderr, "[rgbm] target %d K=%d: count+bins %.1f ms, alloc+pack %.1f ms, enqueue %.1f ms, drain+download %.1f ms\n", target_col, st.K, t_bins - t_start, t_setup - t_bins, t_enq - t_setup, now() - t_enq);
    if (lg) lg->report(target_col);

    model_from_trees(st.h.model.get(), ht, st.NE, st.K, st.NL);
    if (stats) {
        float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, ev_begin.e, ev_end.e));
        const int nranks = st.dp ? comm_nranks() : 1;
        fill_train_stats(stats, ms, st.timers, ht, p, st.level_mode, st.use_bagging, nranks, st.N, st.h.n_train, F, lg ? lg->root_feats : F, st.K, lg ? lg->statrows : 0);
        if (view_stats && st.level_mode && st.h.n_train > 0) {
            // n_train and the device's counter weigh a row by its multiplicity.  Streamed rows: the root passes exactly (every training row of the
            // view, once per tree); the level passes pro rata (a built child's share of distinct rows is not counted on the device)
            const int64_t root_w = stats->root_rows, level_w = std::max<int64_t>(0, stats->hist_rows - root_w);
            stats->root_rows = root_w > 0 ? (int64_t)st.NE * st.K * (int64_t)view_train_rows : 0;
            stats->hist_rows = stats->root_rows + (int64_t)((double)level_w * (double)view_train_rows / (double)st.h.n_train + 0.5);
            stats->hist_bytes = stats->hist_rows * ((int64_t)F + 8);
        }
    }
    return st.h.model.release();
}


struct PredictScratch;
void predict_device(rgbm_model* m, int device, hipStream_t s, const int32_t* d_codes, long long Ntab, long long row0, long long n,
                    const int32_t* d_feat_cols, double* d_proba, int32_t* d_label, double* d_top, PredictScratch* scratch);

// ---------------------------------------------------------------------------------------------
// The batched small-table trainer (rgbm_small.h): many fits, three launches per boosting iteration for all of them.
// Replaces the loop over fits of python/repair/train.py:158-209 (cross_val_score inside the hyper-parameter search: folds x
// trials) and python/repair/model.py:768-815 on <= 10 000-row samples.  Every fit is an rgbm_table_train call in all but time:
// the models are the same bytes.
// ---------------------------------------------------------------------------------------------
struct SmallFitDev {   // device state of one fit of a batch
    FitHost h; int F = 0, K = 1, NL = 0, NE = 0; bool bag = false;
    BinRecords bins; BagState bagst; TreeBlock trees;
    DevBuf<unsigned int> counter; DevBuf<uint8_t> used;
    DevBuf<float2> gh; DevBuf<double> score, init, upd, cw, yv;
    DevBuf<int32_t> idx0, idx1, base, tree_L; DevBuf<rg::HistBin> pool;
    DevBuf<rg::ScanLane> scan_map; std::vector<rg::ScanLane> h_scan; int scan_waves = 0;
    DevBuf<uint4> vrec; DevBuf<double> vscore, vtop; DevBuf<int32_t> vlabel; DevBuf<uint8_t> vlut, vmiss; std::vector<uint8_t> h_vlut, h_vmiss; long long n_valid = 0;
    std::vector<char> host_trees;          // the harvest, when the page-locked block is not to be had
    std::vector<uint8_t> h_used;           // host source of an asynchronous upload: alive until the batch has drained
};

// validation rows of a fit that trained outside the fused kernels: the predictor on its model (same labels / values)
void score_valid_with_model(const rgbm_fit_spec& sp, rgbm_model* m) {
    if (!sp.valid_table || !m || sp.valid_table->n <= 0 || (!sp.valid_label_out && !sp.valid_value_out)) return;
    const rgbm_table& vt = *sp.valid_table;
    StreamGuard sg_; hipStream_t s = sg_.s;
    DevBuf<int32_t> d_fc(sp.n_features), d_lab(vt.n); DevBuf<double> d_top(vt.n);
    d_fc.upload(sp.feat_cols, sp.n_features, s);
    predict_device(m, vt.device, s, vt.codes.p, vt.n, 0, vt.n, d_fc.p, nullptr, d_lab.p, d_top.p, nullptr);
    if (sp.valid_label_out) d_lab.download(sp.valid_label_out, vt.n, s);
    if (sp.valid_value_out) d_top.download(sp.valid_value_out, vt.n, s);
    HIPCHK(hipStreamSynchronize(s));
}

bool small_fit_eligible(const rgbm_table& tab, int32_t F, const rgbm_params& p, long long small_rows) {
    if (tab.n > small_rows || tab.n >= (1ll << 31) - 4096) return false;
    if (tab.has_mult) return false;      // (rows with multiplicities: the level grower of the single-fit trainer)
    if (p.num_leaves > rg::SM_MAX_LEAVES || F > rg::SM_MAX_FEATS) return false;
    if (p.reserved & RGBM_FLAG_ROW_SHARDED) return false;
    return true;
}

// status[i] = RGBM_OK or the error code of fit i (its message is the thread's last error when exactly one fit fails; the Python
// binding raises per fit).  Fits the fused kernel does not cover (large tables, > 256 leaves) run through train_core one by one.
// page-locked host block for the tree harvest of a batch of fits (see phase E of train_batch_small)
struct HarvestArena {
    std::mutex mu; void* p = nullptr; size_t cap = 0; int device = -1;
    static constexpr size_t KEEP_MAX = (size_t)1 << 30;
    // a block of at least `bytes` (null: not available -- the caller falls back to pageable memory)
    void* get(size_t bytes, int dev) {
        if (bytes == 0 || bytes > KEEP_MAX || getenv("RGBM_NO_PIN") != nullptr) return nullptr;
        if (p && cap >= bytes && device == dev) return p;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = std::min(KEEP_MAX, bytes + bytes / 4);
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return nullptr; }
        cap = want; device = dev;
        return p;
    }
};
HarvestArena& harvest_arena() { static HarvestArena* a = new HarvestArena(); return *a; }

// What the last rgbm_table_train_batch call of this thread did with each fit (rgbm_table_train_batch_report): {route, scan_waves, nchunk,
// lds_bytes}; the last three describe the fused kernels' launch of a route-1 fit (route 4: the LDS bytes that were too many) and are 0 otherwise.
enum { ROUTE_NONE = 0, ROUTE_FUSED = 1, ROUTE_SINGLE_INELIGIBLE = 2, ROUTE_SINGLE_ALONE = 3, ROUTE_SINGLE_LDS = 4 };
struct BatchReportRow { int32_t route, scan_waves, nchunk, lds_bytes; };
std::vector<BatchReportRow>& batch_report() { static thread_local std::vector<BatchReportRow> r; return r; }

void train_batch_small(const rgbm_fit_spec* specs, int32_t n_fits, rgbm_model** out, int32_t* status) {
    using namespace rg;
    std::vector<BatchReportRow>& report = batch_report();
    report.assign((size_t)n_fits, BatchReportRow{ROUTE_NONE, 0, 0, 0});
    long long small_rows = 65536;
    if (const char* e = getenv("RGBM_SMALL_ROWS")) small_rows = atoll(e);
    const int device = specs[0].table->device;
    std::vector<int> batch;                                           // fits that go through the fused kernels
    auto record_error = [&](int i, const std::exception& e) { status[i] = rgh::status_of(e); rgh::last_error() = e.what(); };
    auto run_single = [&](int i, int route) {
        const rgbm_fit_spec& sp = specs[i];
        report[i].route = route;
        try {
            out[i] = train_core(*sp.table, sp.target_col, sp.feat_cols, sp.n_features, sp.y_value, sp.class_weight, nullptr, nullptr, *sp.params, nullptr); status[i] = RGBM_OK;
            score_valid_with_model(sp, out[i]);
        }
        catch (const std::exception& e) { record_error(i, e); }
    };
    for (int i = 0; i < n_fits; ++i) {
        out[i] = nullptr; status[i] = RGBM_OK;
        const rgbm_fit_spec& sp = specs[i];
        if (!sp.table || !sp.feat_cols || !sp.params) { status[i] = RGBM_ERR_ARG; rgh::last_error() = "rgbm_table_train_batch: bad fit spec"; continue; }
        if (sp.table->device != device) throw std::invalid_argument("rgbm_table_train_batch: all tables of a batch must live on one device");
        if (small_fit_eligible(*sp.table, sp.n_features, *sp.params, small_rows)) batch.push_back(i); else run_single(i, ROUTE_SINGLE_INELIGIBLE);
    }
    if (batch.empty()) return;
    if (batch.size() == 1 && !getenv("RGBM_SMALL_ALWAYS")) { run_single(batch[0], ROUTE_SINGLE_ALONE); return; }    // one fit: the level grower's kernel chain is faster than one workgroup per class tree

    StreamGuard sg_; hipStream_t s = sg_.s;
    const bool timing = getenv("RGBM_TIMING") != nullptr;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = now();
    std::vector<std::unique_ptr<SmallFitDev>> dev(n_fits);
    // ---- A. argument checks + code frequencies of every fit's training rows (one launch per fit, ONE synchronisation for all)
    std::vector<int> live;
    for (int i : batch) {
        const rgbm_fit_spec& sp = specs[i]; const rgbm_table& tab = *sp.table; const rgbm_params& p = *sp.params; const int F = sp.n_features;
        try { check_fit_args(tab, sp.target_col, sp.feat_cols, F, sp.y_value, p); }
        catch (const std::exception& e) { record_error(i, e); continue; }
        dev[i].reset(new SmallFitDev());
        SmallFitDev& d = *dev[i];
        d.F = F; d.K = p.objective == 1 ? p.num_class : 1; d.NL = p.num_leaves; d.NE = p.n_estimators;
        d.bins.count_codes(tab, sp.target_col, sp.feat_cols, F, d.h, s); d.bins.download_counts(d.h, s);
        live.push_back(i);
    }
    HIPCHK(hipStreamSynchronize(s));
    // ---- B. per fit: bins, tables, records, state
    std::vector<int> ok;
    int NE_max = 0; size_t lds_max = 0; long long N_max = 1, ntrain_max = 1, nrb_max = 1, nvalid_max = 0; bool any_bag = false;
    for (int i : live) {
        const rgbm_fit_spec& sp = specs[i]; const rgbm_table& tab = *sp.table; const rgbm_params& p = *sp.params;
        SmallFitDev& d = *dev[i]; FitHost& h = d.h; const int F = d.F, K = d.K, NL = d.NL, NE = d.NE; const long long N = tab.n;
        // one failing fit does not fail the batch: whatever this fit's set-up throws (arguments, labels, HIP) is ITS status; uploads queued from
        // its host vectors are drained before they are destroyed
        try {
        fit_setup(tab, sp.y_value, sp.class_weight, nullptr, p, F, h);
        // lane map of the packed threshold scan (rgbm_small.h): a lane owns 4 bins of one feature, a feature does not straddle waves;
        // used when a child's features fit half of the workgroup's waves (both children are scanned at once) and the two compact
        // histograms fit next to the rest in LDS -- otherwise one wave per feature (split_find_body)
        {
            std::vector<ScanLane> sm;
            const int Wn = scan_lane_map(h.fmeta.data(), F, sm);
            const bool off_switch = getenv("RGBM_SMALL_PACKED") && atoi(getenv("RGBM_SMALL_PACKED")) == 0;
            if (!off_switch && 2 * Wn <= SM_WAVES && h.tc.totbins <= 2048 && sm_lds_bytes(h.lds_hist, NL, F, h.tc.totbins) <= 150 * 1024) { d.scan_waves = Wn; d.h_scan = std::move(sm); }
        }
        const size_t lds = sm_lds_bytes(h.lds_hist, NL, F, d.scan_waves > 0 ? h.tc.totbins : 0);
        if (lds > 160 * 1024 - 2048) { dev[i].reset(); run_single(i, ROUTE_SINGLE_LDS); report[i].lds_bytes = (int32_t)lds; continue; }          // (histogram working set of one chunk + leaves exceed the LDS)
        const int nchunk = h.nchunk; const long long n_train = h.n_train;
        d.bins.fill(h, N, s);
        d.bins.pack(tab, s);
        const int32_t* d_ycol = tab.codes.p + (long long)sp.target_col * N;
        d.bag = p.bagging_freq > 0 && p.bagging_fraction < 1.0;
        d.counter.alloc(1); d.counter.zero(s);
        d.base.alloc(n_train);
        hipLaunchKernelGGL(k_iota_train, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, d_ycol, N, d.base.p, d.counter.p);
        d.gh.alloc((size_t)K * N); d.gh.zero(s);
        d.score.alloc((size_t)K * N); d.init.alloc(K); d.init.upload(h.init.data(), K, s);
        hipLaunchKernelGGL(k_init_score, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, d.score.p, N, K, d.init.p);
        d.idx0.alloc((size_t)K * n_train); d.idx1.alloc((size_t)K * n_train);
        d.pool.alloc((size_t)K * NL * h.tc.totbins); d.upd.alloc((size_t)K * NL); d.tree_L.alloc(K);
        const size_t NT = (size_t)NE * K;
        d.trees.alloc(NT, NL, NE, s);
        const int n_y = h.ncod[F];
        if (sp.class_weight) { d.cw.alloc(n_y); d.cw.upload(sp.class_weight, n_y, s); }
        if (p.objective == 2) { d.yv.alloc(n_y); d.yv.upload(h.yv32.data(), n_y, s); }
        if (d.scan_waves > 0) { d.scan_map.alloc(d.h_scan.size()); d.scan_map.upload(d.h_scan.data(), d.h_scan.size(), s); }
        if (sp.valid_table && sp.valid_table->n > 0 && (sp.valid_label_out || sp.valid_value_out)) {
            // the validation rows' bin records, in the predictor's convention: a NULL cell, a code outside the dictionary and a category
            // no training row held (Feat::unseen) are MISSING = bin 255 (device_model's lookup table)
            const rgbm_table& vt = *sp.valid_table;
            if (vt.c != tab.c) throw std::invalid_argument("rgbm_table_train_batch: valid_table must have the columns of the training table");
            d.n_valid = vt.n;
            d.h_vlut.assign(std::max<size_t>(h.lut.size(), 1), 0); d.h_vmiss.assign(F, 255);
            for (int f = 0; f < F; ++f) {
                const Feat& ft = h.model->feats[f]; int b = 0;
                for (int cde = 0; cde < h.ncod[f]; ++cde) { while (b < ft.V - 1 && cde > ft.ub[b]) ++b; d.h_vlut[h.lut_off[f] + cde] = ft.is_unseen(cde) ? (uint8_t)255 : (uint8_t)(ft.V > 0 ? b : 0); }
            }
            d.vlut.alloc(d.h_vlut.size()); d.vlut.upload(d.h_vlut.data(), d.h_vlut.size(), s); d.vmiss.alloc(F); d.vmiss.upload(d.h_vmiss.data(), F, s);
            d.vrec.alloc((size_t)nchunk * vt.n);
            d.bins.pack(vt, d.vlut.p, d.vmiss.p, d.vrec.p, nullptr, s);
            d.vscore.alloc((size_t)K * vt.n); d.vlabel.alloc(vt.n); d.vtop.alloc(vt.n);
            hipLaunchKernelGGL(k_init_score, dim3((unsigned)((vt.n + 255) / 256)), dim3(256), 0, s, d.vscore.p, (long long)vt.n, K, d.init.p);
            nvalid_max = std::max<long long>(nvalid_max, vt.n);
        }
        d.h_used = make_used_masks(p, NT, F, h.trivial);
        d.used.alloc(d.h_used.size()); d.used.upload(d.h_used.data(), d.h_used.size(), s);
        if (d.bag) {
            d.bagst.order_rows(d_ycol, N, n_train, s);
            d.bagst.seed(p, 0, n_train, s);
            any_bag = true; nrb_max = std::max(nrb_max, d.bagst.nrb);
        }
        NE_max = std::max(NE_max, NE); lds_max = std::max(lds_max, lds); N_max = std::max(N_max, N); ntrain_max = std::max(ntrain_max, n_train);
        ok.push_back(i);
        report[i] = BatchReportRow{ROUTE_FUSED, d.scan_waves, nchunk, (int32_t)lds};
        }
        catch (const std::exception& e) { (void)hipStreamSynchronize(s); record_error(i, e); dev[i].reset(); continue; }
    }
    if (ok.empty()) return;
    if (timing) HIPCHK(hipStreamSynchronize(s));
    const double t_setup = now();
    // ---- C. descriptors
    std::vector<SmallFit> fits(ok.size()); std::vector<int32_t> tree2fit;
    for (size_t j = 0; j < ok.size(); ++j) {
        const int i = ok[j]; const rgbm_fit_spec& sp = specs[i]; const rgbm_params& p = *sp.params; SmallFitDev& d = *dev[i]; FitHost& h = d.h;
        SmallFit& f = fits[j]; memset(&f, 0, sizeof(f));
        f.c = h.tc; f.rec = d.bins.rec.p; f.ycol = sp.table->codes.p + (long long)sp.target_col * sp.table->n; f.gh = d.gh.p; f.score = d.score.p;
        f.idx0 = d.idx0.p; f.idx1 = d.idx1.p; f.base_idx = d.base.p; f.pool = d.pool.p; f.fmeta = d.bins.fmeta.p; f.cmeta = d.bins.cmeta.p; f.used = d.used.p;
        f.out = d.trees.out();
        f.init = d.init.p; f.upd = d.upd.p; f.tree_L = d.tree_L.p; f.any_split = d.trees.any.p;
        f.class_w = sp.class_weight ? d.cw.p : nullptr; f.y_value = p.objective == 2 ? d.yv.p : nullptr;
        f.rand_state = d.bagst.rand.p; f.sorted_rows = d.bagst.sorted_rows.p; f.inbag = d.bagst.inbag.p; f.bagcnt = d.bagst.bagcnt.p; f.oob = d.bagst.oob.p;
        f.bag_fraction = p.bagging_fraction; f.bag_nrb = d.bagst.nrb; f.bag_freq = d.bag ? p.bagging_freq : 0;
        f.tree0 = (int32_t)tree2fit.size(); f.n_estimators = d.NE; f.lds_hist = (unsigned long long)h.lds_hist;
        f.scan_map = d.scan_map.p; f.scan_waves = d.scan_waves;
        f.vrec = d.vrec.p; f.vscore = d.vscore.p; f.n_valid = d.n_valid;
        for (int k = 0; k < d.K; ++k) tree2fit.push_back((int32_t)j);
    }
    DevBuf<unsigned long long> d_prof(8); d_prof.zero(s);
    for (auto& f : fits) f.prof = d_prof.p;
    DevBuf<SmallFit> d_fits(fits.size()); DevBuf<int32_t> d_t2f(tree2fit.size());
    d_fits.upload(fits.data(), fits.size(), s); d_t2f.upload(tree2fit.data(), tree2fit.size(), s);
    rgh::once_per_device(device, rgh::ONCE_SMALL_TREE_LDS, [] { HIPCHK(hipFuncSetAttribute((const void*)k_small_tree, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048)); });
    if (lds_max > 160 * 1024 - 2048) throw std::invalid_argument("small-table batch: histogram working set exceeds LDS");
    // ---- D. the boosting iterations of the whole batch: enqueue only
    const unsigned nf = (unsigned)fits.size(), KT = (unsigned)tree2fit.size();
    const unsigned gx_rows = (unsigned)std::min<long long>((N_max + 255) / 256, 64), gx_train = (unsigned)std::min<long long>((ntrain_max + 255) / 256, 64);
    for (int it = 0; it < NE_max; ++it) {
        if (any_bag) {
            hipLaunchKernelGGL(k_small_bagging, dim3((unsigned)((nrb_max + 63) / 64), nf), dim3(64), 0, s, d_fits.p, it);
            hipLaunchKernelGGL(k_small_bag_lists, dim3(gx_train, nf), dim3(256), 0, s, d_fits.p, it);
        }
        hipLaunchKernelGGL(k_small_grad, dim3(gx_rows, nf), dim3(256), 0, s, d_fits.p, it);
        hipLaunchKernelGGL(k_small_tree, dim3(KT), dim3(SM_THREADS), lds_max, s, d_fits.p, d_t2f.p, it);
        if (any_bag) hipLaunchKernelGGL(k_small_oob, dim3(gx_train, KT), dim3(256), 0, s, d_fits.p, d_t2f.p, it);
        if (nvalid_max > 0) hipLaunchKernelGGL(k_small_valid, dim3((unsigned)std::min<long long>((nvalid_max + 255) / 256, 64), KT), dim3(256), 0, s, d_fits.p, d_t2f.p, it);
    }
    for (int i : ok) {   // ConvertOutput + arg-max of the validation rows (what model.predict returns for them)
        SmallFitDev& d = *dev[i]; const rgbm_fit_spec& sp = specs[i];
        if (d.n_valid <= 0) continue;
        hipLaunchKernelGGL(k_softmax_argmax, dim3((unsigned)((d.n_valid + 255) / 256)), dim3(256), 0, s, d.vscore.p, d.n_valid, sp.params->objective,
                           d.h.model->num_class, (double*)nullptr, d.vlabel.p, d.vtop.p);
        if (sp.valid_label_out) d.vlabel.download(sp.valid_label_out, d.n_valid, s);
        if (sp.valid_value_out) d.vtop.download(sp.valid_value_out, d.n_valid, s);
    }
    HIPCHK(hipGetLastError());
    const double t_enq = now();
    if (timing) HIPCHK(hipStreamSynchronize(s));
    const double t_iter = now();
    // ---- E. trees back to the host, one model per fit
    std::vector<int> want;                                            // fits whose model is wanted (a CV fold is wanted for its scores only)
    for (int i : ok) if (!((specs[i].params->reserved & RGBM_FLAG_NO_MODEL) && dev[i]->n_valid > 0)) want.push_back(i);
    // The trees of a batch are tens of MB (72 000 trees, 87 MB for the 16 fits of the 10M x 16 job): into fresh pageable vectors that
    // was zero-filling + page faults + 160 staged copies = most of 69 ms.  They land in ONE page-locked block kept for the life of the
    // process (grown on demand, at most 1 GiB kept; a second batch running at the same time uses pageable vectors).
    std::vector<HostTrees> hts(n_fits);
    HarvestArena& HA = harvest_arena();
    std::unique_lock<std::mutex> ha_lock(HA.mu, std::try_to_lock);
    size_t need = 0;
    for (int i : want) need += dev[i]->trees.host_bytes();
    char* base = ha_lock.owns_lock() ? (char*)HA.get(need, device) : nullptr;
    for (int i : want) {
        SmallFitDev& d = *dev[i];
        const size_t bytes = d.trees.host_bytes();
        if (base) { hts[i] = d.trees.download(base, s); base += bytes; }
        else { d.host_trees.resize(bytes); hts[i] = d.trees.download(d.host_trees.data(), s); }
    }
    HIPCHK(hipStreamSynchronize(s));
    const double t_down = now();
    {   // the tree lists of the models: host work proportional to fits x iterations x class trees, spread over a few threads
        struct Item { int fit; size_t t0, t1; };
        std::vector<Item> items;
        for (int i : want) {
            SmallFitDev& d = *dev[i];
            const size_t n = model_trees_begin(d.h.model.get(), hts[i], d.NE, d.K);
            for (size_t t0 = 0; t0 < n; t0 += 512) items.push_back(Item{i, t0, std::min(n, t0 + 512)});
        }
        std::atomic<size_t> next{0};
        auto work = [&]() {
            for (size_t j = next.fetch_add(1); j < items.size(); j = next.fetch_add(1))
                model_trees_fill(dev[items[j].fit]->h.model.get(), hts[items[j].fit], dev[items[j].fit]->NL, items[j].t0, items[j].t1);
        };
        const size_t nth = std::min<size_t>(std::min<size_t>(std::max<size_t>(items.size(), 1), 32), std::max(1u, std::thread::hardware_concurrency()));
        std::vector<std::thread> th;
        for (size_t q = 1; q < nth; ++q) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    for (int i : ok) status[i] = RGBM_OK;
    for (int i : want) out[i] = dev[i]->h.model.release();
#if defined(SM_PROF)
    { unsigned long long hp[8]; d_prof.download(hp, 8, s); HIPCHK(hipStreamSynchronize(s)); unsigned long long tot = 0; for (int q = 0; q < 8; ++q) tot += hp[q];
      fprintf(stderr, "[rgbm] k_small_tree phases (%% of thread-0 cycles): zero %.1f | accumulate %.1f | flush %.1f | split_find %.1f | reduce+pick %.1f | partition %.1f | finish %.1f | score %.1f\n",
              100.0 * hp[0] / tot, 100.0 * hp[1] / tot, 100.0 * hp[2] / tot, 100.0 * hp[3] / tot, 100.0 * hp[4] / tot, 100.0 * hp[5] / tot, 100.0 * hp[6] / tot, 100.0 * hp[7] / tot); }
#endif
    if (timing) fprintf(stderr, "[rgbm] batch of %zu fits, %u class trees, %d iterations: setup %.1f ms, enqueue %.1f ms, iterations drained after %.1f ms, download %.1f ms (%s), models %.1f ms\n",
                        ok.size(), KT, NE_max, t_setup - t_start, t_enq - t_setup, t_iter - t_setup, t_down - t_iter, ha_lock.owns_lock() ? "page-locked block" : "pageable", now() - t_down);
}

// ---------------------------------------------------------------------------------------------
// Predictor mirror
// ---------------------------------------------------------------------------------------------
// run `fn(t0, t1)` over [0, n) in ranges, on a few host threads when there is enough of it (the table builders below: a
// 19 200-tree model is ~20 ms of host work on one thread)
template <class Fn> void parallel_ranges(size_t n, size_t min_per_thread, Fn fn) {
    const size_t nth = std::min<size_t>(std::min<size_t>(8, std::max<size_t>(1, n / std::max<size_t>(min_per_thread, 1))), std::max(1u, std::thread::hardware_concurrency()));
    if (nth <= 1) { fn((size_t)0, n); return; }
    std::exception_ptr err; std::mutex emu; std::vector<std::thread> th;
    for (size_t q = 0; q < nth; ++q)
        th.emplace_back([&, q]() { try { fn(n * q / nth, n * (q + 1) / nth); } catch (...) { std::lock_guard<std::mutex> lk(emu); if (!err) err = std::current_exception(); } });
    for (auto& t : th) t.join();
    if (err) std::rethrow_exception(err);
}

// the index-linked node tables of the tree walk (k_predict_raw): built only for models the bit-vector scorer cannot take, or when
// a test asks for the walk (the caller holds m->mu)
void build_walk_tables(rgbm_model* m, DeviceModel* dm, hipStream_t s) {
    using namespace rg;
    if (dm->nodes.p) return;
    int maxL = 2;
    for (auto& t : m->trees) maxL = std::max(maxL, t.L);
    dm->node_stride = maxL - 1; dm->leaf_stride = maxL;
    const size_t NT = m->trees.size();
    std::vector<PNode> nodes(std::max<size_t>(NT, 1) * dm->node_stride); std::vector<double> lv(std::max<size_t>(NT, 1) * dm->leaf_stride, 0.0);
    parallel_ranges(NT, 2048, [&](size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; ++t) {
            const Tree& tr = m->trees[t];
            PNode* nd = nodes.data() + t * dm->node_stride;
            if (tr.L <= 1) { nd[0].w0 = 0; nd[0].w1 = 0xFFFFFFFFu; /* both children = ~0 */ }
            for (int j = 0; j < tr.L - 1; ++j) {
                nd[j].w0 = (uint32_t)(tr.feat[j] & 0xFFFF) | ((uint32_t)(tr.theta[j] + 1) & 0x1FF) << 16 | (uint32_t)(tr.dleft[j] ? 1 : 0) << 25;
                nd[j].w1 = ((uint32_t)tr.left[j] & 0xFFFFu) | ((uint32_t)tr.right[j] & 0xFFFFu) << 16;
            }
            for (int l = 0; l < tr.L; ++l) lv[t * dm->leaf_stride + l] = tr.leaf_value[l];
        }
    });
    dm->nodes.alloc(nodes.size()); dm->nodes.upload(nodes.data(), nodes.size(), s);
    dm->leaf_value.alloc(lv.size()); dm->leaf_value.upload(lv.data(), lv.size(), s);
    HIPCHK(hipStreamSynchronize(s));     // the vectors are locals
}

// Which kernel scores a model, as a function of the model alone (and of the two test switches): the ONE copy of the rule.
//   fixed    k_predict_qs<MW, FMAX, TW, TBN>: the model's S mask entries (per feature its value bins + the missing entry) and the
//            all-ones pad entry fit a compile-time stride, S * MW + MW <= TW (the first such row of the table below)
//   dynamic  k_predict_qs<MW, FMAX, 0, 0>: any larger table, with as many trees per stage (8 at most) as fit 48 KB of LDS twice
//   walk     k_predict_raw: more than 64 leaves in a tree, more than 32 features, no trees, or not even one tree per stage fits
// RGBM_QS_FIXED=0 skips the fixed variants and RGBM_PREDICTOR=walk forces the walk (tests).
enum { FORM_FIXED = 0, FORM_DYNAMIC = 1, FORM_WALK = 2 };
struct PredictForm { int form, mw, tw, tb; size_t lds; };
PredictForm predict_form(const rgbm_model* m) {
    PredictForm pf{FORM_WALK, 0, 0, 0, 0};
    const char* pe = getenv("RGBM_PREDICTOR");
    if (pe && strcmp(pe, "walk") == 0) return pf;
    int maxLeaves = 1;
    for (const Tree& tr : m->trees) maxLeaves = std::max(maxLeaves, tr.L);
    const int F = m->F;
    if (maxLeaves > 64 || F > 32 || m->trees.empty()) return pf;
    const int MW = maxLeaves <= 32 ? 1 : 2;
    int S = 0;
    for (const Feat& f : m->feats) S += std::max(f.V, 1) + 1;
    const int words = S * MW;
    int tb = 8, tw = 0;        // trees per LDS stage; padded mask words per tree (0: the dynamic-stride kernel)
    // compile-time strides (k_predict_qs<., ., TW, TBN>) for the table sizes that occur: the tree's offset rides in the ds_read
    struct Fix { int mw, fmax, tw, tbn; };
    static const Fix fixes[] = {{1, 16, 256, 8}, {1, 16, 512, 8}, {1, 32, 512, 8}, {1, 32, 1024, 4}, {2, 16, 512, 8}, {2, 16, 1024, 4}, {2, 32, 1024, 4}, {2, 32, 2048, 2}};
    const char* qf = getenv("RGBM_QS_FIXED");
    const bool no_fix = qf && atoi(qf) == 0;
    for (const Fix& fx : fixes)
        if (!no_fix && fx.mw == MW && fx.fmax == (F <= 16 ? 16 : 32) && words + MW <= fx.tw) { tw = fx.tw; tb = fx.tbn; break; }   // (+ one all-ones pad entry)
    const size_t per_tree = (size_t)(tw ? tw : words) * 4 + (size_t)32 * MW * 8 + 4;
    if (!tw) while (tb > 1 && 2 * tb * per_tree + 16 > 48 * 1024) --tb;
    if (2 * tb * per_tree + 16 > 48 * 1024) return pf;
    return PredictForm{tw ? FORM_FIXED : FORM_DYNAMIC, MW, tw, tb, 2 * tb * per_tree + 16};
}

DeviceModel* device_model(rgbm_model* m, int device, hipStream_t s) {
    std::lock_guard<std::mutex> lk(m->mu);
    auto it = m->dev.find(device);
    if (it != m->dev.end()) return it->second;
    using namespace rg;
    auto dm = new DeviceModel();
    std::unique_ptr<DeviceModel> guard(dm);
    const size_t NT = m->trees.size();
    const int F = m->F;
    std::vector<long long> lut_off(F + 1, 0); std::vector<int32_t> ncod(F), ident(F); std::vector<uint8_t> miss(F, 255);
    for (int f = 0; f < F; ++f) { ncod[f] = m->feats[f].n_codes; ident[f] = f; lut_off[f + 1] = lut_off[f] + std::max(ncod[f], 1); }
    std::vector<uint8_t> lut(lut_off[F]);
    for (int f = 0; f < F; ++f) {
        const Feat& ft = m->feats[f]; int b = 0;
        for (int c = 0; c < ncod[f]; ++c) { while (b < ft.V - 1 && c > ft.ub[b]) ++b; lut[lut_off[f] + c] = ft.is_unseen(c) ? (uint8_t)255 : (uint8_t)(ft.V > 0 ? b : 0); }
    }
    // the bit-vector scoring tables (k_predict_qs) when no tree has more than 64 leaves and the model has at most 32 features
    {
        int maxLeaves = 1;
        for (const Tree& tr : m->trees) maxLeaves = std::max(maxLeaves, tr.L);
        const int F_ = m->F;
        if (maxLeaves <= 64 && F_ <= 32 && NT > 0) {
            const int MW = maxLeaves <= 32 ? 1 : 2, LP = 32 * MW;
            std::vector<int32_t> foff(F_ + 1, 0);
            for (int f = 0; f < F_; ++f) foff[f + 1] = foff[f] + std::max(m->feats[f].V, 1) + 1;       // value bins + the missing entry
            const int S = foff[F_];
            // (uninitialised blocks, filled by the thread that owns the range: a 20 MB vector constructor is 5 ms of page faults on one thread)
            const size_t mk_n = (size_t)NT * S * MW, lv2_n = (size_t)NT * LP;
            std::unique_ptr<uint32_t[]> mk_(new uint32_t[mk_n]); std::unique_ptr<double[]> lv2_(new double[lv2_n]);
            uint32_t* const mk = mk_.get(); double* const lv2 = lv2_.get();
            std::vector<uint32_t> usedf(NT, 0u);
            parallel_ranges(NT, 2048, [&](size_t tr0, size_t tr1) {
            memset(mk + tr0 * S * MW, 0xFF, (tr1 - tr0) * S * MW * sizeof(uint32_t));
            std::fill(lv2 + tr0 * LP, lv2 + tr1 * LP, 0.0);
            std::vector<int> lo, mid;                                // per internal node: in-order ids [lo, mid) of the leaves of its left subtree
            std::vector<std::pair<int, int>> st;
            for (size_t t = tr0; t < tr1; ++t) {
                const Tree& tr = m->trees[t];
                uint32_t* tm = mk + t * S * MW; double* tl = lv2 + t * LP;
                if (tr.L <= 1) { tl[0] = tr.leaf_value ? tr.leaf_value[0] : 0.0; continue; }
                lo.assign(tr.L - 1, 0); mid.assign(tr.L - 1, 0);
                // iterative in-order traversal: (ref, state) with state 0 = enter, 1 = left subtree done
                int next_leaf = 0;
                st.clear(); st.emplace_back(0, 0);
                while (!st.empty()) {
                    auto& top = st.back();
                    const int ref = top.first;
                    if (ref < 0) { tl[next_leaf++] = tr.leaf_value[~ref]; st.pop_back(); continue; }
                    if (top.second == 0) { top.second = 1; lo[ref] = next_leaf; st.emplace_back(tr.left[ref], 0); }
                    else { mid[ref] = next_leaf; const int r = tr.right[ref]; st.pop_back(); st.emplace_back(r, 0); }
                }
                for (int j = 0; j < tr.L - 1; ++j) {
                    // mask of node j: zeros for the leaves of its left subtree
                    uint32_t w[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
                    for (int b = lo[j]; b < mid[j]; ++b) w[b >> 5] &= ~(1u << (b & 31));
                    const int f = tr.feat[j], nb = foff[f + 1] - foff[f] - 1;
                    usedf[t] |= 1u << f;
                    // the test of node j is FALSE (the row goes right) for bins above its threshold, and for a missing value unless it defaults left
                    for (int b = std::max(tr.theta[j] + 1, 0); b < nb; ++b) for (int q = 0; q < MW; ++q) tm[(size_t)(foff[f] + b) * MW + q] &= w[q];
                    if (!tr.dleft[j]) for (int q = 0; q < MW; ++q) tm[(size_t)(foff[f] + nb) * MW + q] &= w[q];
                }
            }
            });
            dm->qs_masks.alloc(mk_n); dm->qs_masks.upload(mk, mk_n, s);
            dm->qs_leaves.alloc(lv2_n); dm->qs_leaves.upload(lv2, lv2_n, s);
            dm->qs_used.alloc(usedf.size()); dm->qs_used.upload(usedf.data(), usedf.size(), s);
            dm->qs_foff.alloc(foff.size()); dm->qs_foff.upload(foff.data(), foff.size(), s);
            dm->qs_S = S; dm->qs_MW = MW;
            HIPCHK(hipStreamSynchronize(s));     // the vectors are locals
        }
    }
    if (dm->qs_MW == 0) build_walk_tables(m, dm, s);
    dm->lut.alloc(lut.size()); dm->lut.upload(lut.data(), lut.size(), s);
    dm->lut_off.alloc(F + 1); dm->lut_off.upload(lut_off.data(), F + 1, s);
    dm->n_codes.alloc(F); dm->n_codes.upload(ncod.data(), F, s);
    dm->miss.alloc(F); dm->miss.upload(miss.data(), F, s);
    dm->ident.alloc(F); dm->ident.upload(ident.data(), F, s);
    HIPCHK(hipStreamSynchronize(s));
    m->dev[device] = dm;
    return guard.release();
}

// score rows [row0, row0+n) of device codes (column-major, Ntab rows per column) with model m.
// feat_col_dev: device array of the F column indices.  Outputs are device pointers (any may be null).
// scratch of one scoring call; the chain allocates it once for all its models (hipMalloc of hundreds of MB per target was
// most of the repair time)
struct PredictScratch { DevBuf<uint4> rec; DevBuf<double> raw; };

void predict_device(rgbm_model* m, int device, hipStream_t s, const int32_t* d_codes, long long Ntab, long long row0, long long n,
                    const int32_t* d_feat_cols, double* d_proba, int32_t* d_label, double* d_top, PredictScratch* scratch = nullptr) {
    using namespace rg;
    if (n <= 0) return;
    DeviceModel* dm = device_model(m, device, s);
    const int F = m->F, nchunk = (F + 15) / 16, K = m->K;
    PredictScratch local;
    PredictScratch& sc = scratch ? *scratch : local;
    if (sc.rec.n < (size_t)nchunk * n) sc.rec.alloc((size_t)nchunk * n);
    if (sc.raw.n < (size_t)K * n) sc.raw.alloc((size_t)K * n);
    DevBuf<uint4>& rec = sc.rec; DevBuf<double>& raw = sc.raw;
    hipLaunchKernelGGL(k_pack_bins, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_codes, Ntab, row0, n,
                       d_feat_cols ? d_feat_cols : dm->ident.p, dm->n_codes.p, dm->lut_off.p, dm->lut.p, dm->miss.p, F, nchunk, rec.p);
    const PredictForm pf = predict_form(m);
    const bool qs = pf.form != FORM_WALK;
    if (qs && pf.mw != dm->qs_MW) throw std::logic_error("predict: the scoring tables do not match the model's form");
    const int qs_tb = pf.tb, qs_tw = pf.tw;
    if (!qs) { std::lock_guard<std::mutex> lk(m->mu); build_walk_tables(m, dm, s); }
    if (qs) {   // bit-vector scoring: no tree walk at all
        const size_t lds = pf.lds;
        const dim3 grid((unsigned)((n + 256 * QS_ROWS - 1) / (256 * QS_ROWS)), K);
        const uint8_t* r8 = reinterpret_cast<const uint8_t*>(rec.p);
#define RGBM_QS(MW, FM, TW, TBN) hipLaunchKernelGGL((k_predict_qs<MW, FM, TW, TBN>), grid, dim3(256), lds, s, r8, n, dm->qs_masks.p, dm->qs_leaves.p, dm->qs_used.p, dm->qs_foff.p, F, dm->qs_S, qs_tb, m->n_iter, K, raw.p)
        if (dm->qs_MW == 1 && F <= 16) { if (qs_tw == 256) RGBM_QS(1, 16, 256, 8); else if (qs_tw == 512) RGBM_QS(1, 16, 512, 8); else RGBM_QS(1, 16, 0, 0); }
        else if (dm->qs_MW == 1) { if (qs_tw == 512) RGBM_QS(1, 32, 512, 8); else if (qs_tw == 1024) RGBM_QS(1, 32, 1024, 4); else RGBM_QS(1, 32, 0, 0); }
        else if (F <= 16) { if (qs_tw == 512) RGBM_QS(2, 16, 512, 8); else if (qs_tw == 1024) RGBM_QS(2, 16, 1024, 4); else RGBM_QS(2, 16, 0, 0); }
        else { if (qs_tw == 1024) RGBM_QS(2, 32, 1024, 4); else if (qs_tw == 2048) RGBM_QS(2, 32, 2048, 2); else RGBM_QS(2, 32, 0, 0); }
#undef RGBM_QS
    }
    else if (nchunk == 1) hipLaunchKernelGGL(k_predict_raw<true>, dim3((unsigned)((n + 255) / 256), K), dim3(256), 0, s, reinterpret_cast<const uint8_t*>(rec.p), n,
                                        dm->nodes.p, dm->leaf_value.p, m->n_iter, K, dm->node_stride, dm->leaf_stride, raw.p);
    else hipLaunchKernelGGL(k_predict_raw<false>, dim3((unsigned)((n + 255) / 256), K), dim3(256), 0, s, reinterpret_cast<const uint8_t*>(rec.p), n,
                            dm->nodes.p, dm->leaf_value.p, m->n_iter, K, dm->node_stride, dm->leaf_stride, raw.p);
    hipLaunchKernelGGL(k_softmax_argmax, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, raw.p, n, m->objective, m->num_class, d_proba, d_label, d_top);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));   // rec/raw are freed on return
}


// version 2 = version 1 + the unseen-category bitmap of every feature; written only when a feature has one
int32_t blob_version(const rgbm_model& m) { for (const Feat& f : m.feats) if (!f.unseen.empty()) return 2; return 1; }

size_t serialised_size(const rgbm_model& m) {
    const int32_t ver = blob_version(m);
    size_t n = 28;
    for (const Feat& f : m.feats) n += 12 + 4 * (size_t)f.V + (ver == 2 ? 4 + 4 * f.unseen.size() : 0);
    for (const Tree& t : m.trees) n += 4 + ((size_t)t.L - 1) * 28 + (size_t)t.L * 12;
    return n;
}

// the model blob, written straight into the caller's buffer (a 19 200-tree model is 23 MB: no intermediate vector, one pass)
void serialise_into(const rgbm_model& m, uint8_t* dst) {
    uint8_t* p = dst;
    auto put = [&](const void* src, size_t n) { memcpy(p, src, n); p += n; };
    const int32_t ver = blob_version(m);
    int32_t hdr[7] = {0x4D424752, ver, m.objective, m.num_class, m.K, m.n_iter, m.F};
    put(hdr, sizeof(hdr));
    for (const Feat& f : m.feats) {
        int32_t h3[3] = {f.n_codes, f.V, f.has_nan}; put(h3, sizeof(h3)); put(f.ub.data(), 4 * (size_t)f.V);
        if (ver == 2) { int32_t nw = (int32_t)f.unseen.size(); put(&nw, 4); put(f.unseen.data(), 4 * (size_t)nw); }
    }
    for (const Tree& t : m.trees) {
        const size_t n = (size_t)t.L - 1;
        put(&t.L, 4);
        put(t.feat, 4 * n); put(t.theta, 4 * n); put(t.dleft, 4 * n);
        put(t.left, 4 * n); put(t.right, 4 * n); put(t.gain, 8 * n);
        put(t.leaf_value, 8 * (size_t)t.L); put(t.leaf_count, 4 * (size_t)t.L);
    }
}

}  // namespace

void rgh::predict_proba_device(const rgbm_model* m, int device, hipStream_t s, const int32_t* d_codes, long long n, const int32_t* d_feat_cols,
                               double* d_proba) {
    predict_device(const_cast<rgbm_model*>(m), device, s, d_codes, n, 0, n, d_feat_cols, d_proba, nullptr, nullptr);
}
void rgh::model_shape(const rgbm_model* m, int32_t* objective, int32_t* num_class, int32_t* n_features) {
    *objective = m->objective; *num_class = m->num_class; *n_features = m->F;
}

// page-locked staging of the chain's outputs (two blocks: model t's labels / probabilities leave the device and are copied into the
// caller's arrays while model t + 1 is scored); kept for the life of the process, at most 256 MiB a block
namespace {
struct ChainStage {
    std::mutex mu; void* p[2] = {nullptr, nullptr}; size_t cap = 0; int device = -1;
    static constexpr size_t KEEP_MAX = (size_t)256 << 20;
    bool get(size_t bytes, int dev) {
        if (bytes == 0 || bytes > KEEP_MAX || getenv("RGBM_NO_PIN") != nullptr) return false;
        if (p[0] && cap >= bytes && device == dev) return true;
        for (int i = 0; i < 2; ++i) if (p[i]) { (void)hipHostFree(p[i]); p[i] = nullptr; }
        cap = 0;
        const size_t want = std::min(KEEP_MAX, bytes + bytes / 8);
        if (hipHostMalloc(&p[0], want, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&p[1], want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            for (int i = 0; i < 2; ++i) if (p[i]) { (void)hipHostFree(p[i]); p[i] = nullptr; }
            return false;
        }
        cap = want; device = dev;
        return true;
    }
};
ChainStage& chain_stage() { static ChainStage* c = new ChainStage(); return *c; }
struct ThreadJoiner { std::vector<std::thread> th; ~ThreadJoiner() { for (auto& t : th) if (t.joinable()) t.join(); } };
}  // namespace

// ---------------------------------------------------------------------------------------------
// The distinct-row view of rgbm_table_train.  Three quarters of the rows of the tables this library repairs are exact copies of
// another row, and a row with a multiplicity gives the expanded table's model byte for byte (rgbm_table_set_row_multiplicity): the table is
// deduplicated ONCE (rgbm_host.h: rgbm_distinct_view) and every target is trained on the result.
// ---------------------------------------------------------------------------------------------
namespace {
// May a fit of this shape use the view at all?  No device, no table: exactly what the multiplicity trainer honours (train_core), plus the
// row-count floor.  rgbm_table_train takes no per-row weights, so that condition of train_core is always met here.
bool distinct_view_may(int64_t rows, int32_t f, const rgbm_params& p, bool table_has_mult, int64_t min_rows) {
    if (table_has_mult) return false;                                             // multiplicities of its own: never a view
    if (p.reserved & (RGBM_FLAG_ROW_SHARDED | RGBM_FLAG_WHOLE_TABLE)) return false;
    if (p.max_depth < 1 || p.max_depth > rg::LV_MAX_DEPTH) return false;          // the level grower
    if (p.bagging_freq > 0 && p.bagging_fraction < 1.0) return false;             // LightGBM draws the bag per ORIGINAL row
    if (p.objective != 0 && p.objective != 1) return false;                       // classifiers
    if (f < 1 || f > 32 || f % 16 == 0) return false;                             // byte 15 of the last 16-feature record carries the multiplicity
    return rows >= min_rows;
}

// the shapes the trainer refused on a table version are remembered by this key: what its refusals depend on besides the bin counts
uint64_t view_shape_key(const rgbm_table& t, const int32_t* feat_cols, int32_t f, const rgbm_params& p, const RunSwitches& sw) {
    std::vector<int32_t> nc((size_t)f);
    for (int i = 0; i < f; ++i) nc[(size_t)i] = (feat_cols[i] >= 0 && feat_cols[i] < t.c) ? t.n_codes[(size_t)feat_cols[i]] : -1;
    std::sort(nc.begin(), nc.end());
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&](uint64_t v) { h = (h ^ v) * 0x100000001b3ull; };
    mix((uint64_t)f); mix((uint64_t)p.max_depth); mix((uint64_t)p.max_bin); mix(sw.joint_root ? 1 : 0); mix(sw.mt_acc2 ? 1 : 0);
    for (int32_t v : nc) mix((uint64_t)(uint32_t)v);
    return h;
}

// The view of `t` for a fit of shape `key`, or null: built by the first caller (the others wait on view.mu), one pass per table version.
std::shared_ptr<const rgbm_table> acquire_view(const rgbm_table& t, uint64_t key, const RunSwitches& sw, uint64_t* version) {
    rgbm_distinct_view& v = t.view;
    std::lock_guard<std::mutex> lk(v.mu);
    *version = v.version;
    if (std::find(v.refused.begin(), v.refused.end(), key) != v.refused.end()) return nullptr;
    const int64_t max_rows = (int64_t)std::floor(sw.distinct_max_ratio * (double)t.n);
    if (v.state == RGBM_VIEW_NOT_WORTH && v.rows <= max_rows) v.state = RGBM_VIEW_NONE;      // (the ratio was raised since)
    if (v.state == RGBM_VIEW_NONE) {
        const auto t0 = std::chrono::steady_clock::now();
        try {
            rgh::DistinctOut r = rgh::distinct_rows_device(t, nullptr, max_rows);
            ++v.builds; v.rows = r.rows;
            if (r.tab) { v.tab = std::shared_ptr<const rgbm_table>(r.tab.release()); v.state = RGBM_VIEW_BUILT; }
            else v.state = RGBM_VIEW_NOT_WORTH;
        } catch (const rgh::distinct_cannot& e) {
            v.state = RGBM_VIEW_CANNOT; v.rows = 0;
            if (sw.timing) fprintf(stderr, "[rgbm] distinct view: cannot (%s)\n", e.what());
        } catch (const rgh::device_oom& e) {
            v.state = RGBM_VIEW_CANNOT; v.rows = 0;
            if (sw.timing) fprintf(stderr, "[rgbm] distinct view: cannot (%s)\n", e.what());
        }
        if (sw.timing && v.state != RGBM_VIEW_CANNOT)
            fprintf(stderr, "[rgbm] distinct view: %lld of %lld rows, %s, build %.1f ms\n", (long long)v.rows, (long long)t.n, v.state == RGBM_VIEW_BUILT ? "built" : "not worth it",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    if (v.state != RGBM_VIEW_BUILT || v.rows > max_rows) return nullptr;
    return v.tab;
}
}  // namespace

// rgbm_release_cache (rgbm_runtime.hip): the page-locked blocks kept for the tree harvest of a batch and for the outputs of a repair chain (not
// while a call uses them)
void rgh::release_host_staging() {
        {
            HarvestArena& a = harvest_arena();
            std::unique_lock<std::mutex> lk(a.mu, std::try_to_lock);
            if (lk.owns_lock() && a.p) { (void)hipHostFree(a.p); a.p = nullptr; a.cap = 0; a.device = -1; }
        }
        {
            ChainStage& c = chain_stage();
            std::unique_lock<std::mutex> lk(c.mu, std::try_to_lock);
            if (lk.owns_lock()) { for (int i = 0; i < 2; ++i) if (c.p[i]) { (void)hipHostFree(c.p[i]); c.p[i] = nullptr; } c.cap = 0; c.device = -1; }
        }
}

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

RGBM_EXPORT int rgbm_table_create(const int32_t* codes, int64_t n, int32_t c, const int32_t* n_codes, int32_t device_id, rgbm_table** out) {
    if (!codes || !n_codes || !out || n <= 0 || c <= 0) return fail(RGBM_ERR_ARG, "rgbm_table_create: bad argument");
    return guarded([&]() {
        use_device(device_id);
        std::unique_ptr<rgbm_table> t(new rgbm_table());
        t->device = device_id; t->n = n; t->c = c; t->n_codes.assign(n_codes, n_codes + c);
        t->codes.alloc((size_t)n * c);
        upload_pinned(t->codes.p, codes, (size_t)n * c * sizeof(int32_t));
        *out = t.release();
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_set_column_kind(rgbm_table* t, int32_t col, int32_t kind) {
    if (!t || col < 0 || col >= t->c || kind < 0 || kind > 1) return fail(RGBM_ERR_ARG, "rgbm_table_set_column_kind: bad argument");
    rgh::ViewWrite view_wr(t);
    if (t->col_kind.size() < (size_t)t->c) t->col_kind.resize(t->c, 0);
    t->col_kind[col] = (uint8_t)kind;
    return RGBM_OK;
}

RGBM_EXPORT int rgbm_table_set_column_values(rgbm_table* t, int32_t col, const double* values, int32_t n) {
    if (!t || col < 0 || col >= t->c || n < 0 || (n > 0 && !values)) return fail(RGBM_ERR_ARG, "rgbm_table_set_column_values: bad argument");
    return guarded([&]() {
        rgh::ViewWrite view_wr(t);
        if (n != 0 && n != t->n_codes[col]) throw std::invalid_argument("rgbm_table_set_column_values: one value per code of the column is needed");
        for (int i = 1; i < n; ++i) if (!(values[i - 1] < values[i])) throw std::invalid_argument("rgbm_table_set_column_values: values must be strictly ascending");
        if (t->col_values.size() < (size_t)t->c) t->col_values.resize(t->c);
        t->col_values[col].assign(values, values + n);
        return RGBM_OK;
    });
}

RGBM_EXPORT void rgbm_table_free(rgbm_table* t) { if (t) { (void)hipSetDevice(t->device); delete t; } }

RGBM_EXPORT int rgbm_table_read_column(const rgbm_table* t, int32_t col, int32_t* out) {
    if (!t || !out || col < 0 || col >= t->c) return fail(RGBM_ERR_ARG, "rgbm_table_read_column: bad argument");
    return guarded([&]() {
        use_device(t->device);
        HIPCHK(hipMemcpy(out, t->codes.p + (size_t)col * t->n, (size_t)t->n * sizeof(int32_t), hipMemcpyDeviceToHost));
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_train(const rgbm_table* t, int32_t target_col, const int32_t* feat_cols, int32_t f, const double* y_value,
                                 const double* class_weight, const rgbm_params* p, rgbm_model** out, rgbm_train_stats* stats) {
    if (!t || !feat_cols || !p || !out) return fail(RGBM_ERR_ARG, "rgbm_table_train: bad argument");
    return guarded([&]() {
        use_device(t->device);
        // the distinct-row view: same model, a fraction of the rows.  The guard stays the trainer: what it refuses on the view (RGBM_ERR_PARAM:
        // a two-chunk shape outside the one-pass form or the 15 joint-bin groups, RGBM_MT_ACC2=0, RGBM_JOINT_ROOT=0) trains on the whole table below
        const RunSwitches sw = read_switches();
        if (sw.distinct && sw.grower != 2 && distinct_view_may(t->n, f, *p, t->has_mult, sw.distinct_min_rows)) {
            const uint64_t key = view_shape_key(*t, feat_cols, f, *p, sw);
            uint64_t version = 0;
            if (std::shared_ptr<const rgbm_table> view = acquire_view(*t, key, sw, &version)) {
                try {
                    *out = train_core(*view, target_col, feat_cols, f, y_value, class_weight, nullptr, nullptr, *p, stats, true);
                    return RGBM_OK;
                } catch (const std::invalid_argument& e) {
                    if (sw.timing) fprintf(stderr, "[rgbm] distinct view: target %d refused (%s), training the whole table\n", target_col, e.what());
                    std::lock_guard<std::mutex> lk(t->view.mu);
                    if (t->view.version == version) t->view.refused.push_back(key);
                }
            }
        }
        try {
            *out = train_core(*t, target_col, feat_cols, f, y_value, class_weight, nullptr, nullptr, *p, stats);
        } catch (...) {
            // a rank that fails inside a row-sharded call must not leave its peers waiting in their next all-reduce
            if ((p->reserved & RGBM_FLAG_ROW_SHARDED) && (comm_kind() == 1 || comm_kind() == 3)) comm_abort();
            throw;
        }
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_distinct_view_eligible(int64_t rows, int32_t f, const rgbm_params* p, int32_t table_has_mult, int64_t min_rows) {
    if (!p) return fail(RGBM_ERR_ARG, "rgbm_distinct_view_eligible: bad argument");
    return distinct_view_may(rows, f, *p, table_has_mult != 0, min_rows > 0 ? min_rows : DISTINCT_MIN_ROWS) ? 1 : 0;
}

RGBM_EXPORT int rgbm_table_distinct_view_info(const rgbm_table* t, int32_t* state, int64_t* rows, int64_t* builds) {
    if (!t) return fail(RGBM_ERR_ARG, "rgbm_table_distinct_view_info: bad argument");
    std::lock_guard<std::mutex> lk(t->view.mu);
    if (state) *state = t->view.state;
    if (rows) *rows = t->view.rows;
    if (builds) *builds = t->view.builds;
    return RGBM_OK;
}

RGBM_EXPORT int rgbm_table_train_batch(const rgbm_fit_spec* fits, int32_t n_fits, rgbm_model** out_models, int32_t* out_status) {
    if (!fits || n_fits <= 0 || !out_models || !out_status || !fits[0].table) return fail(RGBM_ERR_ARG, "rgbm_table_train_batch: bad argument");
    return guarded([&]() {
        use_device(fits[0].table->device);
        for (int32_t i = 0; i < n_fits; ++i) { out_models[i] = nullptr; out_status[i] = RGBM_OK; }
        // a failure of the batch as a whole (not of one fit) returns no models: the ones already trained are released here, the caller
        // only sees the error code
        try { train_batch_small(fits, n_fits, out_models, out_status); }
        catch (...) { for (int32_t i = 0; i < n_fits; ++i) { delete out_models[i]; out_models[i] = nullptr; } throw; }
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_train_batch_report(int32_t* out, int32_t n) {
    if (!out || n < 0) return fail(RGBM_ERR_ARG, "rgbm_table_train_batch_report: bad argument");
    const std::vector<BatchReportRow>& r = batch_report();
    if ((size_t)n != r.size()) return fail(RGBM_ERR_ARG, "rgbm_table_train_batch_report: n is not the number of fits of this thread's last rgbm_table_train_batch call");
    for (int32_t i = 0; i < n; ++i) { out[4 * i] = r[i].route; out[4 * i + 1] = r[i].scan_waves; out[4 * i + 2] = r[i].nchunk; out[4 * i + 3] = r[i].lds_bytes; }
    return RGBM_OK;
}

RGBM_EXPORT int rgbm_train(const int32_t* X, int64_t n, int32_t f, const int32_t* n_codes, const int32_t* y_code, int32_t n_y_codes,
                           const double* y_value, const double* class_weight, const double* sample_weight, const rgbm_params* p,
                           rgbm_model** out, rgbm_train_stats* stats) {
    if (!X || !n_codes || !y_code || !p || !out || n <= 0 || f <= 0 || n_y_codes <= 0) return fail(RGBM_ERR_ARG, "rgbm_train: bad argument");
    return guarded([&]() {
        use_device(p->device_id);
        for (int64_t i = 0; i < n; ++i) if (y_code[i] < 0 || y_code[i] >= n_y_codes) throw std::out_of_range("y_code outside [0, n_y_codes)");
        rgbm_table tab; tab.device = p->device_id; tab.n = n; tab.c = f + 1;
        tab.n_codes.assign(n_codes, n_codes + f); tab.n_codes.push_back(n_y_codes);
        tab.codes.alloc((size_t)n * (f + 1));
        HIPCHK(hipMemcpy(tab.codes.p, X, (size_t)n * f * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(tab.codes.p + (size_t)n * f, y_code, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
        std::vector<int32_t> fc(f); for (int i = 0; i < f; ++i) fc[i] = i;
        HostLabelStats hls;
        if (sample_weight) {   // row-order sums (numerics spec: only defined on the host-array path)
            hls.valid = true; hls.tot.assign(n_y_codes, 0.0);
            for (int64_t i = 0; i < n; ++i) {
                double w = (class_weight ? class_weight[y_code[i]] : 1.0); w = w * sample_weight[i]; w = (double)(float)w;
                hls.tot[y_code[i]] += w; if (w > hls.w_max) hls.w_max = w;
                if (y_value) hls.suml += (double)(float)y_value[y_code[i]] * w;
            }
        }
        *out = train_core(tab, f, fc.data(), f, y_value, class_weight, sample_weight, &hls, *p, stats);
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_predict(const rgbm_model* m, const int32_t* X, int64_t n, int32_t f, int32_t device_id, double* out) {
    if (!m || !X || !out || n < 0) return fail(RGBM_ERR_ARG, "rgbm_predict: bad argument");
    if (f != m->F) return fail(RGBM_ERR_ARG, "rgbm_predict: feature count differs from the model's");
    if (n == 0) return RGBM_OK;
    return guarded([&]() {
        use_device(device_id);
        StreamGuard sg; hipStream_t s = sg.s;
        DevBuf<int32_t> codes((size_t)n * f); codes.upload(X, (size_t)n * f, s);
        const int ncol = m->objective == 2 ? 1 : m->num_class;
        DevBuf<double> proba((size_t)n * ncol);
        predict_device(const_cast<rgbm_model*>(m), device_id, s, codes.p, n, 0, n, nullptr, proba.p, nullptr, nullptr);
        HIPCHK(hipMemcpy(out, proba.p, (size_t)n * ncol * sizeof(double), hipMemcpyDeviceToHost));
        return RGBM_OK;
    });
}

static int chain_device(rgbm_model* const* models, int32_t T, const int32_t* target_col, const int32_t* feat_cols, const int32_t* feat_off,
                        const int32_t* class_code, const int32_t* class_off, int32_t* d_codes, long long Ntab, long long row0, long long n,
                        int device, hipStream_t s, int32_t* out_label, double* out_prob,
                        int32_t* d_label_all = nullptr, double* d_prob_all = nullptr, long long sink_stride = 0 /* device sinks [T][sink_stride]: the outputs STAY on the device (C2 on device buffers) */) {
    using namespace rg;
    for (int t = 0; t < T; ++t)
        if (feat_off[t + 1] - feat_off[t] != models[t]->F) throw std::invalid_argument("chain: feature list length differs from the model's feature count");
    PredictScratch scratch;
    {   // size the scratch once for the largest model of the chain
        size_t mr = 0, mk = 0;
        for (int t = 0; t < T; ++t) { mr = std::max(mr, (size_t)((models[t]->F + 15) / 16)); mk = std::max(mk, (size_t)models[t]->K); }
        scratch.rec.alloc(mr * (size_t)n); scratch.raw.alloc(mk * (size_t)n);
    }
    const bool timing = getenv("RGBM_TIMING") != nullptr;
    double t_score = 0, t_fill = 0, t_copy = 0;
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    // ---- outputs: double-buffered on the device and in page-locked host memory when the staging blocks are free
    ChainStage& CS = chain_stage();
    std::unique_lock<std::mutex> cs_lock(CS.mu, std::try_to_lock);
    const size_t lab_bytes = ((size_t)n * sizeof(int32_t) + 255) & ~(size_t)255, out_bytes = lab_bytes + (size_t)n * sizeof(double);
    const bool staged = (out_label || out_prob) && T > 1 && cs_lock.owns_lock() && CS.get(out_bytes, device);
    DevBuf<int32_t> d_label[2]; DevBuf<double> d_top[2];
    for (int b = 0; b < (staged ? 2 : 1); ++b) { d_label[b].alloc(n); d_top[b].alloc(n); }
    StreamGuard copy_stream;
    hipEvent_t e_copied[2] = {nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{e_copied};
    if (staged) for (int b = 0; b < 2; ++b) HIPCHK(hipEventCreateWithFlags(&e_copied[b], hipEventDisableTiming));
    std::atomic<int> copy_err{0};
    std::thread helper[2];
    struct HelperJoin { std::thread* h; ~HelperJoin() { for (int i = 0; i < 2; ++i) if (h[i].joinable()) h[i].join(); } } hj{helper};
    // ---- predictor tables of the chain's models: built in the background, in chain order, on a few host threads (host work + small
    // uploads, 1-25 ms a model); predict_device -> device_model waits on the model's mutex for a build in flight, or builds it itself
    std::vector<rgbm_model*> todo;
    for (int t = 0; t < T; ++t) if (std::find(todo.begin(), todo.end(), models[t]) == todo.end()) todo.push_back(models[t]);
    std::atomic<size_t> next{0}; std::mutex emu; std::exception_ptr build_err;
    ThreadJoiner builders;
    {
        const size_t nth = std::min<size_t>(std::min<size_t>(todo.size(), 16), std::max(1u, std::thread::hardware_concurrency()));
        auto work = [&]() {
            try {
                use_device(device);
                StreamGuard own;
                for (size_t j = next.fetch_add(1); j < todo.size(); j = next.fetch_add(1)) device_model(todo[j], device, own.s);
            } catch (...) { std::lock_guard<std::mutex> lk(emu); if (!build_err) build_err = std::current_exception(); }
        };
        if (todo.size() > 1) for (size_t q = 0; q < nth; ++q) builders.th.emplace_back(work);
    }
    for (int t = 0; t < T; ++t) {
        rgbm_model* m = models[t];
        const int F = m->F, b = staged ? (t & 1) : 0;
        double t1 = now();
        if (helper[b].joinable()) helper[b].join();                  // model t - 2 has left d_label[b] / d_top[b] and the staging block b
        if (copy_err.load()) throw std::runtime_error("chain: copy of the repaired cells to the host failed");
        t_copy += now() - t1; t1 = now();
        DevBuf<int32_t> d_fc(F); d_fc.upload(feat_cols + feat_off[t], F, s);
        predict_device(m, device, s, d_codes, Ntab, row0, n, d_fc.p, nullptr, d_label[b].p, d_top[b].p, &scratch);
        double t2 = now(); t_score += t2 - t1;
        if (m->objective != 2) {
            int ncc = class_off ? class_off[t + 1] - class_off[t] : m->num_class;
            DevBuf<int32_t> d_cc(std::max(ncc, 1));
            std::vector<int32_t> cc(std::max(ncc, 1), 0);
            for (int i = 0; i < ncc; ++i) cc[i] = class_code ? class_code[class_off[t] + i] : i;
            d_cc.upload(cc.data(), cc.size(), s);
            hipLaunchKernelGGL(k_fill_cells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_codes + (long long)target_col[t] * Ntab + row0, n, d_label[b].p, d_cc.p, ncc);
            HIPCHK(hipStreamSynchronize(s));
        }
        double t3 = now(); t_fill += t3 - t2;
        if (d_label_all) HIPCHK(hipMemcpyAsync(d_label_all + (size_t)t * sink_stride, d_label[b].p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        if (d_prob_all) HIPCHK(hipMemcpyAsync(d_prob_all + (size_t)t * sink_stride, d_top[b].p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
        if ((d_label_all || d_prob_all) && !staged) HIPCHK(hipStreamSynchronize(s));
        if (staged) {
            char* pin = (char*)CS.p[b];
            if (out_label) HIPCHK(hipMemcpyAsync(pin, d_label[b].p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, copy_stream.s));
            if (out_prob) HIPCHK(hipMemcpyAsync(pin + lab_bytes, d_top[b].p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, copy_stream.s));
            HIPCHK(hipEventRecord(e_copied[b], copy_stream.s));
            int32_t* ol = out_label ? out_label + (size_t)t * n : nullptr; double* op = out_prob ? out_prob + (size_t)t * n : nullptr;
            hipEvent_t ev = e_copied[b];
            helper[b] = std::thread([=, &copy_err]() {
                if (hipEventSynchronize(ev) != hipSuccess) { copy_err.store(1); return; }
                std::thread second;
                if (ol && op) second = std::thread([=]() { memcpy(op, pin + lab_bytes, (size_t)n * sizeof(double)); });
                else if (op) memcpy(op, pin + lab_bytes, (size_t)n * sizeof(double));
                if (ol) memcpy(ol, pin, (size_t)n * sizeof(int32_t));
                if (second.joinable()) second.join();
            });
        } else {
            if (out_label) HIPCHK(hipMemcpy(out_label + (size_t)t * n, d_label[b].p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
            if (out_prob) HIPCHK(hipMemcpy(out_prob + (size_t)t * n, d_top[b].p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        }
        t_copy += now() - t3;
    }
    {
        const double t4 = now();
        for (int b = 0; b < 2; ++b) if (helper[b].joinable()) helper[b].join();
        t_copy += now() - t4;
        if (copy_err.load()) throw std::runtime_error("chain: copy of the repaired cells to the host failed");
    }
    for (auto& x : builders.th) if (x.joinable()) x.join();
    if (build_err) std::rethrow_exception(build_err);
    if (timing) fprintf(stderr, "[rgbm] chain of %d models over %lld rows: %.1f ms (score incl. waiting for tables %.1f ms, fill %.1f ms, copy out not hidden %.1f ms, %s)\n",
                        T, n, (now() - t_begin) * 1e3, t_score * 1e3, t_fill * 1e3, t_copy * 1e3, staged ? "staged" : "direct");
    return RGBM_OK;
}

RGBM_EXPORT int rgbm_repair_chain(const rgbm_model* const* models, int32_t T, const int32_t* target_col, const int32_t* feat_cols,
                                  const int32_t* feat_off, const int32_t* class_code, const int32_t* class_off, int32_t* table, int64_t n,
                                  int32_t c, int32_t device_id, int32_t* out_label, double* out_prob) {
    if (!models || T < 0 || !target_col || !feat_cols || !feat_off || !class_off || !table || n < 0 || c <= 0) return fail(RGBM_ERR_ARG, "rgbm_repair_chain: bad argument");
    if (n == 0 || T == 0) return RGBM_OK;
    return guarded([&]() {
        use_device(device_id);
        StreamGuard sg; hipStream_t s = sg.s;
        DevBuf<int32_t> codes((size_t)n * c); codes.upload(table, (size_t)n * c, s);
        chain_device(const_cast<rgbm_model* const*>(models), T, target_col, feat_cols, feat_off, class_code, class_off, codes.p, n, 0, n, device_id, s, out_label, out_prob);
        HIPCHK(hipMemcpy(table, codes.p, (size_t)n * c * sizeof(int32_t), hipMemcpyDeviceToHost));
        return RGBM_OK;
    });
}

// Rows with multiplicities: row i of the table stands for mult[i] (1..255) identical rows of a larger table (repair.pipeline.distinct_rows makes
// such a table: identical (features, label) rows take identical paths and gradients in every tree, and every sum of the trainer is an exact
// integer, so m times a row's value IS the sum over its m copies).  Every later rgbm_table_train on this table weighs the row so -- code counts,
// child counts, histogram sums, the coarse sums behind the fixed-point grids -- and returns byte for byte the model the expanded table gives.
// NULL clears.  Level grower, <= 32 features with a free byte in the last record, no bagging (rgbm.hip train_core says so when it does not apply).
RGBM_EXPORT int rgbm_table_set_row_multiplicity(rgbm_table* t, const uint8_t* mult) {
    if (!t) return fail(RGBM_ERR_ARG, "rgbm_table_set_row_multiplicity: bad argument");
    return guarded([&]() {
        use_device(t->device);
        rgh::ViewWrite view_wr(t);
        if (!mult) { t->has_mult = false; t->mult_total = 0; return RGBM_OK; }
        int64_t tot = 0;
        for (int64_t i = 0; i < t->n; ++i) { if (mult[i] == 0) throw std::invalid_argument("rgbm_table_set_row_multiplicity: a multiplicity of 0"); tot += mult[i]; }
        if (tot >= (1ll << 31) - 4096) throw std::invalid_argument("rgbm_table_set_row_multiplicity: the expanded table has more than 2^31 rows");
        StreamGuard sg;
        t->mult.alloc((size_t)t->n);
        t->mult.upload(mult, (size_t)t->n, sg.s);
        HIPCHK(hipStreamSynchronize(sg.s));
        t->has_mult = true; t->mult_total = tot;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_repair_chain(rgbm_table* t, const rgbm_model* const* models, int32_t T, const int32_t* target_col,
                                        const int32_t* feat_cols, const int32_t* feat_off, int64_t row_begin, int64_t n_rows,
                                        int32_t* out_label, double* out_prob) {
    if (!t || !models || T < 0 || !target_col || !feat_cols || !feat_off || row_begin < 0 || n_rows < 0 || row_begin + n_rows > t->n)
        return fail(RGBM_ERR_ARG, "rgbm_table_repair_chain: bad argument");
    if (n_rows == 0 || T == 0) return RGBM_OK;
    return guarded([&]() {
        use_device(t->device);
        rgh::ViewWrite view_wr(t);
        StreamGuard sg;
        return chain_device(const_cast<rgbm_model* const*>(models), T, target_col, feat_cols, feat_off, nullptr, nullptr, t->codes.p, t->n, row_begin, n_rows,
                            t->device, sg.s, out_label, out_prob);
    });
}

RGBM_EXPORT int rgbm_model_save(const rgbm_model* m, void* buf, size_t* len) {
    if (!m || !len) return fail(RGBM_ERR_ARG, "rgbm_model_save: bad argument");
    return guarded([&]() {
        const size_t need = serialised_size(*m);
        if (!buf) { *len = need; return RGBM_OK; }
        if (*len < need) { *len = need; return fail(RGBM_ERR_ARG, "rgbm_model_save: buffer too small"); }
        serialise_into(*m, (uint8_t*)buf); *len = need;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_model_load(const void* buf, size_t len, rgbm_model** out) {
    if (!buf || !out) return fail(RGBM_ERR_ARG, "rgbm_model_load: bad argument");
    return guarded([&]() {
        const uint8_t* p = (const uint8_t*)buf; const uint8_t* end = p + len;
        auto need = [&](size_t n) { if ((size_t)(end - p) < n) throw std::length_error("truncated model"); };
        try {
            need(28); int32_t hdr[7]; memcpy(hdr, p, 28); p += 28;
            if (hdr[0] != 0x4D424752 || (hdr[1] != 1 && hdr[1] != 2)) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: bad magic/version");
            std::unique_ptr<rgbm_model> m(new rgbm_model());
            m->objective = hdr[2]; m->num_class = hdr[3]; m->K = hdr[4]; m->n_iter = hdr[5]; m->F = hdr[6];
            if (m->F < 0 || m->K < 1 || m->n_iter < 0 || m->F > 65535) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: bad header");
            // the predictor indexes its K x n score scratch by num_class: the header must be self-consistent
            if (m->objective < 0 || m->objective > 2 || m->num_class < 1) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: bad objective / num_class");
            if (m->objective == 1 ? m->K != m->num_class : m->K != 1) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: class-tree count does not match the objective");
            if (m->objective == 0 && m->num_class != 2) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: binary model with num_class != 2");
            // every tree needs at least 16 bytes (L + one leaf value + one leaf count): bound the allocation by the buffer
            if ((unsigned long long)m->n_iter * (unsigned long long)m->K > (unsigned long long)(end - p) / 16ull) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: tree count exceeds the buffer");
            m->feats.resize(m->F);
            for (Feat& f : m->feats) {
                need(12); int32_t h3[3]; memcpy(h3, p, 12); p += 12;
                f.n_codes = h3[0]; f.V = h3[1]; f.has_nan = h3[2];
                if (f.V < 0 || f.V > 255) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: bad bin count");
                need(4 * (size_t)f.V); f.ub.resize(f.V); memcpy(f.ub.data(), p, 4 * (size_t)f.V); p += 4 * (size_t)f.V;
                if (hdr[1] == 2) {
                    need(4); int32_t nw; memcpy(&nw, p, 4); p += 4;
                    if (nw < 0 || (nw != 0 && (f.n_codes < 0 || nw != (f.n_codes + 31) / 32))) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: bad unseen-category bitmap");
                    need(4 * (size_t)nw); f.unseen.resize(nw); memcpy(f.unseen.data(), p, 4 * (size_t)nw); p += 4 * (size_t)nw;
                }
            }
            m->trees.resize((size_t)m->n_iter * m->K);
            std::vector<uint8_t> refs;
            for (Tree& t : m->trees) {
                int32_t L_; need(4); memcpy(&L_, p, 4); p += 4;
                if (L_ < 1 || L_ > 32767) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: bad leaf count");
                const size_t n = (size_t)L_ - 1;
                need(n * 28 + (size_t)L_ * 12);
                t.alloc(L_);
                auto rd32 = [&](int32_t* v, size_t k) { memcpy(v, p, 4 * k); p += 4 * k; };
                auto rd64 = [&](double* v, size_t k) { memcpy(v, p, 8 * k); p += 8 * k; };
                rd32(t.feat, n); rd32(t.theta, n); rd32(t.dleft, n); rd32(t.left, n); rd32(t.right, n); rd64(t.gain, n);
                rd64(t.leaf_value, t.L); rd32(t.leaf_count, t.L);
                for (size_t j = 0; j < n; ++j) {
                    if (t.feat[j] < 0 || t.feat[j] >= m->F) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: node feature out of range");
                    if (t.theta[j] < -1 || t.theta[j] > 254) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: node threshold out of range");
                    auto okc = [&](int ch) { return ch < 0 ? (~ch) < t.L : ch < (int)n && ch > (int)j; };
                    if (!okc(t.left[j]) || !okc(t.right[j])) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: bad child link");
                }
                // the links must form a tree: every leaf and every node but the root referenced exactly once (a shared child would make
                // the in-order traversal of device_model emit more than L leaves, past the tree's leaf block)
                refs.assign(n + (size_t)t.L, 0);
                bool tree_ok = true;
                for (size_t j = 0; j < n; ++j)
                    for (int ch : {t.left[j], t.right[j]}) if (++refs[ch < 0 ? n + (size_t)(~ch) : (size_t)ch] > 1) tree_ok = false;
                for (size_t j = 1; j < refs.size(); ++j) if (refs[j] != 1) tree_ok = false;       // (entry 0: the root, or the leaf of a stump)
                if (!tree_ok) return fail(RGBM_ERR_FORMAT, "rgbm_model_load: child links do not form a tree");
            }
            *out = m.release();
            return RGBM_OK;
        } catch (const std::length_error&) { return fail(RGBM_ERR_FORMAT, "rgbm_model_load: truncated buffer"); }
    });
}

// The chained repair of this rank's rows with its outputs LEFT ON THE DEVICE, all-gathered over the communicator there, and only then copied to
// the host: out_label / out_prob = [nranks][T][max_rows] (a rank's block holds its n_rows rows of every model, padded to max_rows = the largest
// rank's row count -- the caller exchanged the counts with rgbm_comm_all_gather_sizes).  Same labels / probabilities as rgbm_table_repair_chain.
RGBM_EXPORT int rgbm_table_repair_chain_gather(rgbm_table* t, const rgbm_model* const* models, int32_t T, const int32_t* target_col,
                                               const int32_t* feat_cols, const int32_t* feat_off, int64_t row_begin, int64_t n_rows, int64_t max_rows,
                                               int32_t* out_label, double* out_prob) {
    if (!t || !models || T < 1 || !target_col || !feat_cols || !feat_off || row_begin < 0 || n_rows < 0 || row_begin + n_rows > t->n || max_rows < n_rows || max_rows < 1 || !out_label || !out_prob)
        return fail(RGBM_ERR_ARG, "rgbm_table_repair_chain_gather: bad argument");
    return guarded([&]() {
        use_device(t->device);
        rgh::ViewWrite view_wr(t);
        const int nr = std::max(1, comm_nranks());
        StreamGuard sg; hipStream_t s = sg.s;
        const size_t blk = (size_t)T * (size_t)max_rows;
        DevBuf<int32_t> d_lab(blk), d_lab_all(blk * (size_t)nr); DevBuf<double> d_prob(blk), d_prob_all(blk * (size_t)nr);
        d_lab.zero(s); d_prob.zero(s);
        if (n_rows > 0)
            chain_device(const_cast<rgbm_model* const*>(models), T, target_col, feat_cols, feat_off, nullptr, nullptr, t->codes.p, t->n, row_begin, n_rows,
                         t->device, s, nullptr, nullptr, d_lab.p, d_prob.p, (long long)max_rows);
        const auto t0 = std::chrono::steady_clock::now();
        all_gather_on(d_lab.p, d_lab_all.p, blk * sizeof(int32_t), s);
        all_gather_on(d_prob.p, d_prob_all.p, blk * sizeof(double), s);
        HIPCHK(hipMemcpyAsync(out_label, d_lab_all.p, blk * (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out_prob, d_prob_all.p, blk * (size_t)nr * sizeof(double), hipMemcpyDeviceToHost, s));
        stream_sync_watchdog(s);
        rgh::GatherStats& G = rgh::gather_stats();
        G.bytes += (long long)(blk * (size_t)nr * 12); G.calls += 2;
        G.ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        return RGBM_OK;
    });
}

RGBM_EXPORT void rgbm_model_free(rgbm_model* m) { delete m; }

RGBM_EXPORT int rgbm_model_info(const rgbm_model* m, int32_t* info) {
    if (!m || !info) return fail(RGBM_ERR_ARG, "rgbm_model_info: bad argument");
    info[0] = m->objective; info[1] = m->num_class; info[2] = m->K; info[3] = m->n_iter; info[4] = m->F;
    return RGBM_OK;
}

RGBM_EXPORT int rgbm_model_predict_form(const rgbm_model* m, int32_t* out) {
    if (!m || !out) return fail(RGBM_ERR_ARG, "rgbm_model_predict_form: bad argument");
    return guarded([&]() {
        const PredictForm pf = predict_form(m);
        out[0] = pf.form; out[1] = pf.mw; out[2] = pf.tw; out[3] = pf.tb; out[4] = (int32_t)pf.lds;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_level_pass_plan(const int32_t* nbins, int32_t f, int64_t n_rows, int32_t k, int32_t max_depth, int32_t with_mult, double* out, int32_t out_len, int32_t* n_out) {
    if (!nbins || !out || !n_out || f < 1 || f > 255 || n_rows < 1 || k < 1 || max_depth < 1 || max_depth > rg::LV_MAX_DEPTH) return fail(RGBM_ERR_ARG, "rgbm_level_pass_plan: bad argument");
    return guarded([&]() {
        using namespace rg;
        const RunSwitches sw = read_switches();
        std::vector<FeatMeta> fmeta(f); std::vector<ChunkMeta> cmeta((f + 15) / 16);
        int totbins = 0;
        for (int j = 0; j < f; ++j) {
            if (nbins[j] < 1 || nbins[j] > 256) return fail(RGBM_ERR_ARG, "rgbm_level_pass_plan: a feature has 1..256 bins");
            FeatMeta& m = fmeta[j]; memset(&m, 0, sizeof(m)); m.nbins = nbins[j]; m.V = nbins[j]; m.hoff = totbins; totbins += nbins[j];
        }
        for (size_t ch = 0; ch < cmeta.size(); ++ch) {
            ChunkMeta& cm = cmeta[ch]; cm.first_feat = (int)ch * 16; cm.nfeat = std::min(16, f - (int)ch * 16); cm.fast_slots = 0; cm.wide_bins = 0;
            for (int j = 0; j < cm.nfeat; ++j) { fmeta[ch * 16 + j].wide_off = cm.wide_bins; cm.wide_bins += fmeta[ch * 16 + j].nbins; }
        }
        const LevelPassPlan P = plan_level_passes(sw, fmeta, cmeta, n_rows, k, max_depth, with_mult != 0, level_lds_bytes(sw));
        std::vector<double> v;
        const long long root_wg = (long long)P.root_gx * k * (long long)cmeta.size();
        v.insert(v.end(), {(double)P.root_gx, (double)P.part_items, 0.0, (double)root_wg, ROOT_PASS_COST.t_fix_us, (double)n_rows / P.root_gx * ROOT_PASS_COST.t_row_ns * 1e-3});
        int nl = 0;
        for (int level = 1; level < max_depth; ++level) for (const MtLaunch& L : P.mt[level]) {
            const PassCost& c = mt_pass_cost(L.acc2 != 0, L.rot != 0);
            v.insert(v.end(), {(double)level, (double)L.ch, (double)L.slot0, (double)L.nslots, (double)L.route, (double)L.T, (double)L.G, (double)L.gx, (double)L.acc2, (double)L.rot,
                               c.t_fix_us, (double)n_rows / L.gx * (c.t_row_ns + std::min(L.T, (int)k) * c.t_pair_ns) * 1e-3});
            ++nl;
        }
        v[2] = (double)nl;
        *n_out = (int32_t)v.size();
        if ((size_t)out_len < v.size()) return fail(RGBM_ERR_ARG, "rgbm_level_pass_plan: output too small");
        std::copy(v.begin(), v.end(), out);
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_model_importance(const rgbm_model* m, int32_t type, double* out) {
    if (!m || !out) return fail(RGBM_ERR_ARG, "rgbm_model_importance: bad argument");
    for (int f = 0; f < m->F; ++f) out[f] = 0.0;
    for (const Tree& t : m->trees) for (int j = 0; j < t.L - 1; ++j) out[t.feat[j]] += type == 0 ? 1.0 : t.gain[j];
    return RGBM_OK;
}

}  // extern "C"
