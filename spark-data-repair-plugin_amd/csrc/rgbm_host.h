// rgbm_host.h -- host-side plumbing shared by the translation units of librepairgbm.so:
// thread-local error text, HIP error checks, device buffers, the HBM-resident table object.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rgbm.h"

#define RGBM_EXPORT __attribute__((visibility("default")))

namespace rgh {

std::string& last_error();                       // thread-local (defined in rgbm_runtime.hip)
inline int fail(int code, const std::string& msg) { last_error() = msg; return code; }

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            char b_[512];                                                                              \
            snprintf(b_, sizeof(b_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            throw std::runtime_error(b_);                                                              \
        }                                                                                              \
    } while (0)

// Device memory comes from a small caching pool: a training call on K class trees allocates ~1.2 KB per row and class
// tree (scores, gradients, node ids, ...) and hipMalloc/hipFree of 12 GB cost 0.3 s -- more than 15 boosting iterations.
// Freed blocks are kept (best fit: the smallest cached block that is large enough) up to RGBM_POOL_MB (default 65536;
// 0 = plain hipMalloc/hipFree); callers release buffers only after synchronising the stream that used them.
void* pool_alloc(size_t bytes, size_t* block_bytes, int* device);     // defined in rgbm_runtime.hip; throws std::runtime_error
void pool_free(void* p, size_t block_bytes, int device);
void pool_trim(size_t keep_bytes);
// The two debugging switches, each read once per process; the first use of either says so on stderr ("[rgbm guard] on, self-check ok",
// "[rgbm poison] on": a run that was meant to have them can tell that it had).  Defined in rgbm_runtime.hip.
bool guard_on();                                 // RGBM_GUARD=1: guard zones around every buffer, checked on free
bool poison_on();                                // RGBM_POISON=1: every DevBuf starts as 0xA5 bytes

template <typename T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;
    size_t block_bytes = 0; int device = 0;
    DevBuf() {}
    explicit DevBuf(size_t count) { alloc(count); }
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    void alloc(size_t count) {
        release(); n = count;
        if (count) p = static_cast<T*>(pool_alloc(count * sizeof(T), &block_bytes, &device));
        // RGBM_POISON=1 (tests): every buffer starts out as 0xA5 bytes instead of whatever the pool block held -- a kernel that reads a
        // location nobody wrote then fails the bit-exact comparison with the oracle every time, not once in a few processes
        static const bool poison = poison_on();
        if (poison && count) { HIPCHK(hipMemset(p, 0xA5, count * sizeof(T))); HIPCHK(hipStreamSynchronize(nullptr)); }   // (our streams do not wait for the null stream)
    }
    void release() { if (p) { pool_free(p, block_bytes, device); p = nullptr; } n = 0; block_bytes = 0; }
    ~DevBuf() { release(); }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(block_bytes, o.block_bytes); std::swap(device, o.device); }
    void upload(const T* h, size_t count, hipStream_t s) { if (count) HIPCHK(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s)); }
    void download(T* h, size_t count, hipStream_t s) const { if (count) HIPCHK(hipMemcpyAsync(h, p, count * sizeof(T), hipMemcpyDeviceToHost, s)); }
    void zero(hipStream_t s) { if (n) HIPCHK(hipMemsetAsync(p, 0, n * sizeof(T), s)); }
};

inline void use_device(int device_id) {
    int nd = 0;
    hipError_t e = hipGetDeviceCount(&nd);
    if (e != hipSuccess || nd <= 0) throw std::domain_error("no HIP device available (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= nd) throw std::domain_error("device_id out of range: there are " + std::to_string(nd) + " HIP device(s)");
    HIPCHK(hipSetDevice(device_id));
}

struct StreamGuard {
    hipStream_t s = nullptr;
    StreamGuard() { HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};

// a HIP event that lives as long as its scope, whatever leaves it (timing events: hipEventElapsedTime needs them)
struct Event {
    hipEvent_t e = nullptr;
    Event() { HIPCHK(hipEventCreate(&e)); }
    Event(const Event&) = delete; Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

// Runs fn once per process, device and tag.  For function attributes (hipFuncSetAttribute): they belong to the function, not to the
// call, and other threads are launching the kernels while a new training call sets up.  A call that throws runs again next time.
enum OnceTag { ONCE_LEVEL_LDS = 0, ONCE_SMALL_TREE_LDS, ONCE_HIST_LDS, ONCE_TAGS };
inline void once_per_device(int device, OnceTag tag, void (*fn)()) {
    static std::mutex mu; static char done[64][ONCE_TAGS] = {};
    std::lock_guard<std::mutex> lk(mu);
    if (done[device & 63][tag]) return;
    fn();
    done[device & 63][tag] = 1;
}

// ---- rgbm_runtime.hip
// blocking host -> HBM copy of a caller-owned block on the current device, through the page-locked staging ring when it pays (RGBM_NO_PIN=1: never); throws
void upload_pinned(void* dst, const void* src, size_t bytes);
// RGBM_TRACE: enqueues on s the wrapping sum of the 64-bit words of src [bytes / 8] (device) into *d_out (device, zeroed by the caller)
void trace_sum(const void* src, size_t bytes, unsigned long long* d_out, hipStream_t s);
// defined in rgbm.hip for rgbm_release_cache: frees the page-locked blocks the batch harvest and the repair chain keep, unless a call is using them
void release_host_staging();

// ---- rgbm_comm.hip: the communicator of the CALLING THREAD, as far as the trainer and the chained repair (rgbm.hip) use it
enum { AR_I64 = 0, AR_U32 = 1, AR_I32 = 2 };     // element type of all_reduce
int comm_kind();                                 // 0 none, 1 RCCL, 2 in-process thread group, 3 member of a fusion group
int comm_rank();                                 // this thread's rank; 0 without a communicator
int comm_nranks();                               // ranks of the communicator; 1 without one
// in-place sum of `count` elements over the ranks, enqueued on s (a fusion member: parks until all members of its group have arrived); no-op without a communicator; throws
void all_reduce(void* buf, size_t count, int type, hipStream_t s);
// recv [nranks][bytes] = every rank's send [bytes] (device), enqueued on s; a copy without a communicator; throws from inside a fusion group
void all_gather_on(const void* send, void* recv, size_t bytes, hipStream_t s);
// waits for s; with an RCCL communicator it polls, and on a stream error, an RCCL error or RGBM_COMM_TIMEOUT_S without progress it aborts the communicator and throws
void stream_sync_watchdog(hipStream_t s);
// a failing rank gives up its RCCL communicator (or leaves its fusion group as failed) so that no peer waits for its next collective; the thread has none afterwards
void comm_abort();
// bytes received by, nanoseconds spent in and number of the all-gathers of this process (rgbm_comm_gather_stats)
struct GatherStats { std::atomic<long long> bytes{0}, ns{0}, calls{0}; };
GatherStats& gather_stats();

// the RGBM_ERR_* code an exception stands for
inline int status_of(const std::exception& e) {
    if (dynamic_cast<const std::invalid_argument*>(&e)) return RGBM_ERR_PARAM;
    if (dynamic_cast<const std::out_of_range*>(&e)) return RGBM_ERR_LABEL;
    if (dynamic_cast<const std::domain_error*>(&e)) return RGBM_ERR_NO_DEVICE;
    if (dynamic_cast<const std::bad_alloc*>(&e)) return RGBM_ERR_NOMEM;
    return RGBM_ERR_HIP;
}

// C++ exceptions never cross the C ABI: every entry point runs its body through this
template <typename Fn>
int guarded(Fn&& fn) {
    try { return fn(); }
    catch (const std::exception& e) { const int code = status_of(e); return fail(code, code == RGBM_ERR_NOMEM ? "out of host memory" : e.what()); }
}

// class probabilities [n][num_class] (row-major, device) of the n rows of a device code block [c][n]; defined in rgbm.hip
void predict_proba_device(const rgbm_model* m, int device, hipStream_t s, const int32_t* d_codes, long long n, const int32_t* d_feat_cols,
                          double* d_proba);
void model_shape(const rgbm_model* m, int32_t* objective, int32_t* num_class, int32_t* n_features);

// what the distinct-row view remembers as "cannot": the two refusals of the distinct pass that depend on the table's size alone, and a refused allocation
struct distinct_cannot : std::invalid_argument { using std::invalid_argument::invalid_argument; };
struct device_oom : std::runtime_error { using std::runtime_error::runtime_error; };

// the body of rgbm_table_distinct_rows (rgbm_distinct.hip), shared with the distinct-row view; throws.  inverse_host_out [n] may be null: then no
// inverse is computed and nothing but two counters leaves the device.  max_rows >= 0: a result of more rows is counted (rows) but not made (tab stays null)
struct DistinctOut { std::unique_ptr<rgbm_table> tab; int64_t rows = 0; };
DistinctOut distinct_rows_device(const rgbm_table& t, int64_t* inverse_host_out, int64_t max_rows);

}  // namespace rgh

// The DISTINCT-ROW VIEW of a table (rgbm_table_train trains on it wherever the model is the same bytes and it pays): the table that
// rgbm_table_distinct_rows makes, built lazily by the first training call that wants it, and the outcome of that build.
enum { RGBM_VIEW_NONE = 0, RGBM_VIEW_BUILT = 1, RGBM_VIEW_NOT_WORTH = 2, RGBM_VIEW_CANNOT = 3 };
struct rgbm_distinct_view {
    std::mutex mu;                               // its own mutex, never prep_mu (the distinct pass takes prep_mu itself); held for the whole build: concurrent callers wait
    uint64_t version = 0;                        // of the table's contents; every writing entry point bumps it (rgh::ViewWrite)
    int state = RGBM_VIEW_NONE; int64_t rows = 0; int64_t builds = 0;
    std::shared_ptr<const rgbm_table> tab;       // state BUILT only; a fit in flight holds its own reference
    std::vector<uint64_t> refused;               // fit shapes the multiplicity trainer refused on this version (rgbm.hip: view_shape_key)
    void drop() { ++version; state = RGBM_VIEW_NONE; rows = 0; tab.reset(); refused.clear(); }
};

// the label-encoded table, resident in HBM: int32 codes [c][n], column-major, -1 = NULL
struct rgbm_table {
    int device = 0; int64_t n = 0; int32_t c = 0;
    std::vector<int32_t> n_codes;
    std::vector<std::vector<double>> col_values;   // NUMERIC columns: the ascending distinct values behind the codes (rgbm_table_set_column_values)
    std::vector<uint8_t> col_kind;                 // 1 = CATEGORICAL column (rgbm_table_set_column_kind): unseen categories are missing for a model
    rgh::DevBuf<int32_t> codes;
    // rows with MULTIPLICITIES (rgbm_table_set_row_multiplicity): row i stands for mult[i] (1..255) identical rows of a larger table -- every count,
    // every gradient sum and every coarse magnitude of a training call weighs it so; the model is byte for byte the one the expanded table gives
    rgh::DevBuf<uint8_t> mult; bool has_mult = false; int64_t mult_total = 0;
    // result of the last rgbm_table_detect_* call (rgbm_prep.hip, rgbm_dc.hip): cells (row, column), device resident
    rgh::DevBuf<long long> cell_rows; rgh::DevBuf<int32_t> cell_cols; int64_t n_cells = 0;
    uint64_t cell_version = 0;                     // bumped by whatever replaces the cell list (emit_to_table, rows_to_cells, no_cells)
    // the CELL SET (rgbm_cellset.hip): a bit matrix of cs_n_cols x 64 * ceil(n / 4096) words in the compaction's ballot layout, its columns
    // (cs_d_cols [cs_n_cols]; cs_d_pos [c]: column -> position, -1 = not in the set) and the codes of the last emit, which are the codes of
    // the cell list while cell_version is still that emit's
    rgh::DevBuf<unsigned long long> cs_bits; rgh::DevBuf<int32_t> cs_d_cols, cs_d_pos, cs_codes;
    int32_t cs_n_cols = 0; bool cs_open = false, cs_emitted = false; uint64_t cs_emit_version = 0;
    std::vector<int32_t> cs_cols;                  // the set's columns on the host (rgbm_table_cellset_drop_weak looks its target up), under prep_mu
    // stream + scratch of the relational steps (rgbm_prep.h: table_stream, enum Scr), kept with the table: a hipMalloc / hipFree / stream
    // creation per call costs more than the kernels (one call at a time per table, as the header says)
    // Python threads share one table (the folds of a hyper-parameter search gather from the training table, ctypes drops the
    // GIL): every entry point that touches the stream / scratch / cell list holds prep_mu from the first use to its final synchronise.
    mutable std::mutex prep_mu;
    mutable hipStream_t stream = nullptr;
    mutable rgh::DevBuf<unsigned char> scratch[12];
    // result of the last rgbm_table_pair_counts call, kept on the device for rgbm_table_cell_domains: the dense joint tables
    // (pair p at pc_off[p], (pc_dx[p] + 1) x (pc_dy[p] + 1) cells, NULL in the last slot of each side), the bins per column and the LUTs
    mutable rgh::DevBuf<unsigned long long> pc_counts; mutable rgh::DevBuf<int32_t> pc_luts; mutable rgh::DevBuf<long long> pc_lut_off;
    mutable rgh::DevBuf<int32_t> pc_bins;
    mutable std::vector<int32_t> pc_x, pc_y, pc_dx, pc_dy, pc_nbins; mutable std::vector<long long> pc_off; mutable std::vector<uint8_t> pc_has_lut;
    // the plan of that call, as its planner made it (rgbm_table_pair_counts_report): per pair {group (-1 = the HBM kernel), slot of x, slot of y};
    // {groups, cells of the largest group, grid x, rows per workgroup}
    mutable std::vector<int32_t> pc_plan; mutable long long pc_plan_head[4] = {0, 0, 0, 0};
    // the route of every right-hand side of the last successful rgbm_table_fd_measures call (0 = LDS counters, 1 = hash tables), under prep_mu
    mutable std::vector<int32_t> fd_routes;
    // the route of every column of the last successful rgbm_table_recode call (0 = identity, 1 = LDS LUT, 2 = global LUT), under prep_mu
    mutable std::vector<int32_t> recode_routes;
    // the cluster of every row after the last rgbm_table_kmeans_assign call (int32 [n]); it leaves the device through rgbm_table_kmeans_read
    mutable rgh::DevBuf<int32_t> km_assign; mutable bool km_valid = false;
    mutable rgbm_distinct_view view;
    ~rgbm_table() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace rgh {
// Every entry point that can write what the distinct-row view was made from -- codes, n_codes, column kinds or values, multiplicities --
// holds one of these for the length of the call: the view is dropped and the version bumped when the call begins and again when it ends,
// so a fit that starts in between (which the caller must not do anyway) never leaves a view of half-written codes behind.  Declared BEFORE
// the call takes prep_mu: view.mu is never taken under prep_mu.  The entry points:
//   rgbm_table_repair_chain, rgbm_table_repair_chain_gather, rgbm_table_null_cells, rgbm_table_cellset_null, rgbm_table_write_cells, rgbm_table_rule_fill,
//   rgbm_table_set_column_kind, rgbm_table_set_column_values, rgbm_table_set_row_multiplicity.
// (rgbm_table_repair_pmf and rgbm_table_repair_pmf_weighted return candidates and write no cell: they are not in the list.)
struct ViewWrite {
    const rgbm_table* t;
    static void drop(const rgbm_table* t) { if (t) { std::lock_guard<std::mutex> lk(t->view.mu); t->view.drop(); } }
    explicit ViewWrite(const rgbm_table* t_) : t(t_) { drop(t); }
    ViewWrite(const ViewWrite&) = delete; ViewWrite& operator=(const ViewWrite&) = delete;
    ~ViewWrite() { drop(t); }
};
}  // namespace rgh
