// rgbm_comm.hip -- the communicator of the CALLING THREAD behind row-sharded multi-GPU training and the C1 / C2 exchanges of a multi-GPU job:
// the two transports (RCCL, the in-process thread group), the fusion group, the watchdog, and every rgbm_comm_*, rgbm_fusion_* and
// rgbm_local_group_* entry point of include/rgbm.h.  Host side only but for k_sum_ranks (the thread group's sum).  What the trainer and the
// chained repair (rgbm.hip) use of it is declared in rgbm_host.h.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "rgbm_host.h"

namespace {
using rgh::fail; using rgh::DevBuf; using rgh::use_device; using rgh::StreamGuard; using rgh::guarded;
using rgh::AR_I64; using rgh::AR_U32;

// ---------------------------------------------------------------------------------------------
// Row-sharded multi-GPU training (DESIGN.md "Multi-GPU"): every rank holds a row shard of the table and grows the
// SAME trees; the only exchanges are integer all-reduces of (a) the code counts used for binning, (b) the built
// children's histograms after each level pass and (c) the exact child row counts.  Sums are exact integers, so the
// model is bit-identical to single-GPU training for any number of ranks and any row split.
// Two transports: RCCL (one process per GPU, all-reduce enqueued on the training stream: no host round trip) and an
// in-process thread group (one rank per host thread on one device) that exists so the sharding logic can be
// verified on a single GPU.
// ---------------------------------------------------------------------------------------------
struct LocalGroup {
    int nranks = 0, device = 0;
    std::mutex mu; std::condition_variable cv;
    int arrived = 0; long long generation = 0;
    std::vector<void*> ptr;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const long long gen = generation;
        if (++arrived == nranks) { arrived = 0; ++generation; cv.notify_all(); }
        else cv.wait(lk, [&] { return generation != gen; });
    }
};

struct Fusion;
struct Comm {
    int kind = 0;   // 0 none, 1 RCCL, 2 local thread group, 3 member of a fusion group (the rank's communicator lives in the group)
    int rank = 0, nranks = 1;
    ncclComm_t nccl = nullptr;
    LocalGroup* lg = nullptr;
    void* tmp = nullptr; size_t tmp_bytes = 0;
    Fusion* fusion = nullptr; int member = 0;      // kind 3
};
thread_local Comm g_comm;


// ---------------------------------------------------------------------------------------------
// Fusion group (round 5): the row-sharded training calls of ONE rank that run at the same time -- one host thread and one HIP stream
// each -- and exchange in LOCK STEP.  Every row-sharded training call makes the same sequence of collectives (code counts once, then per
// boosting iteration one all-reduce per level and one of the deepest counts: the sequence is fixed by the parameters, not by the
// data), so the i-th collective of every member is carried by ONE all-reduce of the rank's communicator over the members' buffers laid
// side by side: a member records an event behind its producers and waits at a host barrier; the last one to arrive copies all parts
// into a staging buffer on the group's stream, enqueues the collective and the copies back and records a `done` event; every member's
// stream then waits for that event.  Nothing synchronises with the device: the host threads only meet at enqueue time.
// What it buys: the row-sharded targets of a rank trained one after another on the thread that owns the
// communicator -- the in-rank concurrency (22 % at N = 1) was gone exactly where every target is row-sharded, and a job paid 8
// collectives per target-iteration.  Now they overlap like the target-sharded ones and a rank issues 8 collectives per iteration of
// ALL its row-sharded targets.  The members' order inside the fused buffer is their index, so it is the same on every rank.
// A member that fails breaks the group: the others raise at their next collective (and the RCCL communicator is aborted, as before).
// ---------------------------------------------------------------------------------------------
struct Fusion {
    static constexpr int MAX_MEMBERS = 64;
    Comm comm;                  // the rank's communicator (moved in by rgbm_fusion_create, moved back by rgbm_fusion_free)
    int device = 0;
    int n = 0;                  // members still taking part
    int n_members = 0;          // members the group was created for (rgbm_fusion_join checks the index against it)
    bool joined[MAX_MEMBERS] = {};
    std::mutex mu; std::condition_variable cv;
    int arrived = 0; long long gen = 0; bool broken = false; std::string why;
    struct Part { void* buf = nullptr; size_t count = 0; int type = 0; hipStream_t s = nullptr; hipEvent_t ready = nullptr; bool in = false; } part[MAX_MEMBERS];
    void* stage = nullptr; size_t stage_bytes = 0;
    hipStream_t cs = nullptr; hipEvent_t done = nullptr;
    long long collectives = 0, fused_parts = 0;    // statistics
};

void all_reduce_on(Comm& c, void* buf, size_t count, int type, hipStream_t s);

// RGBM_COMM_TIMEOUT_S: seconds without progress after which a collective is given up (default 600; read once)
double comm_timeout_s() {
    static const double limit = [] { const char* e = getenv("RGBM_COMM_TIMEOUT_S"); double v = e ? atof(e) : 600.0; return v > 0.0 ? v : 600.0; }();
    return limit;
}

// the collective of one step for every member that is parked in it (called with f->mu held, by the last member to arrive -- or by a member
// that leaves while all the remaining ones are parked).  Members may be at different points of their sequences (one is counting codes for
// its next target while another is in the middle of an iteration): the parts are grouped by element type, one all-reduce per type present,
// in a fixed type order -- the same on every rank, because which member takes part in the k-th step only depends on the sequences.
void fusion_run_step_locked(Fusion* f) {
    try {
        for (int type = 0; type < 3; ++type) {
            const size_t esz = type == AR_I64 ? 8 : 4;
            size_t total = 0; int nparts = 0;
            for (int j = 0; j < Fusion::MAX_MEMBERS; ++j) if (f->part[j].in && f->part[j].type == type) { total += f->part[j].count; ++nparts; }
            if (nparts == 0) continue;
            if (total * esz > f->stage_bytes) {
                HIPCHK(hipStreamSynchronize(f->cs));
                if (f->stage) (void)hipFree(f->stage);
                f->stage_bytes = std::max<size_t>(total * esz * 2, 1 << 20);
                HIPCHK(hipMalloc(&f->stage, f->stage_bytes));
            }
            size_t off = 0;
            for (int j = 0; j < Fusion::MAX_MEMBERS; ++j) {
                Fusion::Part& q = f->part[j];
                if (!q.in || q.type != type) continue;
                HIPCHK(hipStreamWaitEvent(f->cs, q.ready, 0));
                if (q.count) HIPCHK(hipMemcpyAsync(static_cast<char*>(f->stage) + off * esz, q.buf, q.count * esz, hipMemcpyDeviceToDevice, f->cs));
                off += q.count;
            }
            all_reduce_on(f->comm, f->stage, total, type, f->cs);
            off = 0;
            for (int j = 0; j < Fusion::MAX_MEMBERS; ++j) {
                Fusion::Part& q = f->part[j];
                if (!q.in || q.type != type) continue;
                if (q.count) HIPCHK(hipMemcpyAsync(q.buf, static_cast<char*>(f->stage) + off * esz, q.count * esz, hipMemcpyDeviceToDevice, f->cs));
                off += q.count; f->fused_parts += 1;
            }
            f->collectives += 1;
        }
        for (int j = 0; j < Fusion::MAX_MEMBERS; ++j) f->part[j].in = false;
        HIPCHK(hipEventRecord(f->done, f->cs));
    } catch (const std::exception& e) { f->broken = true; f->why = e.what(); }
    f->arrived = 0; ++f->gen; f->cv.notify_all();
}

// one fused collective; called by every member with its own buffer
void fused_all_reduce(Fusion* f, int me, void* buf, size_t count, int type, hipStream_t s) {
    Fusion::Part& mine = f->part[me];
    if (!mine.ready) HIPCHK(hipEventCreateWithFlags(&mine.ready, hipEventDisableTiming));
    HIPCHK(hipEventRecord(mine.ready, s));
    std::unique_lock<std::mutex> lk(f->mu);
    if (f->broken) throw std::runtime_error("fusion group: a concurrent row-sharded training call of this rank failed (" + f->why + ")");
    mine.buf = buf; mine.count = count; mine.type = type; mine.s = s; mine.in = true;
    const long long gen = f->gen;
    if (++f->arrived >= f->n) fusion_run_step_locked(f);
    else {
        // bounded: a member of this rank that never arrives and never leaves -- its thread died before its next collective -- must not
        // park the others (and, through them, the peer ranks) for ever: after RGBM_COMM_TIMEOUT_S the group is broken and everybody raises
        const double limit = comm_timeout_s();
        if (!f->cv.wait_for(lk, std::chrono::duration<double>(limit), [&] { return f->gen != gen || f->broken; })) {
            f->broken = true; f->why = "a member of this rank did not reach its next collective within " + std::to_string((int)limit) + " s";
            if (f->comm.kind == 1 && f->comm.nccl) { (void)ncclCommAbort(f->comm.nccl); f->comm.nccl = nullptr; f->comm.kind = 0; }
            f->cv.notify_all();
        }
    }
    if (f->broken) throw std::runtime_error("fusion group: a concurrent row-sharded training call of this rank failed (" + f->why + ")");
    HIPCHK(hipStreamWaitEvent(s, f->done, 0));
}

// a member is done (its training call returned or failed): the others go on among themselves
void fusion_leave(bool failed, const char* why) {
    Comm& c = g_comm;
    if (c.kind != 3 || !c.fusion) return;
    Fusion* f = c.fusion;
    {
        std::lock_guard<std::mutex> lk(f->mu);
        f->part[c.member].in = false;
        if (failed && !f->broken) { f->broken = true; f->why = why ? why : "unknown error"; if (f->comm.kind == 1 && f->comm.nccl) { (void)ncclCommAbort(f->comm.nccl); f->comm.nccl = nullptr; f->comm.kind = 0; } }
        f->n -= 1;
        if (f->broken) f->cv.notify_all();
        else if (f->n > 0 && f->arrived >= f->n) fusion_run_step_locked(f);     // the remaining members are all parked in their next step: it is theirs alone
    }
    g_comm = Comm();
}

}  // namespace

// Fail-safe for the RCCL transport.  A rank that dies (or throws) in the middle of a training call never enqueues its next
// all-reduce, and its peers would sit in theirs for ever.  So (a) a rank that fails ABORTS its communicator before the error
// leaves the library (comm_abort_on_failure), and (b) every rank waits for its training stream through a watchdog instead of
// a blocking synchronise: it polls the stream, asks RCCL for asynchronous errors and gives up after RGBM_COMM_TIMEOUT_S seconds
// (default 600) without progress -- then it aborts its own communicator (which takes the stuck collective kernel off the stream)
// and raises.  After an abort the thread has no communicator: the caller falls back to target sharding (repair/dist.py).
void rgh::comm_abort() {
    Comm& c = g_comm;
    if (c.kind == 1 && c.nccl) { (void)ncclCommAbort(c.nccl); c.nccl = nullptr; c.kind = 0; c.nranks = 1; c.rank = 0; }
    if (c.kind == 3 && c.fusion) fusion_leave(true, "a member's stream failed or timed out inside a collective");
}

void rgh::stream_sync_watchdog(hipStream_t s) {
    Comm& c = g_comm;
    const bool fused_rccl = c.kind == 3 && c.fusion && c.fusion->comm.kind == 1;
    if (c.kind != 1 && !fused_rccl) { HIPCHK(hipStreamSynchronize(s)); return; }
    const double limit = comm_timeout_s();
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(s);
        if (q == hipSuccess) return;
        if (q != hipErrorNotReady) { (void)hipGetLastError(); comm_abort(); throw std::runtime_error(std::string("training stream failed during a collective: ") + hipGetErrorString(q)); }
        ncclResult_t ae = ncclSuccess; bool have_ae = false;
        if (fused_rccl) {
            // the group's state belongs to its mutex: another member may be leaving right now -- writing `why`, aborting the communicator
            // and clearing the handle -- so the flag, the text and the asynchronous-error query are taken under the lock
            bool broken; std::string w;
            {
                std::lock_guard<std::mutex> lk(c.fusion->mu);
                broken = c.fusion->broken; if (broken) w = c.fusion->why;
                if (!broken && c.fusion->comm.nccl) have_ae = ncclCommGetAsyncError(c.fusion->comm.nccl, &ae) == ncclSuccess;
            }
            if (broken) { comm_abort(); throw std::runtime_error("fusion group broken: " + w); }
        } else if (c.nccl) have_ae = ncclCommGetAsyncError(c.nccl, &ae) == ncclSuccess;
        if (have_ae && ae != ncclSuccess && ae != ncclInProgress) {
            const std::string what = ncclGetErrorString(ae);
            comm_abort();
            throw std::runtime_error("RCCL reported an asynchronous error (a peer rank failed?): " + what);
        }
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (waited > limit) {
            comm_abort();
            throw std::runtime_error("row-sharded training: no progress for " + std::to_string((int)limit) + " s inside a collective (a peer rank is gone); communicator aborted");
        }
        std::this_thread::sleep_for(std::chrono::microseconds(waited < 0.05 ? 50 : 1000));
    }
}

int rgh::comm_kind() { return g_comm.kind; }
int rgh::comm_rank() { return g_comm.rank; }
int rgh::comm_nranks() { return g_comm.nranks; }

namespace {
struct PtrList { const void* p[16]; };
template <typename T>
__global__ void k_sum_ranks(PtrList src, int n, T* __restrict__ out, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    T acc = 0;
    for (int r = 0; r < n; ++r) acc += reinterpret_cast<const T*>(src.p[r])[i];
    out[i] = acc;
}

void all_reduce_on(Comm& c, void* buf, size_t count, int type, hipStream_t s) {
    if (c.kind == 0 || count == 0) return;
    const size_t esz = type == AR_I64 ? 8 : 4;
    if (c.kind == 1) {
        const ncclDataType_t dt = type == AR_I64 ? ncclInt64 : (type == AR_U32 ? ncclUint32 : ncclInt32);
        ncclResult_t r = ncclAllReduce(buf, buf, count, dt, ncclSum, c.nccl, s);
        if (r != ncclSuccess) throw std::runtime_error(std::string("ncclAllReduce failed: ") + ncclGetErrorString(r));
        return;
    }
    LocalGroup* g = c.lg;
    if (c.tmp_bytes < count * esz) { if (c.tmp) (void)hipFree(c.tmp); HIPCHK(hipMalloc(&c.tmp, count * esz)); c.tmp_bytes = count * esz; }
    HIPCHK(hipStreamSynchronize(s));
    { std::lock_guard<std::mutex> lk(g->mu); g->ptr[c.rank] = buf; }
    g->barrier();
    PtrList pl; for (int r = 0; r < g->nranks; ++r) pl.p[r] = g->ptr[r];
    const unsigned blocks = (unsigned)((count + 255) / 256);
    if (type == AR_I64) hipLaunchKernelGGL(k_sum_ranks<long long>, dim3(blocks), dim3(256), 0, s, pl, g->nranks, (long long*)c.tmp, count);
    else if (type == AR_U32) hipLaunchKernelGGL(k_sum_ranks<unsigned int>, dim3(blocks), dim3(256), 0, s, pl, g->nranks, (unsigned int*)c.tmp, count);
    else hipLaunchKernelGGL(k_sum_ranks<int>, dim3(blocks), dim3(256), 0, s, pl, g->nranks, (int*)c.tmp, count);
    HIPCHK(hipStreamSynchronize(s));
    g->barrier();                                   // everyone has read every buffer
    HIPCHK(hipMemcpyAsync(buf, c.tmp, count * esz, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    g->barrier();
}

}  // namespace

// in-place sum all-reduce of `count` elements on stream s
void rgh::all_reduce(void* buf, size_t count, int type, hipStream_t s) {
    Comm& c = g_comm;
    if (c.kind == 3) { fused_all_reduce(c.fusion, c.member, buf, count, type, s); return; }     // (also with count == 0: every member takes part in every step)
    all_reduce_on(c, buf, count, type, s);
}

// all-gather of equal-sized device blocks over the calling thread's own communicator (not from inside a fusion group): recv = [nranks][bytes].
// RCCL: ncclAllGather on the library's communicator, enqueued on s; thread group: every rank copies every rank's block (device copies
// between two barriers); no communicator: a copy.  What the C1 / C2 exchanges of a multi-GPU job ride on (model blobs, repaired cells).
rgh::GatherStats& rgh::gather_stats() { static GatherStats g; return g; }
void rgh::all_gather_on(const void* send, void* recv, size_t bytes, hipStream_t s) {
    Comm& c = g_comm;
    if (c.kind == 3) throw std::invalid_argument("all-gather from inside a fusion group");
    if (bytes == 0) return;
    if (c.kind == 0 || c.nranks <= 1) { if (c.kind != 1) { HIPCHK(hipMemcpyAsync(recv, send, bytes, hipMemcpyDeviceToDevice, s)); return; } }
    if (c.kind == 1) {
        ncclResult_t r = ncclAllGather(send, recv, bytes, ncclUint8, c.nccl, s);
        if (r != ncclSuccess) throw std::runtime_error(std::string("ncclAllGather failed: ") + ncclGetErrorString(r));
        return;
    }
    LocalGroup* g = c.lg;
    HIPCHK(hipStreamSynchronize(s));
    { std::lock_guard<std::mutex> lk(g->mu); g->ptr[c.rank] = const_cast<void*>(send); }
    g->barrier();
    for (int r = 0; r < g->nranks; ++r) HIPCHK(hipMemcpyAsync(static_cast<char*>(recv) + (size_t)r * bytes, g->ptr[r], bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    g->barrier();                                   // everyone has read every block
}

extern "C" {

// ---- row-sharded multi-GPU training: communicator of the CALLING THREAD --------------------------------------
RGBM_EXPORT int rgbm_comm_unique_id(void* id_out) {
    if (!id_out) return fail(RGBM_ERR_ARG, "rgbm_comm_unique_id: bad argument");
    return guarded([&]() {
        static_assert(sizeof(ncclUniqueId) <= RGBM_COMM_ID_BYTES, "ncclUniqueId larger than RGBM_COMM_ID_BYTES");
        ncclUniqueId id; memset(&id, 0, sizeof(id));
        ncclResult_t r = ncclGetUniqueId(&id);
        if (r != ncclSuccess) throw std::runtime_error(std::string("ncclGetUniqueId failed: ") + ncclGetErrorString(r));
        memset(id_out, 0, RGBM_COMM_ID_BYTES); memcpy(id_out, &id, sizeof(id));
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_comm_init(const void* id, int32_t rank, int32_t nranks, int32_t device_id) {
    if (!id || rank < 0 || nranks < 1 || rank >= nranks) return fail(RGBM_ERR_ARG, "rgbm_comm_init: bad argument");
    return guarded([&]() {
        if (g_comm.kind != 0) throw std::invalid_argument("rgbm_comm_init: this thread already has a communicator");
        use_device(device_id);
        ncclUniqueId uid; memcpy(&uid, id, sizeof(uid));
        ncclComm_t c = nullptr;
        ncclResult_t r = ncclCommInitRank(&c, nranks, uid, rank);
        if (r != ncclSuccess) throw std::runtime_error(std::string("ncclCommInitRank failed: ") + ncclGetErrorString(r));
        g_comm.kind = 1; g_comm.rank = rank; g_comm.nranks = nranks; g_comm.nccl = c;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_local_group_create(int32_t nranks, int32_t device_id, void** group_out) {
    if (!group_out || nranks < 1 || nranks > 16) return fail(RGBM_ERR_ARG, "rgbm_local_group_create: bad argument (1..16 ranks)");
    return guarded([&]() {
        use_device(device_id);
        LocalGroup* g = new LocalGroup(); g->nranks = nranks; g->device = device_id; g->ptr.assign(nranks, nullptr);
        *group_out = g;
        return RGBM_OK;
    });
}

RGBM_EXPORT void rgbm_local_group_free(void* group) { delete static_cast<LocalGroup*>(group); }

RGBM_EXPORT int rgbm_comm_init_local(void* group, int32_t rank) {
    LocalGroup* g = static_cast<LocalGroup*>(group);
    if (!g || rank < 0 || rank >= g->nranks) return fail(RGBM_ERR_ARG, "rgbm_comm_init_local: bad argument");
    return guarded([&]() {
        if (g_comm.kind != 0) throw std::invalid_argument("rgbm_comm_init_local: this thread already has a communicator");
        use_device(g->device);
        g_comm.kind = 2; g_comm.rank = rank; g_comm.nranks = g->nranks; g_comm.lg = g;
        return RGBM_OK;
    });
}

// ---- fusion group: concurrent row-sharded training calls of one rank, one collective per step for all of them (see struct Fusion)
RGBM_EXPORT int rgbm_fusion_create(int32_t n_members, void** out) {
    if (!out || n_members < 1 || n_members > Fusion::MAX_MEMBERS) return fail(RGBM_ERR_ARG, "rgbm_fusion_create: bad argument (1..64 members)");
    return guarded([&]() {
        if (g_comm.kind != 1 && g_comm.kind != 2) throw std::invalid_argument("rgbm_fusion_create: the calling thread has no communicator (rgbm_comm_init)");
        std::unique_ptr<Fusion> f(new Fusion());
        HIPCHK(hipGetDevice(&f->device));
        HIPCHK(hipStreamCreateWithFlags(&f->cs, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&f->done, hipEventDisableTiming));
        f->n = n_members; f->n_members = n_members;
        f->comm = g_comm; g_comm = Comm();         // the communicator lives in the group until rgbm_fusion_free hands it back
        *out = f.release();
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_fusion_join(void* fusion, int32_t member) {
    Fusion* f = static_cast<Fusion*>(fusion);
    if (!f || member < 0 || member >= Fusion::MAX_MEMBERS) return fail(RGBM_ERR_ARG, "rgbm_fusion_join: bad argument");
    return guarded([&]() {
        if (g_comm.kind != 0) throw std::invalid_argument("rgbm_fusion_join: this thread already has a communicator");
        {
            std::lock_guard<std::mutex> lk(f->mu);
            if (member >= f->n_members) throw std::invalid_argument("rgbm_fusion_join: member index beyond the members the group was created for");
            if (f->joined[member]) throw std::invalid_argument("rgbm_fusion_join: this member index is taken");
            f->joined[member] = true;
        }
        use_device(f->device);
        g_comm.kind = 3; g_comm.rank = f->comm.rank; g_comm.nranks = f->comm.nranks; g_comm.fusion = f; g_comm.member = member;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_fusion_leave(int32_t failed) {
    fusion_leave(failed != 0, "a member reported a failure");
    return RGBM_OK;
}

RGBM_EXPORT int rgbm_fusion_info(void* fusion, int64_t* info /* [4] = {collectives issued, member parts carried, members still in, broken} */) {
    Fusion* f = static_cast<Fusion*>(fusion);
    if (!f || !info) return fail(RGBM_ERR_ARG, "rgbm_fusion_info: bad argument");
    std::lock_guard<std::mutex> lk(f->mu);
    info[0] = f->collectives; info[1] = f->fused_parts; info[2] = f->n; info[3] = f->broken ? 1 : 0;
    return RGBM_OK;
}

RGBM_EXPORT int rgbm_fusion_free(void* fusion) {
    Fusion* f = static_cast<Fusion*>(fusion);
    if (!f) return RGBM_OK;
    return guarded([&]() {
        (void)hipSetDevice(f->device);
        if (f->cs) { (void)hipStreamSynchronize(f->cs); (void)hipStreamDestroy(f->cs); }
        if (f->done) (void)hipEventDestroy(f->done);
        for (auto& q : f->part) if (q.ready) (void)hipEventDestroy(q.ready);
        if (f->stage) (void)hipFree(f->stage);
        // the communicator goes back to the calling thread (unless that thread has one already, or the group broke and aborted it)
        if (g_comm.kind == 0 && (f->comm.kind == 1 || f->comm.kind == 2)) g_comm = f->comm;
        else { if (f->comm.kind == 1 && f->comm.nccl) (void)ncclCommDestroy(f->comm.nccl); if (f->comm.tmp) (void)hipFree(f->comm.tmp); }
        delete f;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_comm_finalize(void) {
    if (g_comm.kind == 3) { fusion_leave(false, nullptr); return RGBM_OK; }      // a member thread: leave the group (the communicator is the group's)
    if (g_comm.kind == 1 && g_comm.nccl) (void)ncclCommDestroy(g_comm.nccl);
    if (g_comm.tmp) (void)hipFree(g_comm.tmp);
    g_comm = Comm();
    return RGBM_OK;
}

// ---- C1 / C2 of a multi-GPU job on the library's OWN communicator ("C1 / C2 on device buffers and one communicator"): the
// serialised models (Spark broadcast, python/repair/model.py:1069) and the repaired cells (the union of the UDF outputs, model.py:1142) are
// all-gathered by ncclAllGather over xGMI on the communicator the row-sharded trainer uses -- a rank holds ONE RCCL communicator; torch's process
// group only carries control traffic (gloo).  Equal-sized blocks: the callers pad to the largest rank (sizes first, through the same path).
static void gather_host_blocks(const void* send, size_t my_bytes, size_t block_bytes, void* recv) {
    const int nr = std::max(1, g_comm.nranks);
    StreamGuard sg; hipStream_t s = sg.s;
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<unsigned char> d_send(std::max<size_t>(block_bytes, 1)), d_recv(std::max<size_t>(block_bytes, 1) * (size_t)nr);
    d_send.zero(s);
    if (my_bytes) HIPCHK(hipMemcpyAsync(d_send.p, send, my_bytes, hipMemcpyHostToDevice, s));
    rgh::all_gather_on(d_send.p, d_recv.p, block_bytes, s);
    if (block_bytes) HIPCHK(hipMemcpyAsync(recv, d_recv.p, block_bytes * (size_t)nr, hipMemcpyDeviceToHost, s));
    rgh::stream_sync_watchdog(s);
    rgh::GatherStats& G = rgh::gather_stats();
    G.bytes += (long long)(block_bytes * (size_t)nr); G.calls += 1;
    G.ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}

RGBM_EXPORT int rgbm_comm_all_gather_sizes(const int64_t* mine, int32_t n, int64_t* all /* [nranks][n] */) {
    if (!mine || !all || n < 1) return fail(RGBM_ERR_ARG, "rgbm_comm_all_gather_sizes: bad argument");
    return guarded([&]() { gather_host_blocks(mine, (size_t)n * 8, (size_t)n * 8, all); return RGBM_OK; });
}

RGBM_EXPORT int rgbm_comm_all_gather_bytes(const void* send, int64_t my_bytes, int64_t block_bytes, void* recv /* [nranks][block_bytes] */) {
    if (my_bytes < 0 || block_bytes < my_bytes || !recv || (my_bytes > 0 && !send)) return fail(RGBM_ERR_ARG, "rgbm_comm_all_gather_bytes: bad argument");
    return guarded([&]() { gather_host_blocks(send, (size_t)my_bytes, (size_t)block_bytes, recv); return RGBM_OK; });
}

RGBM_EXPORT int rgbm_comm_gather_stats(int64_t* out /* [3] = {bytes received by all-gathers of this process, nanoseconds spent in them, collectives} */) {
    if (!out) return fail(RGBM_ERR_ARG, "rgbm_comm_gather_stats: bad argument");
    rgh::GatherStats& G = rgh::gather_stats();
    out[0] = G.bytes.load(); out[1] = G.ns.load(); out[2] = G.calls.load();
    return RGBM_OK;
}

RGBM_EXPORT int rgbm_comm_info(int32_t* info) {
    if (!info) return fail(RGBM_ERR_ARG, "rgbm_comm_info: bad argument");
    info[0] = g_comm.kind; info[1] = g_comm.rank; info[2] = g_comm.nranks;     // (kind 3: member of a fusion group)
    return RGBM_OK;
}

// ranks the calling thread's RCCL communicator really spans (ncclCommCount), 1 for no communicator: what a multi-GPU job prints so that a
// silent fall-back to fewer ranks is visible in its result line
RGBM_EXPORT int rgbm_comm_count(int32_t* n_out) {
    if (!n_out) return fail(RGBM_ERR_ARG, "rgbm_comm_count: bad argument");
    return guarded([&]() {
        *n_out = 1;
        const Comm& c = (g_comm.kind == 3 && g_comm.fusion) ? g_comm.fusion->comm : g_comm;
        if (c.kind == 2) *n_out = c.nranks;
        if (c.kind == 1 && c.nccl) {
            int n = 0;
            ncclResult_t r = ncclCommCount(c.nccl, &n);
            if (r != ncclSuccess) throw std::runtime_error(std::string("ncclCommCount failed: ") + ncclGetErrorString(r));
            *n_out = n;
        }
        return RGBM_OK;
    });
}

}  // extern "C"
