// rgbm_recode.hip -- a resident code table translated into another code space (a relational step; what the steps share is rgbm_prep.h):
//   table_recode          per column a look-up table from the table's codes to the codes of another dictionary (or none: the codes stay), a
//                         new resident table of the same rows, the cells that lost their value counted per column
//                         (a kept fit applied to a later table: repair/fitted.py; repair/recode_codes.py is the statement)
#include "rgbm_prep.h"

namespace {

using namespace rgh;

// ---------------------------------------------------------------------------------------------
// One streaming pass, k_recode, grid (row blocks, columns): 4 B read and 4 B written per cell, bound by memory.
//   - A column is [n] int32 at codes + j * n: with n % 4 != 0 its base is not 16-byte aligned for j >= 1.  A column is cut into a head of 0..3
//     cells up to the first 16-byte boundary, a body of int4, and a tail of 0..3 cells; the body is a grid-stride loop of 16-byte loads and
//     stores, RC_UNROLL per lane and step, head and tail are the first workgroup's.  Source and destination hold the same column of the same
//     shape, so one cut serves both; buffers that disagree modulo 16 B (no allocator of ours makes such) take 4 B per lane throughout.
//   - Three routes per column, uniform over the workgroup: 0 identity (an in-range code stays), 1 a LUT of at most RECODE_LDS_CODES entries
//     staged in LDS once per workgroup, 2 a larger LUT gathered from global memory (it is read-only and dictionary-sized: L2 and the
//     Infinity Cache serve it).
//   - RECODE_LDS_CODES = 4096: 16 KiB of LDS per workgroup of 256 threads, so eight workgroups -- all 32 waves of a CU -- fit its 160 KiB;
//     a larger stage would take occupancy from a kernel that hides its loads by nothing else.
//   - Unmapped cells (in range before, NULL after): a wave ballot per cell slot, summed per wave as a uniform count, one 64-bit atomic per
//     workgroup and column.  Integers: nothing depends on the order of arrival.
// ---------------------------------------------------------------------------------------------
constexpr int RECODE_LDS_CODES = 4096;    // LUT entries a workgroup stages in LDS (route 1 up to here)
constexpr int RC_UNROLL = 2;              // int4 per lane and grid-stride step of the body
constexpr int RC_WG_CELLS = 256 * 4 * RC_UNROLL * 4;    // cells a workgroup is given at least (grid sizing): four steps of its body
constexpr unsigned RC_MAX_BLOCKS = 256u * 8u;           // workgroups of a launch, over all columns

struct RcDesc { long long lut_off; int32_t n_in, n_out, route, pad; };

template <int ROUTE>
__device__ __forceinline__ int32_t rc_map(int32_t v, int32_t n_in, const int32_t* __restrict__ lut_g, const int32_t* lut_s, bool& lost) {
    lost = false;
    if ((unsigned)v >= (unsigned)n_in) return -1;          // NULL, or a code outside the dictionary (n_in <= 0: every code)
    if (ROUTE == 0) return v;
    const int32_t r = ROUTE == 1 ? lut_s[v] : lut_g[v];
    lost = r < 0;
    return r;
}

// the cells [0, n) of one column; every lane of the workgroup calls it.  Returns the wave's unmapped cells (the same number in every lane).
template <int ROUTE>
__device__ __forceinline__ unsigned rc_column(const int32_t* __restrict__ in, int32_t* __restrict__ out, long long n, int32_t n_in,
                                              const int32_t* __restrict__ lut_g, const int32_t* lut_s) {
    unsigned lost_cnt = 0;
    bool lost;
    const unsigned long long a_in = (unsigned long long)in, a_out = (unsigned long long)out;
    long long head = n, body = 0;                           // addresses that disagree modulo 16 B: all of it is "head", 4 B per lane
    if ((a_in & 15ull) == (a_out & 15ull)) {
        head = (long long)(((16ull - (a_in & 15ull)) & 15ull) >> 2);
        if (head > n) head = n;
        body = (n - head) >> 2;
    }
    const long long tail0 = head + body * 4;
    const int4* in4 = reinterpret_cast<const int4*>(in + head);
    int4* out4 = reinterpret_cast<int4*>(out + head);
    const long long step = (long long)gridDim.x * (256 * RC_UNROLL);
    for (long long base = (long long)blockIdx.x * (256 * RC_UNROLL); base < body; base += step) {      // uniform bounds: every lane reaches the ballots
        int4 v[RC_UNROLL];
#pragma unroll
        for (int u = 0; u < RC_UNROLL; ++u) {
            const long long i = base + (long long)u * 256 + threadIdx.x;
            v[u] = i < body ? in4[i] : make_int4(-1, -1, -1, -1);
        }
#pragma unroll
        for (int u = 0; u < RC_UNROLL; ++u) {
            const long long i = base + (long long)u * 256 + threadIdx.x;
            int4 r;
            r.x = rc_map<ROUTE>(v[u].x, n_in, lut_g, lut_s, lost); lost_cnt += (unsigned)__popcll(__ballot(lost));
            r.y = rc_map<ROUTE>(v[u].y, n_in, lut_g, lut_s, lost); lost_cnt += (unsigned)__popcll(__ballot(lost));
            r.z = rc_map<ROUTE>(v[u].z, n_in, lut_g, lut_s, lost); lost_cnt += (unsigned)__popcll(__ballot(lost));
            r.w = rc_map<ROUTE>(v[u].w, n_in, lut_g, lut_s, lost); lost_cnt += (unsigned)__popcll(__ballot(lost));
            if (i < body) out4[i] = r;
        }
    }
    // head and tail (three cells each at most when the body is wide; the whole column otherwise)
    for (long long base = (long long)blockIdx.x * 256; base < head; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        const int32_t r = rc_map<ROUTE>(i < head ? in[i] : -1, n_in, lut_g, lut_s, lost);
        lost_cnt += (unsigned)__popcll(__ballot(lost));
        if (i < head) out[i] = r;
    }
    if (blockIdx.x == 0 && tail0 < n) {                    // n - tail0 <= 3
        const long long i = tail0 + threadIdx.x;
        const int32_t r = rc_map<ROUTE>(i < n ? in[i] : -1, n_in, lut_g, lut_s, lost);
        lost_cnt += (unsigned)__popcll(__ballot(lost));
        if (i < n) out[i] = r;
    }
    return lost_cnt;
}

__global__ __launch_bounds__(256) void k_recode(const int32_t* __restrict__ codes, int32_t* __restrict__ out, long long n,
                                                const RcDesc* __restrict__ desc, const int32_t* __restrict__ luts,
                                                unsigned long long* __restrict__ unmapped) {
    __shared__ int32_t lut_s[RECODE_LDS_CODES];
    __shared__ unsigned wsum[4];
    const RcDesc d = desc[blockIdx.y];
    const int32_t* in = codes + (long long)blockIdx.y * n;
    int32_t* o = out + (long long)blockIdx.y * n;
    const int32_t* lut_g = luts + d.lut_off;               // route 0: lut_off is 0 and nothing is read
    unsigned lost_cnt;
    if (d.route == 1) {
        for (int i = threadIdx.x; i < d.n_in; i += 256) lut_s[i] = lut_g[i];       // n_in <= RECODE_LDS_CODES by the route's rule
        __syncthreads();
        lost_cnt = rc_column<1>(in, o, n, d.n_in, lut_g, lut_s);
    } else if (d.route == 2) {
        lost_cnt = rc_column<2>(in, o, n, d.n_in, lut_g, lut_s);
    } else {
        lost_cnt = rc_column<0>(in, o, n, d.n_in, lut_g, lut_s);
    }
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = lost_cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tot = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot) atomicAdd(&unmapped[blockIdx.y], tot);
    }
}

}  // namespace

extern "C" {

// scratch slots held together: COLS (the column descriptors) IN_COLS (the LUTs, one after the other) VALS (the unmapped counts)
RGBM_EXPORT int rgbm_table_recode(const rgbm_table* t, const int32_t* const* luts, const int32_t* n_codes_out, rgbm_table** out,
                                  int64_t* unmapped_out) {
    if (!t || !luts || !n_codes_out || !out) return fail(RGBM_ERR_ARG, "rgbm_table_recode: bad argument (a NULL table, LUT list, size list or output)");
    const int c = t->c;
    for (int j = 0; j < c; ++j) {
        if (n_codes_out[j] < 1)
            return fail(RGBM_ERR_ARG, "rgbm_table_recode: column " + std::to_string(j) + " has an output dictionary of " + std::to_string(n_codes_out[j]) + " codes (at least 1)");
        if (!luts[j] && n_codes_out[j] != t->n_codes[j])
            return fail(RGBM_ERR_ARG, "rgbm_table_recode: identity column " + std::to_string(j) + " changes its dictionary size (" +
                                          std::to_string(t->n_codes[j]) + " -> " + std::to_string(n_codes_out[j]) + ")");
    }
    for (int j = 0; j < c; ++j) {                          // on the host: a LUT is dictionary-sized
        if (!luts[j]) continue;
        for (int32_t v = 0; v < t->n_codes[j]; ++v)
            if (luts[j][v] < -1 || luts[j][v] >= n_codes_out[j])
                return fail(RGBM_ERR_ARG, "rgbm_table_recode: column " + std::to_string(j) + ", LUT entry " + std::to_string(v) + " = " +
                                              std::to_string(luts[j][v]) + " is outside [-1, " + std::to_string(n_codes_out[j]) + ")");
    }
    if (t->n >= (1ll << 31)) return fail(RGBM_ERR_PARAM, "rgbm_table_recode: a table of 2^31 rows or more");
    return guarded([&]() {
        const long long n = t->n;
        std::vector<RcDesc> desc((size_t)c);
        std::vector<int32_t> flat, routes((size_t)c);
        for (int j = 0; j < c; ++j) {
            const int32_t n_in = std::max<int32_t>(t->n_codes[j], 0);
            routes[j] = !luts[j] ? 0 : (n_in <= RECODE_LDS_CODES ? 1 : 2);
            desc[j] = RcDesc{luts[j] ? (long long)flat.size() : 0ll, n_in, n_codes_out[j], routes[j], 0};
            if (luts[j]) flat.insert(flat.end(), luts[j], luts[j] + n_in);
        }
        use_device(t->device);
        std::unique_ptr<rgbm_table> o(new rgbm_table());
        o->device = t->device; o->n = n; o->c = c; o->n_codes.assign(n_codes_out, n_codes_out + c);     // no kinds, values or multiplicities: another code space
        std::vector<unsigned long long> lost((size_t)std::max(c, 1), 0ull);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        if (n > 0 && c > 0) {
            hipStream_t s = table_stream(*t);
            o->codes.alloc((size_t)n * c);
            const RcDesc* d_desc = scr_upload<RcDesc>(*t, SCR_COLS, desc.data(), desc.size(), s);
            const int32_t* d_luts = scr_upload<int32_t>(*t, SCR_IN_COLS, flat.data(), flat.size(), s);
            unsigned long long* d_lost = scr<unsigned long long>(*t, SCR_VALS, (size_t)c);
            HIPCHK(hipMemsetAsync(d_lost, 0, (size_t)c * 8, s));
            const unsigned per_col = std::max(RC_MAX_BLOCKS / (unsigned)c, 1u);
            const unsigned nb = std::max(std::min(nblocks(n, RC_WG_CELLS), per_col), 1u);
            hipLaunchKernelGGL(k_recode, dim3(nb, (unsigned)c), dim3(256), 0, s, t->codes.p, o->codes.p, n, d_desc, d_luts, d_lost);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(lost.data(), d_lost, (size_t)c * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (unmapped_out) for (int j = 0; j < c; ++j) unmapped_out[j] = (int64_t)lost[j];
        t->recode_routes.swap(routes);
        *out = o.release();
        return RGBM_OK;
    });
}

// no device work: the route of every column of the table's last successful rgbm_table_recode call (-1 before any), then the LDS limit
RGBM_EXPORT int rgbm_table_recode_report(const rgbm_table* t, int32_t* out, int32_t c) {
    if (!out || c < 0 || (c > 0 && !t)) return fail(RGBM_ERR_ARG, "rgbm_table_recode_report: bad argument");
    if (t) {
        if (c != t->c) return fail(RGBM_ERR_ARG, "rgbm_table_recode_report: c is not the number of columns of the table");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        for (int j = 0; j < c; ++j) out[j] = (size_t)j < t->recode_routes.size() ? t->recode_routes[j] : -1;
    }
    out[c] = RECODE_LDS_CODES;
    return RGBM_OK;
}

}  // extern "C"
