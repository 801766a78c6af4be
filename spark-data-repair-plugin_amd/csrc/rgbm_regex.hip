// rgbm_regex.hip -- a value-space step that needs no table (like rgbm_nearest_values): rgbm_regex_structure.
// =============================================================================================
// Regex-structure repair (RegexStructureRepair.scala; the statement is repair/regex_structure.py) over a pool of strings.
// The program is at most 32 segments, each a run of min..max code points of one membership set (a capture: a 128-bit ASCII class; a
// constant: every code point but the five line terminators, 1..len of them).  With positions 0..len of a string as bits,
//   F[S] = {len} with `$`, every position without;   F[i] = { p : some k in [min, max] has p..p+k-1 members of segment i and p+k in F[i+1] }
// is built backwards by run propagation  R_0 = F[i+1], R_k = (R_{k-1} >> 1) & M,  F[i] = OR of R_k over k in [min, max]  (M = the membership
// mask of the string's code points), the match starts at the least position of F[0] (which must be 0 with `^`), and forwards every segment
// takes the LARGEST k in [min, min(max, run of M from p)] with p+k in F[i+1]: leftmost start, every quantifier greedy, first successful
// backtracking path, without backtracking.  Everything is integers: the result is the statement's code point for code point.
// Two routes, chosen per string (the host counts them into info_out):
//   k_rx_word  len <= 63: positions 0..len are one 64-bit word, one LANE per string.  M and F of every segment are one word each, kept in
//              LDS ([segment][lane]: 2 x 32 x 64 x 8 B = 32 KiB a workgroup of one wave); the greedy pick is a count of trailing ones (the run)
//              and the highest set bit of F[i+1] inside the window.
//   k_rx_wave  64 <= len <= RGBM_RX_WAVE_MAX_CP: one WAVE per string, lane l owns positions 64l..64l+63.  M comes from ballots over coalesced
//              loads, the shift's carry across lanes is one __shfl_down of the neighbour's bit 0, F lives in LDS (32 x 64 words); the forward
//              pass is uniform over the wave (every lane reads the same LDS words).  The strings of this route are listed by the host.
//   longer strings get state 2 and no output.
// Output: the kernels run twice -- a length pass (state and length per string), k_scan_counts over the lengths, a write pass into the
// offsets.  The program (1.2 KB) is a kernel argument staged into LDS.  No atomics; plain vector stores only.
// =============================================================================================
#include "rgbm_prep.h"

#include <cstring>

namespace {

using namespace rgh;

constexpr int RX_MAX_SEGS = 32, RX_WORD_MAX = 63, RX_MAX_BOUND = 65535;
constexpr int RX_B = 64;                       // one wave per workgroup in both kernels
constexpr int RX_WAVE_GRID = 2048;             // workgroups of the wave route (each loops over the listed strings)

struct RxProg { int32_t n_segs, anchors; rgbm_rx_seg seg[RX_MAX_SEGS]; };

__device__ __forceinline__ bool rx_member(const rgbm_rx_seg& sg, int32_t c) {
    if (sg.kind == 1) return !(c == 0x0A || c == 0x0D || c == 0x85 || c == 0x2028 || c == 0x2029);
    return c >= 0 && c < 128 && ((sg.cls[c >> 5] >> (c & 31)) & 1u);
}

__device__ __forceinline__ void rx_stage(RxProg& dst, const RxProg& src) {
    const int32_t* s = reinterpret_cast<const int32_t*>(&src);
    int32_t* d = reinterpret_cast<int32_t*>(&dst);
    for (int i = threadIdx.x; i < (int)(sizeof(RxProg) / 4); i += RX_B) d[i] = s[i];
    __syncthreads();
}

// ---- one word: a lane per string -----------------------------------------------------------------------------------------------------
template <bool WRITE>
__global__ __launch_bounds__(RX_B) void k_rx_word(const RxProg prog_arg, const int32_t* __restrict__ const_cp, const int32_t* __restrict__ cp,
                                                  const long long* __restrict__ off, long long n, uint8_t* __restrict__ state,
                                                  unsigned* __restrict__ out_len, const long long* __restrict__ out_off, int32_t* __restrict__ out_cp) {
    __shared__ RxProg prog;
    __shared__ unsigned long long Ml[RX_MAX_SEGS][RX_B], Fl[RX_MAX_SEGS][RX_B];
    rx_stage(prog, prog_arg);
    const long long i = (long long)blockIdx.x * RX_B + threadIdx.x;
    if (i >= n) return;
    const int t = threadIdx.x;
    const long long base = off[i];
    const long long len_ll = off[i + 1] - base;
    if (len_ll > RX_WORD_MAX) {                 // the wave route writes its own strings; beyond it: state 2
        if (!WRITE && len_ll > RGBM_RX_WAVE_MAX_CP) { state[i] = 2; out_len[i] = 0; }
        return;
    }
    if (WRITE && state[i] != 1) return;
    const int len = (int)len_ll, S = prog.n_segs;
    const int32_t* s = cp + base;
    for (int q = 0; q < S; ++q) {
        unsigned long long m = 0;
        for (int p = 0; p < len; ++p) m |= (unsigned long long)rx_member(prog.seg[q], s[p]) << p;
        Ml[q][t] = m;
    }
    const unsigned long long fend = (prog.anchors & 2) ? (1ull << len) : ((2ull << len) - 1ull);
    unsigned long long G = fend;
    for (int q = S - 1; q >= 0; --q) {
        const int mn = prog.seg[q].min, mx = prog.seg[q].max;
        const int kmax = (mx < 0 || mx > len) ? len : mx;
        const unsigned long long M = Ml[q][t];
        unsigned long long R = G, acc = mn == 0 ? G : 0ull;
        for (int k = 1; k <= kmax; ++k) {
            R = (R >> 1) & M;
            if (!R) break;
            if (k >= mn) acc |= R;
        }
        Fl[q][t] = acc;
        G = acc;
    }
    const bool hit = G != 0 && (!(prog.anchors & 1) || (G & 1ull));
    if (!WRITE) state[i] = hit ? 1 : 0;
    if (!hit) { if (!WRITE) out_len[i] = 0; return; }
    int p = __ffsll((long long)G) - 1;
    unsigned total = 0;
    int32_t* o = WRITE ? out_cp + out_off[i] : nullptr;
    for (int q = 0; q < S; ++q) {
        const rgbm_rx_seg& sg = prog.seg[q];
        const unsigned long long nxt = q + 1 < S ? Fl[q + 1][t] : fend;
        const unsigned long long inv = ~(Ml[q][t] >> p);                  // bit 63 of M is never set: inv != 0
        const int run = __ffsll((long long)inv) - 1;
        const int hi = (sg.max < 0 || sg.max > run) ? run : sg.max;
        const int width = hi - sg.min + 1;                                // >= 1: p is in F[q]
        unsigned long long w = nxt >> (p + sg.min);
        if (width < 64) w &= (1ull << width) - 1ull;
        const int k = sg.min + 63 - __clzll((long long)w);                // w != 0 for the same reason
        if (sg.kind == 1) {
            if (WRITE) for (int j = 0; j < sg.const_len; ++j) o[total + j] = const_cp[sg.const_off + j];
            total += (unsigned)sg.const_len;
        } else {
            if (WRITE) for (int j = 0; j < k; ++j) o[total + j] = s[p + j];
            total += (unsigned)k;
        }
        p += k;
    }
    if (!WRITE) out_len[i] = total;
}

// ---- a wave per string ---------------------------------------------------------------------------------------------------------------
// the membership word of this lane (positions 64 lane .. 64 lane + 63) for one segment: one ballot per 64 code points, coalesced loads
__device__ __forceinline__ unsigned long long rx_wave_mask(const rgbm_rx_seg& sg, const int32_t* __restrict__ s, int len, int lane) {
    unsigned long long mine = 0;
    const int nw = (len + 63) >> 6;
    for (int j = 0; j < nw; ++j) {
        const int idx = (j << 6) + lane;
        const bool in = idx < len && rx_member(sg, s[idx]);
        const unsigned long long b = __ballot(in);
        if (lane == j) mine = b;
    }
    return mine;
}

// the word of F[S] that lane `lane` owns
__device__ __forceinline__ unsigned long long rx_wave_end(int anchors, int len, int lane) {
    const int b = lane << 6;
    if (anchors & 2) return (len >= b && len < b + 64) ? 1ull << (len - b) : 0ull;
    if (len >= b + 63) return ~0ull;
    return len < b ? 0ull : (2ull << (len - b)) - 1ull;
}

template <bool WRITE>
__global__ __launch_bounds__(RX_B) void k_rx_wave(const RxProg prog_arg, const int32_t* __restrict__ const_cp, const int32_t* __restrict__ cp,
                                                  const long long* __restrict__ off, const long long* __restrict__ list, long long n_list,
                                                  uint8_t* __restrict__ state, unsigned* __restrict__ out_len,
                                                  const long long* __restrict__ out_off, int32_t* __restrict__ out_cp) {
    __shared__ RxProg prog;
    __shared__ unsigned long long Fl[RX_MAX_SEGS + 1][RX_B], Ml[RX_B];
    rx_stage(prog, prog_arg);
    const int lane = threadIdx.x, S = prog.n_segs;
    for (long long e = blockIdx.x; e < n_list; e += gridDim.x) {           // uniform over the workgroup (= the wave)
        const long long i = list[e];
        if (WRITE && state[i] != 1) continue;
        const long long base = off[i];
        const int len = (int)(off[i + 1] - base);                          // 64 .. RGBM_RX_WAVE_MAX_CP (the host listed it)
        const int32_t* s = cp + base;
        __syncthreads();                                                   // the previous string's reads of Fl / Ml are done
        unsigned long long G = rx_wave_end(prog.anchors, len, lane);
        Fl[S][lane] = G;
        for (int q = S - 1; q >= 0; --q) {
            const int mn = prog.seg[q].min, mx = prog.seg[q].max;
            const int kmax = (mx < 0 || mx > len) ? len : mx;
            const unsigned long long M = rx_wave_mask(prog.seg[q], s, len, lane);
            unsigned long long R = G, acc = mn == 0 ? G : 0ull;
            for (int k = 1; k <= kmax; ++k) {
                unsigned carry = (unsigned)__shfl_down((int)(R & 1ull), 1);     // bit 0 of the next lane's word
                if (lane == 63) carry = 0;
                R = ((R >> 1) | ((unsigned long long)carry << 63)) & M;
                if (!__any(R != 0)) break;
                if (k >= mn) acc |= R;
            }
            Fl[q][lane] = acc;
            G = acc;
        }
        __syncthreads();
        const unsigned long long have = __ballot(G != 0);
        bool hit = have != 0;
        int p = 0;
        if (hit) {
            const int w0 = __ffsll((long long)have) - 1;
            p = (w0 << 6) + __ffsll((long long)Fl[0][w0]) - 1;
            hit = !(prog.anchors & 1) || p == 0;
        }
        if (!WRITE && lane == 0) { state[i] = hit ? 1 : 0; if (!hit) out_len[i] = 0; }
        if (!hit) continue;
        unsigned total = 0;
        int32_t* o = WRITE ? out_cp + out_off[i] : nullptr;
        for (int q = 0; q < S; ++q) {
            const rgbm_rx_seg& sg = prog.seg[q];
            __syncthreads();                                               // the previous segment's reads of Ml are done
            Ml[lane] = rx_wave_mask(sg, s, len, lane);
            __syncthreads();
            // the run of members from p, as far as max needs it
            const int want = sg.max < 0 ? len : sg.max;
            int run = 0, w = p >> 6;
            {
                const int bit = p & 63;
                const unsigned long long inv = ~(Ml[w] >> bit);            // the zeros shifted in end the count inside this word ...
                const int tz = inv ? __ffsll((long long)inv) - 1 : 64;
                if (tz < 64 - bit) run = tz;
                else {                                                     // ... unless the run reaches the word's last position
                    run = 64 - bit;
                    for (++w; w < RX_B && run < want; ++w) {
                        const unsigned long long iv = ~Ml[w];
                        if (iv) { run += __ffsll((long long)iv) - 1; break; }
                        run += 64;
                    }
                }
            }
            const int hi = run < want ? run : want;
            const int lo_q = p + sg.min, hi_q = p + hi;                    // lo_q <= hi_q <= len: p is in F[q]
            int qq = -1;
            for (int ww = hi_q >> 6; ww >= (lo_q >> 6); --ww) {
                unsigned long long x = Fl[q + 1][ww];
                if (ww == (hi_q >> 6) && (hi_q & 63) != 63) x &= (2ull << (hi_q & 63)) - 1ull;
                if (ww == (lo_q >> 6)) x &= ~0ull << (lo_q & 63);
                if (x) { qq = (ww << 6) + 63 - __clzll((long long)x); break; }
            }
            if (qq < 0) { total = 0; break; }                              // (not reachable: p is in F[q])
            const int k = qq - p;
            if (sg.kind == 1) {
                if (WRITE) for (int j = lane; j < sg.const_len; j += 64) o[total + j] = const_cp[sg.const_off + j];
                total += (unsigned)sg.const_len;
            } else {
                if (WRITE) for (int j = lane; j < k; j += 64) o[total + j] = s[p + j];
                total += (unsigned)k;
            }
            p = qq;
        }
        if (!WRITE && lane == 0) out_len[i] = total;
    }
}

}  // namespace

extern "C" {

RGBM_EXPORT int rgbm_regex_structure(int32_t device_id, const rgbm_rx_seg* segs, int32_t n_segs, int32_t anchors, const int32_t* const_cp,
                                     int32_t n_const_cp, const int32_t* cp, const int64_t* off, int64_t n, uint8_t* state_out, int64_t* out_off,
                                     int32_t* out_cp, int64_t* info_out) {
    if (!segs || !out_off || !info_out || n_segs < 1 || n_segs > RX_MAX_SEGS || anchors < 0 || anchors > 3 || n_const_cp < 0 || n < 0 ||
        (n_const_cp > 0 && !const_cp) || (n > 0 && (!off || !state_out || !out_cp)))
        return fail(RGBM_ERR_ARG, "rgbm_regex_structure: bad argument (1 .. 32 segments, anchors 0 .. 3, arrays that are needed)");
    long long const_sum = 0;
    for (int q = 0; q < n_segs; ++q) {
        const rgbm_rx_seg& sg = segs[q];
        if (sg.kind == 0) {
            if (sg.min < 0 || sg.min > RX_MAX_BOUND || sg.max < -1 || sg.max > RX_MAX_BOUND || (sg.max >= 0 && sg.max < sg.min))
                return fail(RGBM_ERR_ARG, "rgbm_regex_structure: a capture with bounds outside 0 <= min <= max <= 65535 (max -1: unbounded)");
        } else if (sg.kind == 1) {
            if (sg.const_len < 1 || sg.const_off < 0 || (long long)sg.const_off + sg.const_len > n_const_cp || sg.min != 1 || sg.max != sg.const_len)
                return fail(RGBM_ERR_ARG, "rgbm_regex_structure: a constant outside const_cp, or whose bounds are not 1 .. its length");
            const_sum += sg.const_len;
        } else
            return fail(RGBM_ERR_ARG, "rgbm_regex_structure: a segment kind other than 0 (capture) and 1 (constant)");
    }
    if (const_sum > n_const_cp) return fail(RGBM_ERR_ARG, "rgbm_regex_structure: the constants overlap in const_cp");
    // routes, from the offsets alone
    std::vector<long long> wave_list;
    long long n_word = 0, n_long = 0;
    if (n > 0) {
        if (off[0] != 0) return fail(RGBM_ERR_ARG, "rgbm_regex_structure: off[0] is not 0");
        for (int64_t i = 0; i < n; ++i) {
            const long long len = off[i + 1] - off[i];
            if (len < 0) return fail(RGBM_ERR_ARG, "rgbm_regex_structure: the offsets decrease");
            if (len <= RX_WORD_MAX) ++n_word;
            else if (len <= RGBM_RX_WAVE_MAX_CP) wave_list.push_back((long long)i);
            else ++n_long;
        }
        if (off[n] > 0 && !cp) return fail(RGBM_ERR_ARG, "rgbm_regex_structure: cp is NULL");
    }
    out_off[0] = 0;
    info_out[0] = n_word; info_out[1] = (int64_t)wave_list.size(); info_out[2] = n_long; info_out[3] = 0;
    if (n == 0) return RGBM_OK;
    return guarded([&]() {
        use_device(device_id);
        StreamGuard sg;
        RxProg prog;
        memset(&prog, 0, sizeof(prog));
        prog.n_segs = n_segs; prog.anchors = anchors;
        for (int q = 0; q < n_segs; ++q) prog.seg[q] = segs[q];
        const size_t N = (size_t)n, n_cp = (size_t)off[n], n_wave = wave_list.size();
        DevBuf<int32_t> d_cp(n_cp), d_const((size_t)n_const_cp);
        DevBuf<long long> d_off(N + 1), d_list(n_wave), d_out_off(N + 1);
        DevBuf<uint8_t> d_state(N);
        DevBuf<unsigned> d_len(N);
        d_cp.upload(cp, n_cp, sg.s);
        d_const.upload(const_cp, (size_t)n_const_cp, sg.s);
        d_off.upload(reinterpret_cast<const long long*>(off), N + 1, sg.s);
        d_list.upload(wave_list.data(), n_wave, sg.s);
        const unsigned grid_word = nblocks(n, RX_B), grid_wave = (unsigned)std::min<size_t>(n_wave, RX_WAVE_GRID);
        hipLaunchKernelGGL(k_rx_word<false>, dim3(grid_word), dim3(RX_B), 0, sg.s, prog, d_const.p, d_cp.p, d_off.p, (long long)n, d_state.p, d_len.p,
                           (const long long*)nullptr, (int32_t*)nullptr);
        if (n_wave)
            hipLaunchKernelGGL(k_rx_wave<false>, dim3(grid_wave), dim3(RX_B), 0, sg.s, prog, d_const.p, d_cp.p, d_off.p, d_list.p, (long long)n_wave,
                               d_state.p, d_len.p, (const long long*)nullptr, (int32_t*)nullptr);
        launch_scan_counts(d_len.p, (long long)n, d_out_off.p, d_out_off.p + N, sg.s);
        HIPCHK(hipGetLastError());
        d_state.download(state_out, N, sg.s);
        d_out_off.download(reinterpret_cast<long long*>(out_off), N + 1, sg.s);
        HIPCHK(hipStreamSynchronize(sg.s));
        const size_t total = (size_t)out_off[n];
        long long repaired = 0;
        for (size_t i = 0; i < N; ++i) repaired += state_out[i] == 1;
        info_out[3] = repaired;
        if (total == 0) return RGBM_OK;
        DevBuf<int32_t> d_out(total);
        hipLaunchKernelGGL(k_rx_word<true>, dim3(grid_word), dim3(RX_B), 0, sg.s, prog, d_const.p, d_cp.p, d_off.p, (long long)n, d_state.p, d_len.p,
                           d_out_off.p, d_out.p);
        if (n_wave)
            hipLaunchKernelGGL(k_rx_wave<true>, dim3(grid_wave), dim3(RX_B), 0, sg.s, prog, d_const.p, d_cp.p, d_off.p, d_list.p, (long long)n_wave,
                               d_state.p, d_len.p, d_out_off.p, d_out.p);
        HIPCHK(hipGetLastError());
        d_out.download(out_cp, total, sg.s);
        HIPCHK(hipStreamSynchronize(sg.s));
        return RGBM_OK;
    });
}

}  // extern "C"
