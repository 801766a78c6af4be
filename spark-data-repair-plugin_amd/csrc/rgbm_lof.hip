// rgbm_lof.hip -- a relational step next to the HBM-resident code table (what the steps share is rgbm_prep.h):
// =============================================================================================
// LOF in code space (LOFOutlierErrorDetector = scikit-learn's LocalOutlierFactor(novelty=False) on one continuous attribute; the statement
// is repair/lof_codes.py).  The input is the column's sorted dictionary with the rows per entry: in one dimension the k
// nearest neighbours of a value are the other copies of itself and a contiguous window of at most k neighbouring positions, so the factor is
// a function of the POSITION.  One lane per position, tiles of LOF_TILE positions, the tile and a halo of LOF_HALO positions on either
// side staged in LDS (a window never spans more than k <= 64 positions on a side).  Three launches, because each pass reads what the one
// before wrote for the neighbouring positions, other tiles' included:
//   k_lof_window   the outward merge (at most k steps): kdist and the window record
//                  bits 0-7 left extent, 8-15 right extent, 16-23 copies taken of the last neighbour, 24-25 its side (1 left, 2 right, 0: the
//                  copies of the value itself suffice), 26 the tie flag (both candidates at one distance and only one fits: taken left)
//   k_lof_lrd      local reachability density  1 / (sum_j taken_j * max(kdist[j], |v_c - v_j|) / k_ + 1e-10)
//   k_lof_score    lof = (sum_j taken_j * (lrd[j] / lrd[c])) / k_; the flag word of a wave is one ballot, stored by one lane; ties and
//                  scores within threshold * 2^-40 of the threshold are counted (one atomic per wave)
// Both sums run over the window's positions in ascending order, one multiplication and one addition per position (the library is built with
// -ffp-contract=off): the scores are the numpy statement's bit for bit.  Counts are staged clamped to k_ + 1: no comparison of the merge can
// tell a larger count from that.  LDS of a tile: 384 x (8 + 4) B = 4.5 KiB in the first pass, 384 x (8 + 8 + 4) B = 7.5 KiB in the second,
// 384 x (8 + 4) B in the third.  Algorithmic bytes per position: 16 in, 12 / 8 / 16 out of the three passes.
// =============================================================================================
#include "rgbm_prep.h"

#include <cmath>

namespace {

using namespace rgh;

constexpr int LOF_TILE = 256, LOF_HALO = 64, LOF_SPAN = LOF_TILE + 2 * LOF_HALO, LOF_MAX_K = 64;

// dst[i] = f(src[first + i]) for the positions of [first, first + LOF_SPAN) that exist; the others are never read
template <typename T, typename S, typename F>
__device__ __forceinline__ void lof_stage(T (&dst)[LOF_SPAN], const S* __restrict__ src, long long first, int d, F f) {
    for (int i = threadIdx.x; i < LOF_SPAN; i += LOF_TILE) {
        const long long g = first + i;
        if (g >= 0 && g < d) dst[i] = f(src[g]);
    }
}

__device__ __forceinline__ int lof_taken(int j, int li, int last, int self_taken, int part, const int* lm) {
    return j == li ? self_taken : (j == last ? part : lm[j]);
}

__global__ __launch_bounds__(LOF_TILE) void k_lof_window(const double* __restrict__ values, const long long* __restrict__ counts, int d, int k_,
                                                         double* __restrict__ kdist, unsigned* __restrict__ win) {
    __shared__ double lv[LOF_SPAN];
    __shared__ int lm[LOF_SPAN];
    const long long first = (long long)blockIdx.x * LOF_TILE - LOF_HALO;
    lof_stage(lv, values, first, d, [](double x) { return x; });
    lof_stage(lm, counts, first, d, [k_](long long m) { return (int)(m < (long long)k_ + 1 ? m : (long long)k_ + 1); });
    __syncthreads();
    const int li = (int)threadIdx.x + LOF_HALO;
    const long long p = first + li;
    if (p >= d) return;
    const long long lo = 0 - first, hi = (long long)d - 1 - first;                   // the LDS slots of positions 0 and d - 1 (may lie outside the span)
    const double vc = lv[li];
    const int self_taken = min(lm[li] - 1, k_);
    int need = k_ - self_taken, l = li, r = li, side = 0, part = 0, tie = 0;
    double kd = 0.0;
    for (int step = 0; step < k_ && need > 0; ++step) {
        const bool has_l = l > lo, has_r = r < hi;
        if (!has_l && !has_r) break;                                                  // (not reachable: the other values hold k_ copies at least)
        const double dl = has_l ? fabs(vc - lv[l - 1]) : 0.0, dr = has_r ? fabs(vc - lv[r + 1]) : 0.0;
        const bool go_l = has_l && (!has_r || dl <= dr);
        if (has_l && has_r && dl == dr && need < lm[l - 1] + lm[r + 1]) tie = 1;
        const int j = go_l ? l - 1 : r + 1;
        const int take = min(need, lm[j]);
        need -= take;
        kd = go_l ? dl : dr;
        side = go_l ? 1 : 2;
        part = take;
        if (go_l) l = j; else r = j;
    }
    kdist[p] = kd;
    win[p] = (unsigned)(li - l) | ((unsigned)(r - li) << 8) | ((unsigned)part << 16) | ((unsigned)side << 24) | ((unsigned)tie << 26);
}

__global__ __launch_bounds__(LOF_TILE) void k_lof_lrd(const double* __restrict__ values, const long long* __restrict__ counts,
                                                      const double* __restrict__ kdist, const unsigned* __restrict__ win, int d, int k_,
                                                      double* __restrict__ lrd) {
    __shared__ double lv[LOF_SPAN];
    __shared__ double lk[LOF_SPAN];
    __shared__ int lm[LOF_SPAN];
    const long long first = (long long)blockIdx.x * LOF_TILE - LOF_HALO;
    lof_stage(lv, values, first, d, [](double x) { return x; });
    lof_stage(lk, kdist, first, d, [](double x) { return x; });
    lof_stage(lm, counts, first, d, [k_](long long m) { return (int)(m < (long long)k_ + 1 ? m : (long long)k_ + 1); });
    __syncthreads();
    const int li = (int)threadIdx.x + LOF_HALO;
    const long long p = first + li;
    if (p >= d) return;
    const unsigned w = win[p];
    const int l = li - (int)(w & 255u), r = li + (int)((w >> 8) & 255u), part = (int)((w >> 16) & 255u), side = (int)((w >> 24) & 3u);
    const int last = side == 1 ? l : (side == 2 ? r : -1);
    const int self_taken = min(lm[li] - 1, k_);
    const double vc = lv[li];
    double s = 0.0;
    for (int j = l; j <= r; ++j) {
        const double reach = fmax(lk[j], fabs(vc - lv[j]));
        s = s + (double)lof_taken(j, li, last, self_taken, part, lm) * reach;
    }
    lrd[p] = 1.0 / (s / (double)k_ + 1e-10);
}

__global__ __launch_bounds__(LOF_TILE) void k_lof_score(const long long* __restrict__ counts, const double* __restrict__ lrd,
                                                        const unsigned* __restrict__ win, int d, int k_, double threshold,
                                                        double* __restrict__ score, unsigned long long* __restrict__ flag_bits,
                                                        unsigned long long* __restrict__ info) {
    __shared__ double lr[LOF_SPAN];
    __shared__ int lm[LOF_SPAN];
    const long long first = (long long)blockIdx.x * LOF_TILE - LOF_HALO;
    lof_stage(lr, lrd, first, d, [](double x) { return x; });
    lof_stage(lm, counts, first, d, [k_](long long m) { return (int)(m < (long long)k_ + 1 ? m : (long long)k_ + 1); });
    __syncthreads();
    const int li = (int)threadIdx.x + LOF_HALO;
    const long long p = first + li;
    const bool live = p < d;                       // every lane stays for the ballots
    bool flag = false, tie = false, near = false;
    if (live) {
        const unsigned w = win[p];
        const int l = li - (int)(w & 255u), r = li + (int)((w >> 8) & 255u), part = (int)((w >> 16) & 255u), side = (int)((w >> 24) & 3u);
        const int last = side == 1 ? l : (side == 2 ? r : -1);
        const int self_taken = min(lm[li] - 1, k_);
        const double mine = lr[li];
        double s = 0.0;
        for (int j = l; j <= r; ++j) s = s + (double)lof_taken(j, li, last, self_taken, part, lm) * (lr[j] / mine);
        const double lof = s / (double)k_;
        if (score) score[p] = lof;
        flag = -lof < -threshold;
        near = fabs(lof - threshold) <= threshold * 0x1p-40;
        tie = ((w >> 26) & 1u) != 0;
    }
    const unsigned long long fb = __ballot(flag), tb = __ballot(tie), nb = __ballot(near);
    if (lane_id() == 0 && live) {                  // lane 0 holds the wave's lowest position: live = the word exists
        flag_bits[p >> 6] = fb;
        if (tb) atomicAdd(&info[0], (unsigned long long)__popcll(tb));
        if (nb) atomicAdd(&info[1], (unsigned long long)__popcll(nb));
    }
}

}  // namespace

extern "C" {

RGBM_EXPORT int rgbm_lof_1d(int32_t device_id, const double* values, const int64_t* counts, int32_t d, int32_t k, double threshold,
                            double* score_out, uint64_t* flag_bits_out, int64_t* info_out) {
    if (!values || !counts || !flag_bits_out || !info_out || d < 1 || k < 1 || k > LOF_MAX_K || !(threshold > 0.0) || threshold > 1e300)
        return fail(RGBM_ERR_ARG, "rgbm_lof_1d: bad argument (d >= 1, k in 1 .. 64, a positive threshold)");
    long long n = 0;                               // the sum of the counts, as far as k_ needs it
    for (int32_t i = 0; i < d; ++i) {
        if (counts[i] < 1) return fail(RGBM_ERR_ARG, "rgbm_lof_1d: a count below 1");
        if (!std::isfinite(values[i])) return fail(RGBM_ERR_ARG, "rgbm_lof_1d: a value that is not finite");
        if (i > 0 && !(values[i] > values[i - 1])) return fail(RGBM_ERR_ARG, "rgbm_lof_1d: the values are not ascending");
        n = std::min<long long>(n + std::min<long long>(counts[i], 2 * LOF_MAX_K), 1ll << 40);
    }
    if (!std::isfinite(values[d - 1] - values[0])) return fail(RGBM_ERR_ARG, "rgbm_lof_1d: the range of the values is not finite");
    if (n < 2) return fail(RGBM_ERR_ARG, "rgbm_lof_1d: fewer than two values in all");
    return guarded([&]() {
        use_device(device_id);
        StreamGuard sg;
        const int k_ = (int)std::max<long long>(1, std::min<long long>(k, n - 1));
        const size_t D = (size_t)d, nw = (D + 63) / 64;
        DevBuf<double> d_v(D), d_kd(D), d_lrd(D), d_score(score_out ? D : 0);
        DevBuf<long long> d_m(D);
        DevBuf<unsigned> d_win(D);
        DevBuf<unsigned long long> d_bits(nw), d_info(2);
        d_v.upload(values, D, sg.s);
        d_m.upload(reinterpret_cast<const long long*>(counts), D, sg.s);
        d_info.zero(sg.s);
        const unsigned grid = nblocks(d, LOF_TILE);
        hipLaunchKernelGGL(k_lof_window, dim3(grid), dim3(LOF_TILE), 0, sg.s, d_v.p, d_m.p, (int)d, k_, d_kd.p, d_win.p);
        hipLaunchKernelGGL(k_lof_lrd, dim3(grid), dim3(LOF_TILE), 0, sg.s, d_v.p, d_m.p, d_kd.p, d_win.p, (int)d, k_, d_lrd.p);
        hipLaunchKernelGGL(k_lof_score, dim3(grid), dim3(LOF_TILE), 0, sg.s, d_m.p, d_lrd.p, d_win.p, (int)d, k_, threshold, d_score.p, d_bits.p,
                           d_info.p);
        HIPCHK(hipGetLastError());
        unsigned long long info[2] = {0, 0};
        if (score_out) d_score.download(score_out, D, sg.s);
        d_bits.download(reinterpret_cast<unsigned long long*>(flag_bits_out), nw, sg.s);
        d_info.download(info, 2, sg.s);
        HIPCHK(hipStreamSynchronize(sg.s));
        info_out[0] = (int64_t)info[0];
        info_out[1] = (int64_t)info[1];
        return RGBM_OK;
    });
}

}  // extern "C"
