// rgbm_cost.h -- the update-cost side of the probability modes (python/repair/model.py `_compute_repair_pmf`, `_compute_score`;
// reference model.py:1145-1277), included by rgbm_pmf.hip and by no other source (the kernels are file-local):
//
//   k_edit_distance       Levenshtein distance of every (a, b) pair of two string pools      (repair.costs.edit_distance)
//   k_edit_distance_long  the same for pairs whose strings are BOTH longer than 64 code points
//   k_weighted_pmf        the stable top-k candidates of every cell, after the cost re-weighting + renormalisation where asked for   (_compute_weighted_probs)
//
// Strings are int32 Unicode code points with int64 offsets (Python's str indexes code points, so the distances are the
// ones repair.costs computes).  Probabilities follow the Python expression order step by step; the library is built with
// -ffp-contract=off -fno-fast-math, so `1.0 + weight * c`, the reciprocal and the divisions round as CPython's do.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace rgbm_cost {

constexpr int ED_BLOCK = 256;        // pairs per block of k_edit_distance (one b string per blockIdx.y)
constexpr int ED_PAT = 64;           // longest bit-parallel pattern: one 64-bit word

// Levenshtein distance with the pattern P (m <= 64 code points) against the text T (any length): Myers' bit-vector algorithm
// in Hyyro's formulation for the global distance (the top row of the DP grows by one per text character, hence `Ph | 1`).
// `pat(k)` / `txt(j)` read code points, so the pattern may sit in LDS or global memory.  Eq masks are built per text character
// by comparing against the pattern (code points are unbounded: no alphabet table).
template <typename Pat, typename Txt>
__host__ __device__ inline int myers_distance(Pat pat, int m, Txt txt, long long n) {
    if (m == 0) return (int)n;
    if (n == 0) return m;
    const uint64_t top = 1ull << (m - 1);
    uint64_t pv = m == 64 ? ~0ull : ((1ull << m) - 1), mv = 0;
    int score = m;
    for (long long j = 0; j < n; ++j) {
        const int32_t ch = txt(j);
        uint64_t eq = 0;
        for (int k = 0; k < m; ++k) eq |= (uint64_t)(pat(k) == ch) << k;
        const uint64_t xv = eq | mv;
        const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
        uint64_t ph = mv | ~(xh | pv);
        uint64_t mh = pv & xh;
        if (ph & top) ++score;
        else if (mh & top) --score;
        ph = (ph << 1) | 1ull;
        mh <<= 1;
        pv = mh | ~(xv | ph);
        mv = ph & xv;
    }
    return score;
}

}  // namespace rgbm_cost

namespace {

// ---------------------------------------------------------------------------------------------
// dist[i][j] = Levenshtein(a_i, b_j).  grid (ceil(n_a / 256), b strings from j0 on): the block's b string is staged in LDS when it has at most
// 64 code points and is the pattern of every lane; otherwise a lane takes its own a string as the pattern (global reads, L1
// resident) when that one has at most 64, and leaves the pair to k_edit_distance_long when neither does.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rgbm_cost::ED_BLOCK) void k_edit_distance(const int32_t* __restrict__ a_cp, const int64_t* __restrict__ a_off,
                                                                      long long n_a, const int32_t* __restrict__ b_cp,
                                                                      const int64_t* __restrict__ b_off, long long n_b, long long j0,
                                                                      int32_t* __restrict__ dist) {
    __shared__ int32_t pat[rgbm_cost::ED_PAT];
    const long long j = j0 + blockIdx.y;
    const int64_t b0 = b_off[j];
    const long long nb = b_off[j + 1] - b0;
    const bool b_is_pattern = nb <= rgbm_cost::ED_PAT;
    if (b_is_pattern)
        for (int k = threadIdx.x; k < (int)nb; k += blockDim.x) pat[k] = b_cp[b0 + k];
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_a) return;
    const int64_t a0 = a_off[i];
    const long long na = a_off[i + 1] - a0;
    const int32_t* a = a_cp + a0;
    const int32_t* b = b_cp + b0;
    int d;
    if (b_is_pattern)
        d = rgbm_cost::myers_distance([&](int k) { return pat[k]; }, (int)nb, [&](long long q) { return a[q]; }, na);
    else if (na <= rgbm_cost::ED_PAT)
        d = rgbm_cost::myers_distance([&](int k) { return a[k]; }, (int)na, [&](long long q) { return b[q]; }, nb);
    else
        return;                                            // k_edit_distance_long
    dist[i * n_b + j] = d;
}

// Pairs whose strings both exceed 64 code points: one single-wave workgroup per pair, the DP over anti-diagonals (the cells of a
// diagonal are independent; lanes stride over it).  The three live diagonals sit in global scratch, 3 * (min(na, nb) + 2) ints
// per pair from `scr_off[p]`, touched by this workgroup only; a barrier separates consecutive diagonals.
__global__ __launch_bounds__(64) void k_edit_distance_long(const int32_t* __restrict__ a_cp, const int64_t* __restrict__ a_off,
                                                          const int32_t* __restrict__ b_cp, const int64_t* __restrict__ b_off, long long n_b,
                                                          const int64_t* __restrict__ pair_a, const int64_t* __restrict__ pair_b,
                                                          const int64_t* __restrict__ scr_off, int32_t* __restrict__ scr,
                                                          int32_t* __restrict__ dist) {
    const long long p = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const long long i = pair_a[p], j = pair_b[p];
    const int32_t* s = a_cp + a_off[i];
    const int32_t* t = b_cp + b_off[j];
    long long ns = a_off[i + 1] - a_off[i], nt = b_off[j + 1] - b_off[j];
    if (nt < ns) { const int32_t* x = s; s = t; t = x; const long long y = ns; ns = nt; nt = y; }     // s: the shorter one
    const long long w = ns + 2;
    int32_t* const base = scr + scr_off[p];
    // diagonal d holds D[r][d - r] for r in [max(0, d - nt), min(ns, d)], at index r of buffer d % 3
    for (long long d = 0; d <= ns + nt; ++d) {
        int32_t* cur = base + (d % 3) * w;
        const int32_t* prev = base + ((d + 2) % 3) * w;     // diagonal d - 1
        const int32_t* prev2 = base + ((d + 1) % 3) * w;    // diagonal d - 2
        const long long r0 = d - nt > 0 ? d - nt : 0, r1 = d < ns ? d : ns;
        for (long long r = r0 + lane; r <= r1; r += 64) {
            const long long c = d - r;
            int32_t v;
            if (r == 0) v = (int32_t)c;
            else if (c == 0) v = (int32_t)r;
            else {
                const int32_t up = prev[r - 1] + 1, left = prev[r] + 1, sub = prev2[r - 1] + (s[r - 1] == t[c - 1] ? 0 : 1);
                v = up < left ? up : left;
                v = sub < v ? sub : v;
            }
            cur[r] = v;
        }
        __syncthreads();
    }
    if (lane == 0) dist[i * n_b + j] = base[((ns + nt) % 3) * w + ns];
}

// ---------------------------------------------------------------------------------------------
// the top-k candidate distributions, with or without the update costs (model.py `_compute_repair_pmf`, reference `_compute_weighted_probs` model.py:1145-1165).
// One wave per cell; lane l owns the classes c = l (mod 64) and overwrites proba[cell][c] with the final probability, so no
// lane reads what another wrote.  Per cell, in the order (and the roundings) of the Python loop:
//   p_c *= 1.0 / (1.0 + weight * cost[row][c])    for cost_row[cell] = row >= 0 and cost[row][c] not NaN (NaN = None)
//   renormalise: norm = p_0 + p_1 + ... (sequential, class order, like Python's sum); p_c /= norm when norm > 0
//   cur_prob = p[cur_code] (0.0 when the current value is not a class), stable top-k (desc, ties in class order, p > threshold)
//   top1_cost = cost[base][top-1 class], base = cost_row[cell] when >= 0 else the self row (n_rows); NaN without a top-1
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_weighted_pmf(double* __restrict__ proba, long long m, int K, int top_k, double threshold,
                                                      const int32_t* __restrict__ cur_code, const int32_t* __restrict__ cost_row,
                                                      const double* __restrict__ cost, long long n_cost_rows, double weight, int renormalise,
                                                      int32_t* __restrict__ cls_out, double* __restrict__ prob_out,
                                                      double* __restrict__ cur_prob_out, double* __restrict__ top1_cost_out) {
    const long long cell = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (cell >= m) return;
    const int lane = (int)(threadIdx.x & 63u);
    double* p = proba + cell * K;
    const int row = (cost && cost_row) ? cost_row[cell] : -1;
    const double* crow = row >= 0 ? cost + (long long)row * K : nullptr;
    double norm = 0.0;
    const int Kw = (crow || renormalise) ? K : 0;          // (uniform over the wave) with neither, the probabilities stay as they are: no pass over them
    for (int base = 0; base < Kw; base += 64) {
        const int c = base + lane;
        double v = 0.0;
        if (c < K) {
            v = p[c];
            if (crow) {
                const double cc = crow[c];
                if (!isnan(cc)) {
                    const double den = 1.0 + weight * cc;
                    v = v * (1.0 / den);
                }
                p[c] = v;                                    // (only where a cost row exists: nothing else changes a value here)
            }
        }
        if (renormalise) {                                   // every lane adds the chunk's values in class order: the same sum everywhere
            const int cnt = K - base < 64 ? K - base : 64;
            for (int l = 0; l < cnt; ++l) norm = norm + __shfl(v, l);
        }
    }
    if (renormalise && norm > 0.0)
        for (int c = lane; c < K; c += 64) p[c] = p[c] / norm;
    if (cur_prob_out) {
        const int cc = cur_code ? cur_code[cell] : -1;
        if (cc >= 0 && cc < K) { if ((cc & 63) == lane) cur_prob_out[cell] = p[cc]; }
        else if (lane == 0) cur_prob_out[cell] = 0.0;
    }
    double last_p = INFINITY; int last_c = -1;
    int top1 = -1;
    for (int j = 0; j < top_k; ++j) {
        double bp = -1.0; int bc = 0x7FFFFFFF;
        for (int c = lane; c < K; c += 64) {
            const double v = p[c];
            const bool after = v < last_p || (v == last_p && c > last_c);
            if (after && v > threshold && (v > bp || (v == bp && c < bc))) { bp = v; bc = c; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double op = __shfl_xor(bp, d); const int oc = __shfl_xor(bc, d);
            if (op > bp || (op == bp && oc < bc)) { bp = op; bc = oc; }
        }
        const bool found = bc != 0x7FFFFFFF;
        if (lane == 0) { cls_out[cell * top_k + j] = found ? bc : -1; prob_out[cell * top_k + j] = found ? bp : 0.0; }
        if (!found) {
            for (int r = j + 1 + lane; r < top_k; r += 64) { cls_out[cell * top_k + r] = -1; prob_out[cell * top_k + r] = 0.0; }
            break;
        }
        if (j == 0) top1 = bc;
        last_p = bp; last_c = bc;
    }
    if (top1_cost_out && lane == 0) {
        double tc = NAN;
        if (cost && top1 >= 0) tc = cost[(row >= 0 ? (long long)row : n_cost_rows) * K + top1];
        top1_cost_out[cell] = tc;
    }
}

}  // namespace
