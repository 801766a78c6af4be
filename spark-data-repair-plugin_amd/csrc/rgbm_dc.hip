// rgbm_dc.hip -- a relational step on the HBM-resident code table (what the steps share is rgbm_prep.h):
//   detect_dc / row_bits  ConstraintErrorDetector for every parsed constraint but  X1..Xm -> Y  (that one is rgbm_table_detect_constraint,
//                         rgbm_prep.hip): all-pairs predicates inside the EQ groups; constants as one bit per (column, code)
//                         (ErrorDetectorApi.scala:189-244; repair/dc_codes.py builds the programs)
// ---------------------------------------------------------------------------------------------
// general denial constraints (rgbm_table_detect_dc, rgbm_table_detect_row_bits; the host lowering is repair/dc_codes.py).
//
// Two tuples: row i violates iff SOME row j (j == i included, the reference's EXISTS sub-query) makes every predicate true.  The EQ
// predicates group the rows (NULL-safe mixed-radix key, as rgbm_table_detect_constraint); the other predicates are evaluated over the
// pairs of each group.  The answer is an existence mask, so no step depends on an order:
//   k_dc_slots    open-addressing slot of every row's key (ht_claim); count[slot] takes the group's rows and hands every row its arrival rank (wave_add)
//   k_dc_stats    sum of |g|^2 and max |g| over the slots -- the exact pair count, known BEFORE any pair is evaluated
//   k_scan_counts exclusive scan of the slot counts = first position of every group
//   k_dc_scatter  the rows laid out by group: position -> row, its group's [begin, end), and per predicate the left and the right
//                 operand of the row (rank-mapped, NULL / "no number" = -1) with the predicate folded into the operand:
//                     IQ   L != R                      operands as they are (NULL is a value of its own)
//                     LT   L >= 0 && R >= 0 && L < R   L: -1 -> INT_MAX             so that it is   L' < R'
//                     GT   L >= 0 && R >= 0 && L > R   L: -v, -1 -> INT_MAX;  R: -v, -1 -> INT_MIN   so that it is   L' < R'
//   k_dc_pairs    one lane = one t1 position (DC_T1 per workgroup, operands in registers); the t2 operands of the positions the
//                 workgroup's groups cover go through LDS in tiles of DC_T2 and are read as wave-wide broadcasts, four at a time;
//                 a position counts for a lane when it lies in the lane's group.  A wave walks only the span of its own lanes'
//                 groups (millions of tiny groups: ~64 + |g| positions per wave) and stops once every lane has a witness; the
//                 workgroup stops when no lane needs a later tile.  One launch covers at most `window` t2 positions per workgroup
//                 (window * n <= DC_LAUNCH_PAIRS pair evaluations); later launches start from the mask and skip marked rows.
// Integer compares only; the mask is written with plain byte stores (idempotent: 0 -> 1).
// Order constraints (rgbm_table_detect_dc_scan): EQ predicates plus one or two LT / GT and no IQ need no pairs.  After the same grouping
// and folding every predicate is  L' < R',  so row i violates iff its group holds a j with  L1 < R1[j]  (and  L2 < R2[j]):
//   one predicate    L1 < max R1 of the group
//   two predicates   a 2-D dominance query: the group's positions sorted by R1, suf[p] = max R2 over the sorted positions p .. end of
//                    the group; with p = the first sorted position whose R1 > L1 the row violates iff p exists and suf[p] > L2
//   k_dc_sort_keys   position -> (group's first position << 32) | (R1 with the sign bit flipped): ascending = by group, then by R1
//   (rocPRIM)        radix_sort_pairs of those keys with R2 as the payload, temporary storage from the pool
//   k_dc_tile_runs / k_dc_tile_carry / k_dc_suffix_max   the segmented suffix maximum, a segment = a run of equal groups: each tile
//                    of DC_SCAN_TILE positions reports the run it starts with (group, maximum, "reaches the tile's end"), ONE workgroup
//                    joins those right to left (a group may straddle any number of tiles), each tile scans again with what follows it.
//                    The one-predicate form scans R1 in group order as it lies: suf[first position of the group] = the group's maximum
//   k_dc_lookup      one lane = one t1 position: (two predicates: binary search of L1 among the group's sorted keys, <= 31 steps,) test, byte store
// O(n log n) whatever the groups are; nothing is refused for its pair count.
// Single tuple: one bit per (column, code) -- k_row_bits ANDs them per row in one streaming pass.
// ---------------------------------------------------------------------------------------------
#include "rgbm_prep.h"

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

using namespace rgh;

constexpr int DC_T1 = 256;                          // t1 rows per workgroup, one per lane
constexpr int DC_T2 = 512;                          // t2 rows per LDS tile
constexpr int DC_MAX_PREDS = 16;
constexpr int DC_WAVE_ROUNDS = 4;                   // slots a wave combines before its remaining lanes add on their own
// pair evaluations one launch may cover: 15 ms at the no-early-exit rate measured with two pair predicates (1.11e12 pairs/s), 117 ms with
// fifteen (1.47e11 pairs/s).  RGBM_DC_LAUNCH_PAIRS overrides it (tests: many launches on a small table)
constexpr long long DC_LAUNCH_PAIRS = 1ll << 34;
// default of max_pairs, the sum of |g|^2 a call accepts: 8.8e12 pairs = 8 s without any early exit at two pair predicates, 60 s at fifteen
constexpr long long DC_DEFAULT_MAX_PAIRS = 1ll << 43;

struct DcSide { int32_t col, n_codes; long long rank_off; };          // rank_off: int32 entries into the uploaded rank arrays, -1 = identity
struct DcPair { int32_t op, pad; DcSide l, r; };                     // op: RGBM_DC_IQ / LT / GT
struct DcProgram { int32_t np, pad; DcPair p[DC_MAX_PREDS]; };

__global__ __launch_bounds__(256) void k_dc_slots(const int32_t* __restrict__ codes, long long n, KeySpec ks, unsigned long long* __restrict__ keys,
                                                  unsigned* __restrict__ count, unsigned long long cap_mask, unsigned* __restrict__ row_slot,
                                                  unsigned* __restrict__ row_rank) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;                     // no early return: every lane takes part in the ballots below
    const unsigned s32 = valid ? (unsigned)ht_claim(keys, cap_mask, row_key<true>(codes, n, ks, i)) : 0u;
    const unsigned rank = wave_add<DC_WAVE_ROUNDS>(count, s32, valid);
    if (valid) { row_slot[i] = s32; row_rank[i] = rank; }
}

// stats[0] += sum of count^2, stats[1] = max count  (n < 2^31: the sum stays below 2^62)
__global__ __launch_bounds__(256) void k_dc_stats(const unsigned* __restrict__ count, unsigned long long cap, unsigned long long* __restrict__ stats) {
    unsigned long long sq = 0, mx = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long c = count[i];
        sq += c * c; mx = c > mx ? c : mx;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sq += __shfl_xor(sq, d);
        const unsigned long long o = __shfl_xor(mx, d); mx = o > mx ? o : mx;
    }
    if (lane_id() == 0 && sq) { atomicAdd(&stats[0], sq); atomicMax(&stats[1], mx); }
}

__device__ __forceinline__ int32_t dc_operand(const int32_t* __restrict__ codes, long long n, long long i, const DcSide& sd, const int32_t* __restrict__ ranks) {
    int32_t v = codes[(long long)sd.col * n + i];
    if (v < 0 || v >= sd.n_codes) return -1;
    return sd.rank_off >= 0 ? ranks[sd.rank_off + v] : v;
}

__global__ __launch_bounds__(256) void k_dc_scatter(const int32_t* __restrict__ codes, long long n, DcProgram pg, const int32_t* __restrict__ ranks,
                                                    const unsigned* __restrict__ row_slot, const unsigned* __restrict__ row_rank,
                                                    const long long* __restrict__ goff, const unsigned* __restrict__ count, int32_t* __restrict__ perm,
                                                    int32_t* __restrict__ gbeg, int32_t* __restrict__ gend, int32_t* __restrict__ lop, int32_t* __restrict__ rop) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned s = row_slot[i];
    const long long b = goff[s], pos = b + row_rank[i];
    if (pos < 0 || pos >= n) return;              // (never: the ranks of a slot are 0 .. count - 1)
    perm[pos] = (int32_t)i; gbeg[pos] = (int32_t)b; gend[pos] = (int32_t)(b + count[s]);
    for (int p = 0; p < pg.np; ++p) {
        const int32_t l = dc_operand(codes, n, i, pg.p[p].l, ranks), r = dc_operand(codes, n, i, pg.p[p].r, ranks);
        int32_t lv = l, rv = r;
        if (pg.p[p].op == RGBM_DC_LT) lv = l < 0 ? 0x7FFFFFFF : l;
        else if (pg.p[p].op == RGBM_DC_GT) { lv = l < 0 ? 0x7FFFFFFF : -l; rv = r < 0 ? (int32_t)0x80000000 : -r; }
        lop[(long long)p * n + pos] = lv; rop[(long long)p * n + pos] = rv;
    }
}

template <int NP>
__global__ __launch_bounds__(DC_T1) void k_dc_pairs(const int32_t* __restrict__ lop, const int32_t* __restrict__ rop, const int32_t* __restrict__ gbeg,
                                                    const int32_t* __restrict__ gend, const int32_t* __restrict__ perm, int n, int np, unsigned ne_bits,
                                                    long long w_off, int window, uint8_t* __restrict__ mask) {
    extern __shared__ __align__(16) int32_t dc_sh[];          // [np][DC_T2]: the t2 operands of the tile
    const int tid = threadIdx.x;
    const int p0 = (int)blockIdx.x * DC_T1, pos = p0 + tid, plast = min(p0 + DC_T1, n) - 1;
    const bool valid = pos < n;
    // the positions this workgroup's groups cover, and the slice of them this launch looks at
    const int lo = gbeg[p0], hi = gend[plast];
    if ((long long)lo + w_off >= (long long)hi) return;
    const int wb = (int)(lo + w_off), we = (int)min((long long)wb + window, (long long)hi);
    int row = 0, clo = 0, chi = 0; bool found = true;
    int L[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) L[p] = 0;
    if (valid) {
        row = perm[pos]; found = mask[row] != 0;
        clo = max(gbeg[pos], wb); chi = min(gend[pos], we);
#pragma unroll
        for (int p = 0; p < NP; ++p) if (p < np) L[p] = lop[(long long)p * n + pos];
    }
    const bool had = found;
    if (found || clo >= chi) clo = chi = 0;                   // nothing to look for in this launch
    for (int tb = wb; tb < we; tb += DC_T2) {
        if (!__syncthreads_or(chi > tb)) break;               // also the barrier between the last tile's reads and this tile's writes
        const int te = min(tb + DC_T2, we);
        for (int idx = tid; idx < np * DC_T2; idx += DC_T1) {
            const int p = idx / DC_T2, j = idx % DC_T2;
            if (tb + j < te) dc_sh[idx] = rop[(long long)p * n + tb + j];
        }
        __syncthreads();
        // the span of this wave's lanes inside the tile
        const bool want = !found && clo < te && chi > tb;
        int a = want ? max(clo, tb) : 0x7FFFFFFF, b = want ? min(chi, te) : (int)0x80000000;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { a = min(a, __shfl_xor(a, d)); b = max(b, __shfl_xor(b, d)); }
        const unsigned span = (unsigned)(chi - clo);
        for (int j = (a - tb) & ~3; a < b && j < b - tb; j += 4) {        // (a, b, j are wave-uniform)
            const unsigned rel = (unsigned)(tb + j - clo);
            bool ok0 = rel < span, ok1 = rel + 1u < span, ok2 = rel + 2u < span, ok3 = rel + 3u < span;   // position inside the lane's group (and the launch's slice)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (p < np) {
                    const int4 r = *reinterpret_cast<const int4*>(&dc_sh[p * DC_T2 + j]);        // one address for the whole wave: a broadcast
                    const bool ne = (ne_bits >> p) & 1u;
                    ok0 = ok0 && ((L[p] < r.x) || (ne && L[p] > r.x));
                    ok1 = ok1 && ((L[p] < r.y) || (ne && L[p] > r.y));
                    ok2 = ok2 && ((L[p] < r.z) || (ne && L[p] > r.z));
                    ok3 = ok3 && ((L[p] < r.w) || (ne && L[p] > r.w));
                }
            }
            found = found || ok0 || ok1 || ok2 || ok3;
            if ((j & 60) == 60 && __all(found || clo == chi)) break;      // every lane of the wave has its witness
        }
        if (found) clo = chi = 0;
    }
    if (valid && found && !had) mask[row] = 1;
}

// ---- order constraints: sort, segmented suffix maximum, lookup
constexpr int DC_SCAN_TILE = 1024;                  // positions per workgroup of the suffix-max scan: 256 lanes x 4 consecutive positions
constexpr int DC_SCAN_ITEMS = DC_SCAN_TILE / 256;
constexpr int32_t DC_NO_VAL = (int32_t)0x80000000;  // identity of the maximum
constexpr int32_t DC_SEG_PAD = -1;                  // segment of the positions beyond n (a real segment is a position: >= 0)
constexpr int32_t DC_SEG_END = -2;                  // segment of "nothing follows"

__global__ __launch_bounds__(256) void k_dc_sort_keys(const int32_t* __restrict__ gbeg, const int32_t* __restrict__ r1, long long n,
                                                      unsigned long long* __restrict__ key) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) key[p] = ((unsigned long long)(unsigned)gbeg[p] << 32) | (unsigned long long)((unsigned)r1[p] ^ 0x80000000u);
}

// A range of positions seen from its left end: the segment of its first position, the maximum over the run of that segment which
// starts there, and whether that run reaches the end of the range.  dc_join(a, b): the range a followed by the range b; "nothing
// follows" (DC_SEG_END) leaves a as it is, still open: a tile's range must stay open for the tiles behind it.
struct DcRun { int32_t seg, open, val; };
__device__ __forceinline__ DcRun dc_join(const DcRun& a, const DcRun& b) {
    const bool ext = a.open && a.seg == b.seg;
    const bool end = b.seg == DC_SEG_END;
    return DcRun{a.seg, end ? a.open : (ext ? b.open : 0), ext ? max(a.val, b.val) : a.val};
}
__device__ __forceinline__ DcRun dc_shfl_down(const DcRun& a, int d) { return DcRun{__shfl_down(a.seg, d), __shfl_down(a.open, d), __shfl_down(a.val, d)}; }

// What follows this lane's range: the ranges of the workgroup's later lanes (each lane holds a range, lane order = position order), then
// `tail`.  Every lane of the 256 calls it; a workgroup that calls it again puts a __syncthreads() in between.
__device__ __forceinline__ DcRun dc_right_of(const DcRun& mine, const DcRun& tail) {
    __shared__ DcRun wagg[4];
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
    DcRun inc = mine;                             // the ranges of lanes lane .. min(lane + 2d, 64) - 1 of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const DcRun o = dc_shfl_down(inc, d);
        if (lane + d < 64) inc = dc_join(inc, o);
    }
    if (lane == 0) wagg[w] = inc;
    __syncthreads();
    DcRun r = tail;
    for (int k = 3; k > w; --k) r = dc_join(wagg[k], r);
    const DcRun nx = dc_shfl_down(inc, 1);
    if (lane < 63) r = dc_join(nx, r);
    return r;
}

__device__ __forceinline__ int32_t dc_seg(int32_t g) { return g; }
__device__ __forceinline__ int32_t dc_seg(unsigned long long key) { return (int32_t)(key >> 32); }

// the DC_SCAN_ITEMS consecutive positions of this lane: segments, the suffix maximum inside the lane, and the lane's range
template <typename SegT>
__device__ __forceinline__ DcRun dc_scan_lane(const SegT* __restrict__ seg, const int32_t* __restrict__ val, long long n, long long q0,
                                              int32_t (&sg)[DC_SCAN_ITEMS], int32_t (&loc)[DC_SCAN_ITEMS]) {
    int32_t v[DC_SCAN_ITEMS];
    if (q0 + DC_SCAN_ITEMS <= n) {                // 16 B (values, int32 segments) or 2 x 16 B (keys) per lane; q0 is a multiple of 4
        const int4 v4 = *reinterpret_cast<const int4*>(val + q0);
        v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
#pragma unroll
        for (int i = 0; i < DC_SCAN_ITEMS; ++i) sg[i] = dc_seg(seg[q0 + i]);
    } else {
#pragma unroll
        for (int i = 0; i < DC_SCAN_ITEMS; ++i) {
            const bool in = q0 + i < n;
            sg[i] = in ? dc_seg(seg[q0 + i]) : DC_SEG_PAD; v[i] = in ? val[q0 + i] : DC_NO_VAL;
        }
    }
    bool one = true;
    int32_t run = DC_NO_VAL;
#pragma unroll
    for (int i = DC_SCAN_ITEMS - 1; i >= 0; --i) {
        if (i + 1 < DC_SCAN_ITEMS && sg[i] != sg[i + 1]) { run = DC_NO_VAL; one = false; }
        run = max(run, v[i]); loc[i] = run;
    }
    return DcRun{sg[0], one ? 1 : 0, loc[0]};
}

// tile_run[tile] = the range of the tile
template <typename SegT>
__global__ __launch_bounds__(256) void k_dc_tile_runs(const SegT* __restrict__ seg, const int32_t* __restrict__ val, long long n, DcRun* __restrict__ tile_run) {
    static_assert(DC_SCAN_ITEMS == 4, "dc_scan_lane loads four values as one int4");
    int32_t sg[DC_SCAN_ITEMS], loc[DC_SCAN_ITEMS];
    const DcRun mine = dc_scan_lane(seg, val, n, (long long)blockIdx.x * DC_SCAN_TILE + (long long)threadIdx.x * DC_SCAN_ITEMS, sg, loc);
    const DcRun r = dc_right_of(mine, DcRun{DC_SEG_END, 0, DC_NO_VAL});
    if (threadIdx.x == 0) tile_run[blockIdx.x] = dc_join(mine, r);
}

// in place, ONE workgroup: tile_run[t] = the range of tiles t .. ntiles - 1, 256 tiles per round from the right
__global__ __launch_bounds__(256) void k_dc_tile_carry(DcRun* __restrict__ tile_run, long long ntiles) {
    __shared__ DcRun carry;
    DcRun tail{DC_SEG_END, 0, DC_NO_VAL};
    for (long long c0 = (ntiles - 1) / 256 * 256; c0 >= 0; c0 -= 256) {
        const long long t = c0 + threadIdx.x;
        const DcRun mine = t < ntiles ? tile_run[t] : DcRun{DC_SEG_PAD, 0, DC_NO_VAL};
        const DcRun inc = dc_join(mine, dc_right_of(mine, tail));
        if (t < ntiles) tile_run[t] = inc;
        if (threadIdx.x == 0) carry = inc;
        __syncthreads();                          // also the barrier between this round's reads of dc_right_of's LDS and the next round's writes
        tail = carry;
    }
}

// suf[p] = max of val over p .. the end of p's segment; tile_run as k_dc_tile_carry left it
template <typename SegT>
__global__ __launch_bounds__(256) void k_dc_suffix_max(const SegT* __restrict__ seg, const int32_t* __restrict__ val, long long n,
                                                       const DcRun* __restrict__ tile_run, int32_t* __restrict__ suf) {
    int32_t sg[DC_SCAN_ITEMS], loc[DC_SCAN_ITEMS];
    const long long q0 = (long long)blockIdx.x * DC_SCAN_TILE + (long long)threadIdx.x * DC_SCAN_ITEMS;
    const DcRun mine = dc_scan_lane(seg, val, n, q0, sg, loc);
    const DcRun tail = blockIdx.x + 1u < gridDim.x ? tile_run[blockIdx.x + 1u] : DcRun{DC_SEG_END, 0, DC_NO_VAL};
    const DcRun r = dc_right_of(mine, tail);
    const int32_t more = r.seg == sg[DC_SCAN_ITEMS - 1] ? r.val : DC_NO_VAL;      // what follows continues the lane's last segment
#pragma unroll
    for (int i = 0; i < DC_SCAN_ITEMS; ++i) if (sg[i] == sg[DC_SCAN_ITEMS - 1]) loc[i] = max(loc[i], more);
    if (q0 + DC_SCAN_ITEMS <= n) *reinterpret_cast<int4*>(suf + q0) = make_int4(loc[0], loc[1], loc[2], loc[3]);
    else {
#pragma unroll
        for (int i = 0; i < DC_SCAN_ITEMS; ++i) if (q0 + i < n) suf[q0 + i] = loc[i];
    }
}

// one lane = one t1 position.  TWO: skey = the group's positions sorted by (group, R1), suf over R2 in that order, lop = [2][n];
// otherwise suf over R1 in group order and the group's first position holds its maximum.
template <bool TWO>
__global__ __launch_bounds__(256) void k_dc_lookup(const int32_t* __restrict__ lop, const int32_t* __restrict__ gbeg, const int32_t* __restrict__ gend,
                                                   const int32_t* __restrict__ perm, long long n, const unsigned long long* __restrict__ skey,
                                                   const int32_t* __restrict__ suf, uint8_t* __restrict__ mask) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int32_t b = gbeg[p], l1 = lop[p];
    bool hit;
    if (!TWO) hit = l1 < suf[b];
    else {
        const int32_t e = gend[p];
        const unsigned long long k = ((unsigned long long)(unsigned)b << 32) | (unsigned long long)((unsigned)l1 ^ 0x80000000u);
        int32_t lo = b, hi = e;                   // the first sorted position of the group whose R1 > L1 (signed, through the flipped bit)
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (skey[mid] > k) hi = mid; else lo = mid + 1;
        }
        hit = lo < e && suf[lo] > lop[n + p];
    }
    if (hit) mask[perm[p]] = 1;
}

struct RowBitDesc { int32_t col, n_codes; long long bit_off; int32_t n_words, pad; };      // bit_off: 64-bit words; n_codes + 1 bits, the last one = NULL

// single-tuple constraints: flag = AND over the listed columns of "the bit of the row's code is set".  grid (nblk, 1); the bitset of each
// column goes through the LDS staging of k_detect (up to DET_LDS_WORDS words), one column after the other.  4 B per (row, column).
__global__ __launch_bounds__(PB) void k_row_bits(const int32_t* __restrict__ codes, const RowBitDesc* __restrict__ desc, int ncols,
                                                 const unsigned long long* __restrict__ bits, long long n, unsigned long long* __restrict__ ballots,
                                                 unsigned* __restrict__ bcount) {
    const long long b = blockIdx.x;
    const long long base = b * PROWS;
    bool f[PSUB];
#pragma unroll
    for (int s = 0; s < PSUB; ++s) f[s] = base + (long long)s * PB + threadIdx.x < n;
    for (int j = 0; j < ncols; ++j) {
        const RowBitDesc d = desc[j];
        const int32_t* col = codes + (long long)d.col * n;
        int32_t v[PSUB];
#pragma unroll
        for (int s = 0; s < PSUB; ++s) {             // 16 independent coalesced loads in flight per lane
            const long long r = base + (long long)s * PB + threadIdx.x;
            v[s] = r < n ? col[r] : -1;
        }
        __syncthreads();                             // the last column's tests are done with the staged bitset
        const BitsetView bv = bitset_stage(bits, d.bit_off, d.n_words);
#pragma unroll
        for (int s = 0; s < PSUB; ++s) {
            const unsigned x = (v[s] < 0 || v[s] >= d.n_codes) ? (unsigned)d.n_codes : (unsigned)v[s];     // NULL: the last bit
            f[s] = f[s] && bitset_test(bv, x);
        }
    }
    flags_to_ballots(f, b, ballots, bcount);
}

template <int NP>
void launch_dc_pairs(unsigned nb, size_t lds, hipStream_t s, const int32_t* lop, const int32_t* rop, const int32_t* gbeg, const int32_t* gend,
                     const int32_t* perm, int n, int np, unsigned ne_bits, long long w_off, int window, uint8_t* mask) {
    hipLaunchKernelGGL(k_dc_pairs<NP>, dim3(nb), dim3(DC_T1), lds, s, lop, rop, gbeg, gend, perm, n, np, ne_bits, w_off, window, mask);
}

// ---- what the two two-tuple entries share on the host
// The argument checks (RGBM_ERR_ARG under `entry`'s name, min_preds to 16 predicates): RGBM_OK with the EQ attributes (each once) and
// the predicates evaluated beyond them, or the refusal.
int dc_args(const rgbm_table* t, const rgbm_dc_pred* preds, int32_t n_preds, int min_preds, const int32_t* cell_cols, int32_t n_cell_cols,
            const int64_t* n_cells_out, const char* entry, std::vector<int32_t>& eq, std::vector<const rgbm_dc_pred*>& others) {
    if (!t || !preds || n_preds < min_preds || n_preds > DC_MAX_PREDS || n_cell_cols < 0 || (n_cell_cols > 0 && !cell_cols) || !n_cells_out)
        return fail(RGBM_ERR_ARG, std::string(entry) + ": bad argument (" + std::to_string(min_preds) + " to 16 predicates)");
    for (int i = 0; i < n_preds; ++i) {
        const rgbm_dc_pred& p = preds[i];
        if (p.op < RGBM_DC_EQ || p.op > RGBM_DC_GT) return fail(RGBM_ERR_ARG, std::string(entry) + ": unknown predicate");
        if (p.left_col < 0 || p.left_col >= t->c || p.right_col < 0 || p.right_col >= t->c)
            return fail(RGBM_ERR_ARG, std::string(entry) + ": column index out of range");
        if ((p.op == RGBM_DC_EQ || p.op == RGBM_DC_IQ) && (p.left_col != p.right_col || p.left_rank || p.right_rank))
            return fail(RGBM_ERR_ARG, std::string(entry) + ": EQ / IQ take one attribute on both sides and no rank arrays");
        if (p.op != RGBM_DC_EQ) others.push_back(&p);
        else if (std::find(eq.begin(), eq.end(), p.left_col) == eq.end()) eq.push_back(p.left_col);
    }
    if (eq.size() > 12) return fail(RGBM_ERR_ARG, std::string(entry) + ": at most 12 EQ attributes");
    return refuse_cols(*t, cell_cols, n_cell_cols, false, nullptr, entry);
}

// the program: operands per predicate beyond EQ, the rank arrays one after the other; bit i of ne_bits = predicate i is an IQ
struct DcLowered { DcProgram pg; std::vector<int32_t> ranks; unsigned ne_bits = 0; };
void dc_lower(const rgbm_table& t, const std::vector<const rgbm_dc_pred*>& others, DcLowered& lw) {
    memset(&lw.pg, 0, sizeof(lw.pg)); lw.pg.np = (int32_t)others.size();
    auto side = [&](int32_t col, const int32_t* rank) {
        DcSide sd; sd.col = col; sd.n_codes = std::max<int32_t>(t.n_codes[col], 0); sd.rank_off = -1;
        if (rank) { sd.rank_off = (long long)lw.ranks.size(); lw.ranks.insert(lw.ranks.end(), rank, rank + sd.n_codes); }
        return sd;
    };
    for (size_t i = 0; i < others.size(); ++i) {
        lw.pg.p[i].op = others[i]->op;
        lw.pg.p[i].l = side(others[i]->left_col, others[i]->left_rank);
        lw.pg.p[i].r = side(others[i]->right_col, others[i]->right_rank);
        if (others[i]->op == RGBM_DC_IQ) lw.ne_bits |= 1u << i;
    }
    for (int32_t& v : lw.ranks) if (v < 0) v = -1;
}

// k_dc_slots: the hash table of the EQ key, the rows per slot, every row's slot and arrival rank (enqueued on s)
struct DcSlots { unsigned long long cap = 0; DevBuf<unsigned long long> keys; DevBuf<unsigned> count, row_slot, row_rank; };
void dc_slots(const rgbm_table& t, const KeySpec& ks, unsigned __int128 span, hipStream_t s, DcSlots& g) {
    const long long n = t.n;
    g.cap = table_capacity(n, span);
    g.keys.alloc((size_t)g.cap); g.count.alloc((size_t)g.cap); g.row_slot.alloc((size_t)n); g.row_rank.alloc((size_t)n);
    HIPCHK(hipMemsetAsync(g.keys.p, 0xFF, (size_t)g.cap * 8, s));
    g.count.zero(s);
    hipLaunchKernelGGL(k_dc_slots, dim3(nblocks(n, 256)), dim3(256), 0, s, t.codes.p, n, ks, g.keys.p, g.count.p, g.cap - 1, g.row_slot.p, g.row_rank.p);
}

// k_scan_counts + k_dc_scatter: the rows laid out by group with their folded operands (enqueued on s).  Nothing of `g` is released here:
// k_dc_slots may still be running, and a buffer goes back to the pool only after a synchronise of the stream that used it.
struct DcLayout { DevBuf<long long> goff; DevBuf<int32_t> perm, gbeg, gend, lop, rop, d_ranks; };
void dc_layout(const rgbm_table& t, const DcLowered& lw, const DcSlots& g, hipStream_t s, DcLayout& y) {
    const long long n = t.n;
    y.goff.alloc((size_t)g.cap + 1);
    launch_scan_counts(g.count.p, (long long)g.cap, y.goff.p, y.goff.p + g.cap, s);
    y.perm.alloc((size_t)n); y.gbeg.alloc((size_t)n); y.gend.alloc((size_t)n);
    y.lop.alloc((size_t)lw.pg.np * n); y.rop.alloc((size_t)lw.pg.np * n); y.d_ranks.alloc(std::max<size_t>(lw.ranks.size(), 1));
    y.d_ranks.upload(lw.ranks.data(), lw.ranks.size(), s);
    hipLaunchKernelGGL(k_dc_scatter, dim3(nblocks(n, 256)), dim3(256), 0, s, t.codes.p, n, lw.pg, y.d_ranks.p, g.row_slot.p, g.row_rank.p, y.goff.p, g.count.p,
                       y.perm.p, y.gbeg.p, y.gend.p, y.lop.p, y.rop.p);
}

// suf [n] = the segmented suffix maximum of val [n], the segments from seg [n] (int32 segments or sort keys whose high word is the segment)
template <typename SegT>
void dc_suffix_max(const SegT* seg, const int32_t* val, long long n, DcRun* tile_run, int32_t* suf, hipStream_t s) {
    const long long ntiles = (n + DC_SCAN_TILE - 1) / DC_SCAN_TILE;
    hipLaunchKernelGGL(k_dc_tile_runs<SegT>, dim3((unsigned)ntiles), dim3(256), 0, s, seg, val, n, tile_run);
    hipLaunchKernelGGL(k_dc_tile_carry, dim3(1), dim3(256), 0, s, tile_run, ntiles);
    hipLaunchKernelGGL(k_dc_suffix_max<SegT>, dim3((unsigned)ntiles), dim3(256), 0, s, seg, val, n, (const DcRun*)tile_run, suf);
}

}  // namespace

extern "C" {

// scratch slots held together: ROW_MASK | BALLOTS BCOUNT BOFF | COLS          (its hash table and operands are DevBufs)
RGBM_EXPORT int rgbm_table_detect_dc(rgbm_table* t, const rgbm_dc_pred* preds, int32_t n_preds, const int32_t* cell_cols, int32_t n_cell_cols,
                                     int64_t max_pairs, int64_t* n_rows_out, int64_t* n_cells_out) {
    std::vector<int32_t> eq;
    std::vector<const rgbm_dc_pred*> others;
    if (const int rc = dc_args(t, preds, n_preds, 2, cell_cols, n_cell_cols, n_cells_out, "rgbm_table_detect_dc", eq, others)) return rc;
    if (t->n >= (1ll << 31)) return fail(RGBM_ERR_PARAM, "rgbm_table_detect_dc: 2^31 rows or more");
    return guarded([&]() {
        use_device(t->device);
        unsigned __int128 span = 1;
        const KeySpec ks = key_spec(*t, eq.data(), (int)eq.size(), "rgbm_table_detect_dc", &span);
        const long long n = t->n;
        const long long limit = max_pairs > 0 ? (long long)max_pairs : DC_DEFAULT_MAX_PAIRS;
        DcLowered lw; dc_lower(*t, others, lw);
        const DcProgram& pg = lw.pg;
        const unsigned ne_bits = lw.ne_bits;
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        uint8_t* mask = scr<uint8_t>(*t, SCR_ROW_MASK, (size_t)std::max<long long>(n, 1));
        if (n == 0) return no_cells(*t, true, n_rows_out, n_cells_out);
        if (pg.np == 0) {
            // EQ predicates only: t2 = t1 satisfies them, every row violates
            HIPCHK(hipMemsetAsync(mask, 1, (size_t)n, s));
        } else {
            DcSlots g; dc_slots(*t, ks, span, s, g);
            DevBuf<unsigned long long> stats(2);
            stats.zero(s);
            hipLaunchKernelGGL(k_dc_stats, dim3((unsigned)std::min<unsigned long long>((g.cap + 255) / 256, 2048ull)), dim3(256), 0, s, g.count.p, g.cap, stats.p);
            HIPCHK(hipGetLastError());
            unsigned long long h_stats[2] = {0, 0};
            HIPCHK(hipMemcpyAsync(h_stats, stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (h_stats[0] > (unsigned long long)limit)
                throw std::invalid_argument("rgbm_table_detect_dc: the groups of the EQ attributes hold " + std::to_string(h_stats[0]) +
                                            " pairs, more than max_pairs = " + std::to_string(limit));
            g.keys.release();                         // (the stream is synchronised: k_dc_slots is done with them)
            DcLayout y; dc_layout(*t, lw, g, s, y);
            HIPCHK(hipMemsetAsync(mask, 0, (size_t)n, s));
            // launches: every workgroup looks at `window` t2 positions of its span per launch; a span is at most DC_T1 + 2 max|g| positions
            long long launch_pairs = DC_LAUNCH_PAIRS;
            if (const char* e = getenv("RGBM_DC_LAUNCH_PAIRS")) { const long long v = atoll(e); if (v > 0) launch_pairs = v; }
            long long window = std::max<long long>(launch_pairs / n / DC_T2, 1) * DC_T2;
            const long long max_span = std::min<long long>(DC_T1 + 2 * (long long)h_stats[1], n);
            window = std::min<long long>(std::min<long long>(window, (max_span + DC_T2 - 1) / DC_T2 * DC_T2), 1ll << 30);
            const unsigned nbp = nblocks(n, DC_T1);
            const size_t lds = (size_t)pg.np * DC_T2 * sizeof(int32_t);
            for (long long w_off = 0; w_off < max_span; w_off += window) {
                if (pg.np <= 2) launch_dc_pairs<2>(nbp, lds, s, y.lop.p, y.rop.p, y.gbeg.p, y.gend.p, y.perm.p, (int)n, pg.np, ne_bits, w_off, (int)window, mask);
                else if (pg.np <= 4) launch_dc_pairs<4>(nbp, lds, s, y.lop.p, y.rop.p, y.gbeg.p, y.gend.p, y.perm.p, (int)n, pg.np, ne_bits, w_off, (int)window, mask);
                else if (pg.np <= 8) launch_dc_pairs<8>(nbp, lds, s, y.lop.p, y.rop.p, y.gbeg.p, y.gend.p, y.perm.p, (int)n, pg.np, ne_bits, w_off, (int)window, mask);
                else launch_dc_pairs<16>(nbp, lds, s, y.lop.p, y.rop.p, y.gbeg.p, y.gend.p, y.perm.p, (int)n, pg.np, ne_bits, w_off, (int)window, mask);
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));          // the temporaries go back to the pool
        }
        const long long m = compact<1>(*t, mask, nullptr, 1, false, s);     // ascending violating rows
        rows_to_cells(*t, m, cell_cols, n_cell_cols, s, n_rows_out, n_cells_out);
        return RGBM_OK;
    });
}

// scratch slots held together: ROW_MASK | BALLOTS BCOUNT BOFF | COLS          (hash table, operands, sort buffers and scan state are DevBufs)
RGBM_EXPORT int rgbm_table_detect_dc_scan(rgbm_table* t, const rgbm_dc_pred* preds, int32_t n_preds, const int32_t* cell_cols, int32_t n_cell_cols,
                                          int64_t* n_rows_out, int64_t* n_cells_out) {
    std::vector<int32_t> eq;
    std::vector<const rgbm_dc_pred*> others;
    if (const int rc = dc_args(t, preds, n_preds, 1, cell_cols, n_cell_cols, n_cells_out, "rgbm_table_detect_dc_scan", eq, others)) return rc;
    for (const rgbm_dc_pred* p : others)
        if (p->op == RGBM_DC_IQ) return fail(RGBM_ERR_PARAM, "rgbm_table_detect_dc_scan: an IQ predicate takes the pairs of rgbm_table_detect_dc");
    if (others.empty() || others.size() > 2)
        return fail(RGBM_ERR_PARAM, "rgbm_table_detect_dc_scan: one or two LT / GT predicates (" + std::to_string(others.size()) + " given)");
    if (t->n >= (1ll << 31)) return fail(RGBM_ERR_PARAM, "rgbm_table_detect_dc_scan: 2^31 rows or more");
    return guarded([&]() {
        use_device(t->device);
        unsigned __int128 span = 1;
        const KeySpec ks = key_spec(*t, eq.data(), (int)eq.size(), "rgbm_table_detect_dc_scan", &span);
        const long long n = t->n;
        DcLowered lw; dc_lower(*t, others, lw);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        uint8_t* mask = scr<uint8_t>(*t, SCR_ROW_MASK, (size_t)std::max<long long>(n, 1));
        if (n == 0) return no_cells(*t, true, n_rows_out, n_cells_out);
        {
            DcSlots g; dc_slots(*t, ks, span, s, g);
            DcLayout y; dc_layout(*t, lw, g, s, y);
            HIPCHK(hipMemsetAsync(mask, 0, (size_t)n, s));
            DevBuf<DcRun> tile_run((size_t)((n + DC_SCAN_TILE - 1) / DC_SCAN_TILE));
            DevBuf<int32_t> suf((size_t)n);
            const unsigned nb = nblocks(n, 256);
            if (lw.pg.np == 1) {
                dc_suffix_max(y.gbeg.p, y.rop.p, n, tile_run.p, suf.p, s);
                hipLaunchKernelGGL(k_dc_lookup<false>, dim3(nb), dim3(256), 0, s, y.lop.p, y.gbeg.p, y.gend.p, y.perm.p, n, (const unsigned long long*)nullptr,
                                   suf.p, mask);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(s));
            } else {
                DevBuf<unsigned long long> key((size_t)n), skey((size_t)n);
                DevBuf<int32_t> sval((size_t)n);
                hipLaunchKernelGGL(k_dc_sort_keys, dim3(nb), dim3(256), 0, s, y.gbeg.p, y.rop.p, n, key.p);
                HIPCHK(hipGetLastError());
                unsigned end_bit = 33;                // the low word and the bits of the largest first position, n - 1
                while (end_bit < 64 && ((unsigned long long)(n - 1) >> (end_bit - 32))) ++end_bit;
                size_t tmp_bytes = 0;
                HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key.p, skey.p, y.rop.p + n, sval.p, (size_t)n, 0u, end_bit, s));
                DevBuf<char> tmp(std::max<size_t>(tmp_bytes, 1));
                HIPCHK(rocprim::radix_sort_pairs((void*)tmp.p, tmp_bytes, key.p, skey.p, y.rop.p + n, sval.p, (size_t)n, 0u, end_bit, s));
                dc_suffix_max(skey.p, sval.p, n, tile_run.p, suf.p, s);
                hipLaunchKernelGGL(k_dc_lookup<true>, dim3(nb), dim3(256), 0, s, y.lop.p, y.gbeg.p, y.gend.p, y.perm.p, n, (const unsigned long long*)skey.p,
                                   suf.p, mask);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(s));      // the temporaries go back to the pool
            }
        }
        const long long m = compact<1>(*t, mask, nullptr, 1, false, s);     // ascending violating rows
        rows_to_cells(*t, m, cell_cols, n_cell_cols, s, n_rows_out, n_cells_out);
        return RGBM_OK;
    });
}

// scratch slots held together: TABLE_A (descriptors) TABLE_B (bitsets) BALLOTS BCOUNT BOFF | COLS
RGBM_EXPORT int rgbm_table_detect_row_bits(rgbm_table* t, const int32_t* cols, int32_t n_cols, const uint64_t* const* bits, const int32_t* cell_cols,
                                           int32_t n_cell_cols, int64_t* n_rows_out, int64_t* n_cells_out) {
    if (!t || n_cols < 1 || !cols || !bits || n_cell_cols < 0 || (n_cell_cols > 0 && !cell_cols) || !n_cells_out)
        return fail(RGBM_ERR_ARG, "rgbm_table_detect_row_bits: bad argument (at least one column)");
    if (const int rc = refuse_cols(*t, cols, n_cols, true, bits, "rgbm_table_detect_row_bits")) return rc;
    if (const int rc = refuse_cols(*t, cell_cols, n_cell_cols, false, nullptr, "rgbm_table_detect_row_bits")) return rc;
    return guarded([&]() {
        use_device(t->device);
        // one descriptor per column; the bitsets one after the other, bits beyond the NULL bit cleared
        std::vector<RowBitDesc> desc((size_t)n_cols);
        std::vector<unsigned long long> words;
        for (int i = 0; i < n_cols; ++i) {
            RowBitDesc& d = desc[i];
            d.col = cols[i]; d.n_codes = std::max<int32_t>(t->n_codes[cols[i]], 0); d.pad = 0;
            d.bit_off = append_bitset(words, bits[i], (long long)d.n_codes + 1, &d.n_words);
        }
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (t->n == 0) return no_cells(*t, true, n_rows_out, n_cells_out);
        const Ballots b = table_ballots(*t, 1);
        const RowBitDesc* d_desc = scr_upload<RowBitDesc>(*t, SCR_TABLE_A, desc.data(), desc.size(), s);
        const unsigned long long* d_bits = scr_upload<unsigned long long>(*t, SCR_TABLE_B, words.data(), words.size(), s);
        hipLaunchKernelGGL(k_row_bits, dim3((unsigned)b.nblk, 1u), dim3(PB), 0, s, t->codes.p, d_desc, (int)n_cols, d_bits, (long long)t->n, b.ballots, b.bcount);
        const long long m = emit_to_table(*t, b, nullptr, s);
        rows_to_cells(*t, m, cell_cols, n_cell_cols, s, n_rows_out, n_cells_out);
        return RGBM_OK;
    });
}

}  // extern "C"
