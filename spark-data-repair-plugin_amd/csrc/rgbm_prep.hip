// rgbm_prep.hip -- the relational steps either side of the repair models, on the HBM-resident code table
// (SURVEY.md 8(f) rows 2-4).  Everything here is HBM-bound integer work over int32 codes [c][n]:
//
//   detect_nulls          NullErrorDetector                      (reference: ErrorDetectorApi.scala:128-157)
//   detect_constraint     ConstraintErrorDetector for  X1..Xm -> Y  style denial constraints
//                         t1&t2&EQ(t1.X,t2.X)&..&IQ(t1.Y,t2.Y)     (ErrorDetectorApi.scala:189-244)
//   detect_dc / row_bits  ConstraintErrorDetector for every other parsed constraint: all-pairs predicates inside the EQ groups; constants
//                         as one bit per (column, code)   (end of this file; repair/dc_codes.py builds the programs)
//   detect_cells          RegEx / DomainValues / GaussianOutlier detectors as predicates on the dictionary codes, NULL detector fused in
//                         (ErrorDetectorApi.scala:159-187, 249-300; repair/detect_codes.py builds the predicates)
//   null_cells            convertErrorCellsToNull                 (RepairApi.scala:171-211)
//   rows_of_cells         clean / dirty row split                 (python/repair/model.py:549-553)
//   gather_rows           the dirty-row table
//   count_codes           per-code row counts of a column (class weights, domain statistics)
//   column_stats          distinct / NULL counts, min / max, value lengths and equi-height histogram edges of many columns in one call
//                         (RepairMiscApi.computeAndGetStats in code space; repair/table_stats.py is the statement)
//   encode_dict           dictionary indices -> sorted-rank codes (replaces the pandas encoders, model.py:701-729)
//   repair_pmf[_weighted] candidate distributions of the NULL cells, optionally re-weighted by update costs (rgbm_cost.h)
//   edit_distance         Levenshtein matrix of two string pools (the Levenshtein update cost, rgbm_cost.h)
//   kmeans_assign / read  one Lloyd step of the q-gram k-means of RepairMisc.splitInputTable, in code space (RepairMiscApi.scala:52-153)
//
// Result lists are ORDERED (by position in the column list, then ascending row), so the output is a deterministic
// function of the input: the device stream compaction is two passes (coalesced flag pass that leaves 64-row ballots
// behind, exclusive scan of the per-block counts, emit pass over the ballots) and never uses arrival order.
// Every later section uses the ONE copy of each mechanism that this first section holds -- compaction: flags_to_ballots, scan_emit (into the
// table's cell list: emit_to_table, compact<MODE>), rows_to_cells;  keys: key_digit / row_key, key_spec, table_capacity, ht_claim, wave_add;
// bitsets: append_bitset, bitset_stage / bitset_test;  scratch: enum Scr, with its rule; every entry point names its slots above its definition.
#include "rgbm_host.h"
#include "rgbm_cost.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

using namespace rgh;

constexpr int PB = 256;                 // threads per block
constexpr int PSUB = 16;                // 256-row sub-tiles per block
constexpr int PROWS = PB * PSUB;        // 4096 rows per block
constexpr int PBAL = PROWS / 64;        // 64 ballots per block

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

// the 16 x 256 flags of block (b, j) -> its 64 ballots (ballot q covers rows [b*4096 + q*64, +64)) and its count
__device__ __forceinline__ void flags_to_ballots(const bool (&f)[PSUB], long long e, unsigned long long* __restrict__ ballots,
                                                 unsigned* __restrict__ bcount) {
    __shared__ unsigned wsum[PB / 64];
    unsigned cnt = 0;
    unsigned long long* bo = ballots + e * PBAL;
#pragma unroll
    for (int s = 0; s < PSUB; ++s) {
        const unsigned long long m = __ballot(f[s]);
        if (lane_id() == 0) { bo[s * (PB / 64) + (threadIdx.x >> 6)] = m; cnt += (unsigned)__popcll(m); }
    }
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned t = 0; for (int w = 0; w < PB / 64; ++w) t += wsum[w]; bcount[e] = t; }
}

// ---------------------------------------------------------------------------------------------
// stream compaction, pass 1: flags -> 64-row ballots + per-block count.   grid (nblk, ncols)
//   MODE 0: flag = cell of column cols[blockIdx.y] is NULL;  MODE 1: flag = mask[row] != 0 (blockIdx.y == 0)
//   (MODE 2 of compact<> is k_detect below: same grid, same ballots)
// Algorithmic bytes: 4 B per (row, column) for MODE 0, 1 B per row for MODE 1.
// ---------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(PB) void k_flag(const int32_t* __restrict__ codes, const uint8_t* __restrict__ mask,
                                             const int32_t* __restrict__ cols, long long n, long long nblk,
                                             unsigned long long* __restrict__ ballots, unsigned* __restrict__ bcount) {
    const long long b = blockIdx.x;
    const int j = blockIdx.y;
    const long long base = b * PROWS;
    const int32_t* col = MODE == 0 ? codes + (long long)cols[j] * n : nullptr;
    bool f[PSUB];
#pragma unroll
    for (int s = 0; s < PSUB; ++s) {             // 16 independent coalesced loads in flight per lane
        const long long r = base + (long long)s * PB + threadIdx.x;
        if (MODE == 0) f[s] = r < n ? (col[r] < 0) : false;
        else f[s] = r < n ? (mask[r] != 0) : false;
    }
    flags_to_ballots(f, (long long)j * nblk + b, ballots, bcount);
}

// ---------------------------------------------------------------------------------------------
// pass 1 of the VALUE detectors (regex / value domain / Tukey fences, repair/detect_codes.py): on a label-encoded column each of
// them is a predicate on the dictionary code, so one read of the column answers all of them and the NULL detector.  grid (nblk, ncols)
//   flag = v < 0 ? null_is_error : (range given && (v < keep_lo || v > keep_hi)) || (bitset given && bit v set)
// The bitset of the block's column (1 bit per code) is staged into LDS up to DET_LDS_WORDS 64-bit words (8 KiB = 65536 codes: a
// fifth of what 8 resident workgroups -- the 32 waves a CU holds -- could declare of its 160 KiB, so LDS never costs occupancy, and at
// most half the bytes of the block's 16 KiB row tile); larger ones are read where they lie (small next to the column, L2 resident).
// A column without a bitset never touches one.  Bit tests are on 32-bit halves (little endian: bit v of the 64-bit words is bit v & 31
// of half v >> 5).  Algorithmic bytes: 4 B per (row, column) + the bitset once per block.
// ---------------------------------------------------------------------------------------------
struct DetDesc { int32_t col, null_is_error, keep_lo, keep_hi; long long bit_off; int32_t n_words, pad; };   // bit_off: 64-bit words, -1 = none
constexpr int DET_LDS_WORDS = 1024;

// The bitset of a block's column, n_words 64-bit words at bits + bit_off (bit_off < 0: none, nw32 = 0): staged into LDS (in_lds, uniform over the
// block) or read where it lies.  Every lane calls bitset_stage; a block that restages puts a __syncthreads() between the last tests and the call.
struct BitsetView { const unsigned* g32; const unsigned* lds; unsigned nw32; bool in_lds; };
__device__ __forceinline__ BitsetView bitset_stage(const unsigned long long* __restrict__ bits, long long bit_off, int32_t n_words) {
    __shared__ unsigned lbits[DET_LDS_WORDS * 2];
    const bool has_bits = bit_off >= 0 && n_words > 0;
    const BitsetView v{reinterpret_cast<const unsigned*>(bits + (has_bits ? bit_off : 0)), lbits, has_bits ? 2u * (unsigned)n_words : 0u,
                       has_bits && n_words <= DET_LDS_WORDS};
    if (v.in_lds) {
        for (unsigned i = threadIdx.x; i < v.nw32; i += PB) lbits[i] = v.g32[i];
        __syncthreads();
    }
    return v;
}
__device__ __forceinline__ bool bitset_test(const BitsetView& v, unsigned x) {           // a code beyond the bitset has no bit
    const unsigned w = x >> 5;
    return w < v.nw32 && (((v.in_lds ? v.lds[w] : v.g32[w]) >> (x & 31u)) & 1u);
}

__global__ __launch_bounds__(PB) void k_detect(const int32_t* __restrict__ codes, const DetDesc* __restrict__ desc,
                                               const unsigned long long* __restrict__ bits, long long n, long long nblk,
                                               unsigned long long* __restrict__ ballots, unsigned* __restrict__ bcount) {
    const long long b = blockIdx.x;
    const int j = blockIdx.y;
    const long long base = b * PROWS;
    const DetDesc d = desc[j];
    const int32_t* col = codes + (long long)d.col * n;
    int32_t v[PSUB];
#pragma unroll
    for (int s = 0; s < PSUB; ++s) {             // 16 independent coalesced loads in flight per lane
        const long long r = base + (long long)s * PB + threadIdx.x;
        v[s] = r < n ? col[r] : 0;
    }
    const BitsetView bv = bitset_stage(bits, d.bit_off, d.n_words);
    const bool has_range = d.keep_lo <= d.keep_hi;
    bool f[PSUB];
#pragma unroll
    for (int s = 0; s < PSUB; ++s) {
        const long long r = base + (long long)s * PB + threadIdx.x;
        const int32_t x = v[s];
        bool e;
        if (x < 0) e = d.null_is_error != 0;
        else e = (has_range && (x < d.keep_lo || x > d.keep_hi)) || bitset_test(bv, (unsigned)x);
        f[s] = r < n && e;
    }
    flags_to_ballots(f, (long long)j * nblk + b, ballots, bcount);
}

// exclusive scan of m block counts (one workgroup; 8 entries per thread and step)
__global__ __launch_bounds__(1024) void k_scan_counts(const unsigned* __restrict__ cnt, long long m, long long* __restrict__ off,
                                                      long long* __restrict__ total) {
    __shared__ long long wtot[16];
    __shared__ long long carry_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (long long base = 0; base < m; base += 8192) {
        long long v[8]; long long s = 0;
        const long long i0 = base + (long long)tid * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = (i0 + k < m) ? (long long)cnt[i0 + k] : 0; s += v[k]; }
        long long incl = s;                               // inclusive wave scan of the per-thread sums
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const long long o = __shfl_up(incl, d); if (lane >= d) incl += o; }
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        long long wbase = 0;
        for (int q = 0; q < w; ++q) wbase += wtot[q];
        long long run = carry_s + wbase + incl - s;
#pragma unroll
        for (int k = 0; k < 8; ++k) { if (i0 + k < m) off[i0 + k] = run; run += v[k]; }
        __syncthreads();
        if (tid == 1023) carry_s = run;
        __syncthreads();
    }
    if (tid == 0) *total = carry_s;
}

// pass 2: ballots -> ordered (row, column) cells.   grid (nblk, ncols), one workgroup of 64 lanes x 4 waves
__global__ __launch_bounds__(PB) void k_emit(const unsigned long long* __restrict__ ballots, const long long* __restrict__ off,
                                             const int32_t* __restrict__ cols, long long nblk,
                                             long long* __restrict__ out_rows, int32_t* __restrict__ out_cols) {
    const long long b = blockIdx.x;
    const int j = blockIdx.y;
    const long long e = (long long)j * nblk + b;
    __shared__ unsigned pre[PBAL];
    __shared__ unsigned long long bal[PBAL];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < PBAL) {                        // wave 0: exclusive scan of the 64 ballot popcounts
        const unsigned long long m = ballots[e * PBAL + tid];
        bal[tid] = m;
        const unsigned c = (unsigned)__popcll(m);
        unsigned incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned o = __shfl_up(incl, d); if (lane >= d) incl += o; }
        pre[tid] = incl - c;
    }
    __syncthreads();
    const long long o0 = off[e];
    const int32_t cj = cols ? cols[j] : -1;
#pragma unroll
    for (int s = 0; s < PSUB; ++s) {
        const int q = s * (PB / 64) + w;     // ballot q covers rows [b*4096 + q*64, +64): ascending in q
        const unsigned long long m = bal[q];
        if ((m >> lane) & 1ull) {
            const long long p = o0 + pre[q] + __popcll(m & ((1ull << lane) - 1ull));
            out_rows[p] = b * PROWS + (long long)q * 64 + lane;
            if (out_cols) out_cols[p] = cj;
        }
    }
}

// cells = rows x columns (column-major): the constraint detector reports every given attribute of a violating row
__global__ void k_replicate(const long long* __restrict__ rows, long long m, const int32_t* __restrict__ cols, int ncols,
                            long long* __restrict__ out_rows, int32_t* __restrict__ out_cols) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const long long r = rows[i];
    for (int j = 0; j < ncols; ++j) { out_rows[(long long)j * m + i] = r; out_cols[(long long)j * m + i] = cols[j]; }
}

// ---------------------------------------------------------------------------------------------
// denial constraints EQ(X1)..EQ(Xm) & IQ(Y) on two tuples: open-addressing hash table keyed by the NULL-safe
// mixed-radix code of (X1..Xm); a group remembers the first Y it has seen and a flag "another Y exists"
// .  The violation mask is a pure function of the table -- insertion order is irrelevant.
// Algorithmic bytes per row: 4 B per EQ/IQ column + ~12 B of table traffic per probe, twice (insert, lookup).
// ---------------------------------------------------------------------------------------------
struct KeySpec { int32_t ncols; int32_t col[12]; unsigned long long radix[12]; };
constexpr unsigned long long HT_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31; return x;
}
// digit of a code in the NULL-safe mixed-radix key: code + 1, NULL (-1) -> 0.  CLAMP: a code at or above the column's dictionary (digit >=
// radix) or below -1 counts as NULL, so distinct keys never collide.  Neither rgbm_table_create nor rgbm_table_write_cells refuses such
// codes, and on them the unclamped digit gives other (colliding) keys: rgbm_table_detect_constraint, which has always used it, keeps it
// (CLAMP = false), so that its result stays what it was on every table; the two forms are the same wherever codes lie in [-1, n_codes).
template <bool CLAMP>
__device__ __forceinline__ unsigned long long key_digit(int32_t v, unsigned long long radix) {
    if (!CLAMP) return (unsigned long long)(v + 1);
    return (v < 0 || (unsigned long long)v + 1ull >= radix) ? 0ull : (unsigned long long)v + 1ull;
}
template <bool CLAMP>
__device__ __forceinline__ unsigned long long row_key(const int32_t* __restrict__ codes, long long n, const KeySpec& ks, long long i) {
    unsigned long long k = 0;
    for (int c = 0; c < ks.ncols; ++c) k = k * ks.radix[c] + key_digit<CLAMP>(codes[(long long)ks.col[c] * n + i], ks.radix[c]);
    return k;
}

// The slot of `key` in an open-addressing table of cap_mask + 1 >= 2 x (number of keys) slots, claimed if nobody has.  A slot only ever
// goes EMPTY -> key, so a plain read that already shows the key makes the atomic unnecessary: low-cardinality keys (few groups,
// millions of rows each) would otherwise serialise on a handful of addresses.
__device__ __forceinline__ unsigned long long ht_claim(unsigned long long* __restrict__ keys, unsigned long long cap_mask, unsigned long long key) {
    unsigned long long slot = mix64(key) & cap_mask;
    for (;;) {
        unsigned long long prev = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // read at L2, never a stale L1 line
        if (prev == key) break;
        if (prev == HT_EMPTY) { prev = atomicCAS(&keys[slot], HT_EMPTY, key); if (prev == HT_EMPTY || prev == key) break; }
        slot = (slot + 1) & cap_mask;
    }
    return slot;
}

// count[slot] += 1 for every `active` lane, the lanes of a wave that hold the same slot adding once (one group may span the table and
// would otherwise serialise on one address); after ROUNDS leaders the remaining lanes add on their own.  Returns the lane's arrival
// rank in its slot.  Every lane of the wave calls it.
template <int ROUNDS>
__device__ __forceinline__ unsigned wave_add(unsigned* __restrict__ count, unsigned slot, bool active) {
    const int lane = lane_id();
    unsigned rank = 0;
    unsigned long long pend = __ballot(active);
    for (int round = 0; round < ROUNDS && pend; ++round) {
        const int leader = __ffsll((long long)pend) - 1;
        const unsigned s = (unsigned)__shfl((int)slot, leader);
        const unsigned long long same = __ballot(active && slot == s);      // (a subset of pend: a slot leaves pend with all its lanes)
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&count[s], (unsigned)__popcll(same));
        base = (unsigned)__shfl((int)base, leader);
        if ((same >> lane) & 1ull) rank = base + (unsigned)__popcll(same & ((1ull << lane) - 1ull));
        pend &= ~same;
    }
    if ((pend >> lane) & 1ull) rank = atomicAdd(&count[slot], 1u);
    return rank;
}

__global__ __launch_bounds__(256) void k_ht_insert(const int32_t* __restrict__ codes, long long n, KeySpec ks, int iq_col,
                                                   unsigned long long* __restrict__ keys, unsigned* __restrict__ state, unsigned long long cap_mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long slot = ht_claim(keys, cap_mask, row_key<false>(codes, n, ks, i));
    // the state only grows (0 -> first value -> | "another value"): a read that already shows the final answer needs no atomic either
    const unsigned v = (unsigned)(codes[(long long)iq_col * n + i] + 1) + 1u;            // >= 1; NULL is a value of its own (<=>)
    unsigned old = __hip_atomic_load(&state[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((old >> 31) || old == v) return;
    if (old == 0u) old = atomicCAS(&state[slot], 0u, v);
    if (old != 0u && (old & 0x7FFFFFFFu) != v) atomicOr(&state[slot], 0x80000000u);
}

__global__ __launch_bounds__(256) void k_ht_lookup(const int32_t* __restrict__ codes, long long n, KeySpec ks,
                                                   const unsigned long long* __restrict__ keys, const unsigned* __restrict__ state,
                                                   unsigned long long cap_mask, uint8_t* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = row_key<false>(codes, n, ks, i);
    unsigned long long slot = mix64(key) & cap_mask;
    while (keys[slot] != key) slot = (slot + 1) & cap_mask;
    const unsigned st = state[slot];
    mask[i] = (uint8_t)(st >> 31);
}

// ---------------------------------------------------------------------------------------------
// small scatter / gather kernels
// ---------------------------------------------------------------------------------------------
__global__ void k_null_cells(int32_t* __restrict__ codes, long long n, int c, const long long* __restrict__ rows,
                             const int32_t* __restrict__ cols, long long m, const uint8_t* __restrict__ is_target) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const long long r = rows[i]; const int cc = cols[i];
    if (r < 0 || r >= n || cc < 0 || cc >= c || !is_target[cc]) return;     // cells outside the table / the targets are ignored (join semantics)
    codes[(long long)cc * n + r] = -1;
}

__global__ void k_write_cells(int32_t* __restrict__ codes, long long n, int c, const long long* __restrict__ rows,
                              const int32_t* __restrict__ cols, const int32_t* __restrict__ vals, long long m) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const long long r = rows[i]; const int cc = cols[i];
    if (r < 0 || r >= n || cc < 0 || cc >= c) return;
    codes[(long long)cc * n + r] = vals[i];
}

__global__ void k_read_cells(const int32_t* __restrict__ codes, long long n, int c, const long long* __restrict__ rows,
                             const int32_t* __restrict__ cols, long long m, int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const long long r = rows[i]; const int cc = cols[i];
    out[i] = (r < 0 || r >= n || cc < 0 || cc >= c) ? -1 : codes[(long long)cc * n + r];
}

__global__ void k_mark_rows(uint8_t* __restrict__ mask, long long n, const long long* __restrict__ rows, long long m) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const long long r = rows[i];
    if (r >= 0 && r < n) mask[r] = 1;
}

__global__ void k_gather_rows(const int32_t* __restrict__ in, long long n_in, int32_t* __restrict__ out, long long n_out,
                              const long long* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const int cc = blockIdx.y;
    out[(long long)cc * n_out + i] = in[(long long)cc * n_in + rows[i]];
}

// per-code counts of one column: LDS histogram per workgroup when the domain fits, flushed with global atomics
constexpr int CC_LDS = 8192;
__global__ __launch_bounds__(256) void k_count_codes(const int32_t* __restrict__ col, long long n, int n_codes,
                                                     unsigned long long* __restrict__ counts /* [n_codes + 1], last = NULL */) {
    __shared__ unsigned h[CC_LDS + 1];
    const bool lds = n_codes <= CC_LDS;
    if (lds) { for (int i = threadIdx.x; i <= n_codes; i += blockDim.x) h[i] = 0; __syncthreads(); }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int v = col[i];
        const int b = (v < 0 || v >= n_codes) ? n_codes : v;
        if (lds) atomicAdd(&h[b], 1u); else atomicAdd(&counts[b], 1ull);
    }
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i <= n_codes; i += blockDim.x) if (h[i]) atomicAdd(&counts[i], (unsigned long long)h[i]);
    }
}

// ---------------------------------------------------------------------------------------------
// column statistics (rgbm_table_column_stats; the statement is repair/table_stats.py column_stats): the counts of every listed column in one
// launch, then one workgroup per column reduces its counts to six numbers and the histogram edges.  The counts never leave the device.
//   k_colstat_count   grid (blocks, listed columns): the two regimes of k_count_codes (32-bit LDS counters flushed with 64-bit atomics up to CC_LDS
//                     codes, 64-bit atomics to HBM above); NULL rows per wave by ballot / popcount, one atomic per wave.  4 B per (row, column).
//   k_colstat_reduce  grid (listed columns): walks the counts in chunks of CS_CHUNK codes (CS_ITEMS consecutive codes per lane), a block scan per
//                     chunk and a running sum between chunks: distinct, min, max, len_sum, len_max, and the first code at which the cumulative
//                     count reaches each target rank  ceil(i * m / n_bins)  (m = non-NULL rows; the ranks wait in LDS, and a chunk that no rank
//                     falls into -- all but n_bins of them at most -- skips the selection).  8 B per code, + 4 B with a length LUT.
// ---------------------------------------------------------------------------------------------
struct CsDesc { long long cnt_off, lut_off; int32_t col, n_codes; };       // lut_off < 0: no length LUT
constexpr int CS_UNROLL = 4;              // independent coalesced loads in flight per lane
constexpr int CS_ITEMS = 8;               // consecutive codes per lane and chunk
constexpr int CS_CHUNK = 256 * CS_ITEMS;
constexpr int CS_STATS = 6;               // nulls, distinct, min_code, max_code, len_sum, len_max
constexpr int CS_MAX_BINS = 254;

__global__ __launch_bounds__(256) void k_colstat_count(const int32_t* __restrict__ codes, long long n, const CsDesc* __restrict__ desc,
                                                       unsigned long long* __restrict__ counts, unsigned long long* __restrict__ stats) {
    __shared__ unsigned h[CC_LDS];
    const CsDesc d = desc[blockIdx.y];
    const int nc = d.n_codes;
    const int32_t* col = codes + (long long)d.col * n;
    unsigned long long* cnt = counts + d.cnt_off;
    const bool lds = nc <= CC_LDS;
    if (lds) { for (int i = threadIdx.x; i < nc; i += 256) h[i] = 0; __syncthreads(); }
    unsigned long long nulls = 0;        // of this wave (every lane holds the same number)
    for (long long base = (long long)blockIdx.x * (256 * CS_UNROLL); base < n; base += (long long)gridDim.x * (256 * CS_UNROLL)) {   // uniform over the block
        int v[CS_UNROLL];
#pragma unroll
        for (int s = 0; s < CS_UNROLL; ++s) {
            const long long r = base + (long long)s * 256 + threadIdx.x;
            v[s] = r < n ? col[r] : 0;
        }
#pragma unroll
        for (int s = 0; s < CS_UNROLL; ++s) {
            const bool in = base + (long long)s * 256 + threadIdx.x < n;
            const bool null = in && (v[s] < 0 || v[s] >= nc);
            nulls += (unsigned long long)__popcll(__ballot(null));
            if (in && !null) { if (lds) atomicAdd(&h[v[s]], 1u); else atomicAdd(&cnt[v[s]], 1ull); }
        }
    }
    if (lane_id() == 0 && nulls) atomicAdd(&stats[(long long)blockIdx.y * CS_STATS], nulls);
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < nc; i += 256) if (h[i]) atomicAdd(&cnt[i], (unsigned long long)h[i]);
    }
}

__global__ __launch_bounds__(256) void k_colstat_reduce(const CsDesc* __restrict__ desc, const unsigned long long* __restrict__ counts,
                                                        const int32_t* __restrict__ luts, long long n, int n_bins,
                                                        long long* __restrict__ stats /* [.][CS_STATS], nulls filled in */,
                                                        int32_t* __restrict__ edges /* [.][n_bins + 1] or null */) {
    __shared__ long long wsum[2][4];
    __shared__ long long red_sum[2][4];
    __shared__ int red_i[3][4];
    __shared__ long long rank[CS_MAX_BINS + 1];           // rank[i] = ceil(i * m / n_bins), i = 1 .. n_bins: ascending
    const CsDesc d = desc[blockIdx.x];
    const int nc = d.n_codes;
    const unsigned long long* cnt = counts + d.cnt_off;
    const int32_t* lut = d.lut_off >= 0 ? luts + d.lut_off : nullptr;
    long long* st = stats + (long long)blockIdx.x * CS_STATS;
    int32_t* ed = edges ? edges + (long long)blockIdx.x * (n_bins + 1) : nullptr;
    const long long m = n - st[0];                        // non-NULL rows
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    if (ed) {
        for (int i = threadIdx.x; i <= n_bins; i += 256) { ed[i] = -1; rank[i] = ((long long)i * m + n_bins - 1) / n_bins; }
        __syncthreads();
    }
    const bool select = ed && m > 0;
    long long distinct = 0, len_sum = 0, carry = 0;
    int mn = 0x7FFFFFFF, mx = -1, len_max = 0;
    int buf = 0, next_edge = 1;                           // next_edge (uniform): the first edge that no earlier chunk has placed
    long long c[CS_ITEMS], c_next[CS_ITEMS];
    int l[CS_ITEMS], l_next[CS_ITEMS];
    auto load = [&](long long chunk, long long (&cc)[CS_ITEMS], int (&ll)[CS_ITEMS]) {
        const long long c0 = chunk + (long long)threadIdx.x * CS_ITEMS;
#pragma unroll
        for (int k = 0; k < CS_ITEMS; ++k) { const bool in = c0 + k < nc; cc[k] = in ? (long long)cnt[c0 + k] : 0; ll[k] = in && lut ? lut[c0 + k] : 0; }
    };
    load(0, c, l);
    for (long long chunk = 0; chunk < nc; chunk += CS_CHUNK, buf ^= 1) {
        load(chunk + CS_CHUNK, c_next, l_next);           // the next chunk's loads are in flight while this one is scanned (beyond the end: zeros, no load)
        const long long c0 = chunk + (long long)threadIdx.x * CS_ITEMS;
        long long mine = 0;
#pragma unroll
        for (int k = 0; k < CS_ITEMS; ++k) mine += c[k];
        long long incl = mine;                            // inclusive scan of `mine` over the wave, then over the block
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) { const long long o = __shfl_up(incl, s); if (lane >= s) incl += o; }
        if (lane == 63) wsum[buf][wave] = incl;
        __syncthreads();                                  // (wsum is double buffered: one barrier per chunk)
        long long before = carry + incl - mine, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const long long t = wsum[buf][w]; if (w < wave) before += t; all += t; }
        carry += all;
        // an edge lands in this chunk iff the first unplaced rank is within the rows counted so far (uniform over the block)
        const bool here = select && next_edge <= n_bins && rank[next_edge] <= carry;
        int e = next_edge;
        if (here) while (e <= n_bins && rank[e] <= before) ++e;         // placed by the codes before this lane's
#pragma unroll
        for (int k = 0; k < CS_ITEMS; ++k) {
            if (c[k] <= 0) continue;
            const int code = (int)(c0 + k);
            ++distinct; mn = min(mn, code); mx = max(mx, code);
            len_sum += c[k] * (long long)l[k]; len_max = max(len_max, l[k]);
            before += c[k];
            if (here) while (e <= n_bins && rank[e] <= before) ed[e++] = code;   // the ranks in (before - c, before]
        }
        if (here) while (next_edge <= n_bins && rank[next_edge] <= carry) ++next_edge;
#pragma unroll
        for (int k = 0; k < CS_ITEMS; ++k) { c[k] = c_next[k]; l[k] = l_next[k]; }
    }
    // block reduction of the five per-lane results
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        distinct += __shfl_xor(distinct, s); len_sum += __shfl_xor(len_sum, s);
        mn = min(mn, __shfl_xor(mn, s)); mx = max(mx, __shfl_xor(mx, s)); len_max = max(len_max, __shfl_xor(len_max, s));
    }
    if (lane == 0) { red_sum[0][wave] = distinct; red_sum[1][wave] = len_sum; red_i[0][wave] = mn; red_i[1][wave] = mx; red_i[2][wave] = len_max; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            distinct += red_sum[0][w]; len_sum += red_sum[1][w];
            mn = min(mn, red_i[0][w]); mx = max(mx, red_i[1][w]); len_max = max(len_max, red_i[2][w]);
        }
        st[1] = distinct; st[2] = mx < 0 ? -1 : mn; st[3] = mx; st[4] = len_sum; st[5] = len_max;
        if (ed && mx >= 0) ed[0] = mn;
    }
}

// dictionary indices -> codes through a per-column remap table (index < 0 or >= dict size -> NULL)
__global__ void k_encode_dict(const int32_t* __restrict__ idx, long long n, const int32_t* __restrict__ remap,
                              const long long* __restrict__ remap_off, const int32_t* __restrict__ dict_size, int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int cc = blockIdx.y;
    const int v = idx[(long long)cc * n + i];
    out[(long long)cc * n + i] = (v < 0 || v >= dict_size[cc]) ? -1 : remap[remap_off[cc] + v];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline unsigned nblocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

hipStream_t table_stream(const rgbm_table& t) {
    if (!t.stream) HIPCHK(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking));
    return t.stream;
}
// The table's twelve scratch buffers by what they hold.  A buffer's content lives from its scr / scr_upload call to the entry point's last
// synchronise (prep_mu is held all that time); inside one entry point no two uses may share a slot.  Every entry point names the slots it
// holds together in the line above its definition ("scratch slots held together": a | separates the slots the entry takes itself from those
// of the compaction or of rows_to_cells it calls).  rgbm_table_distinct_rows works on a const table whose cell list and scratch must survive:
// DevBufs of its own throughout.
enum Scr {
    SCR_BALLOTS = 0,      // compaction: the 64-row ballots of every (block, column)
    SCR_BCOUNT = 1,       // compaction: flags per (block, column)
    SCR_BOFF = 2,         // compaction: their exclusive scan, the total behind it
    SCR_TABLE_A = 3,      // the entry's first table: column descriptors / hash keys / pair-count groups / domain attributes / fd lo / k-means P
    SCR_TABLE_B = 4,      // its second: bitset words / hash state / pair-count pairs / fd hi
    SCR_ROW_MASK = 5,     // one byte per row (the flag of compact<1>) or per cell (weak labels)
    SCR_COLS = 6,         // a short list per call: columns, cell columns, is-target bytes, group columns, single_ok
    SCR_IN_ROWS = 7,      // the caller's row positions
    SCR_IN_COLS = 8,      // int32 per cell or code: the caller's columns, a LUT, top codes
    SCR_VALS = 9,         // values per cell or code, in or out: codes, counts, labels, probabilities, the fd map
    SCR_FREE_10 = 10, SCR_FREE_11 = 11      // nobody's yet
};

// scratch buffer `slot` of the table, at least `count` elements of T (grown, never shrunk)
template <typename T>
T* scr(const rgbm_table& t, Scr slot, size_t count) {
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (t.scratch[slot].n < bytes) t.scratch[slot].alloc(bytes + bytes / 4);
    return reinterpret_cast<T*>(t.scratch[slot].p);
}
template <typename T>
T* scr_upload(const rgbm_table& t, Scr slot, const T* host, size_t count, hipStream_t s) {
    T* d = scr<T>(t, slot, count);
    if (count) HIPCHK(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
}

// The ordered compaction behind every flag kernel.  The ballots and counts of nblk x ncols blocks are written: scan the counts, read the total (one
// synchronise), let dest(total, &rows, &cols) size the output (cols stays null for a row list), emit (left in flight).  Returns the total.
template <typename Dest>
long long scan_emit(const unsigned long long* ballots, const unsigned* bcount, long long* off, long long nblk, int ncols, const int32_t* d_cols,
                    hipStream_t s, Dest dest) {
    const long long m = nblk * ncols;
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, bcount, m, off, off + m);
    HIPCHK(hipGetLastError());
    long long total = 0;
    HIPCHK(hipMemcpyAsync(&total, off + m, sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    long long* rows = nullptr; int32_t* cols = nullptr;
    dest(total, &rows, &cols);
    if (total > 0) hipLaunchKernelGGL(k_emit, dim3((unsigned)nblk, (unsigned)ncols), dim3(PB), 0, s, ballots, off, cols ? d_cols : nullptr, nblk, rows, cols);
    HIPCHK(hipGetLastError());
    return total;
}

// the table's own compaction buffers (a flag kernel fills ballots and bcount) and scan_emit into its cell list: (row, column) cells when
// d_cols is given, a row list otherwise; returns the cell count
struct Ballots { unsigned long long* ballots; unsigned* bcount; long long* off; long long nblk; int ncols; };
Ballots table_ballots(const rgbm_table& t, int ncols) {
    const long long nblk = (t.n + PROWS - 1) / PROWS, m = nblk * ncols;
    return Ballots{scr<unsigned long long>(t, SCR_BALLOTS, (size_t)m * PBAL), scr<unsigned>(t, SCR_BCOUNT, (size_t)m), scr<long long>(t, SCR_BOFF, (size_t)m + 1),
                   nblk, ncols};
}
long long emit_to_table(rgbm_table& t, const Ballots& b, const int32_t* d_cols, hipStream_t s) {
    const long long total = scan_emit(b.ballots, b.bcount, b.off, b.nblk, b.ncols, d_cols, s, [&](long long tot, long long** rows, int32_t** cols) {
        const size_t need = (size_t)std::max<long long>(tot, 1);
        if (t.cell_rows.n < need) t.cell_rows.alloc(need * 5 / 4);
        if (d_cols) { if (t.cell_cols.n < need) t.cell_cols.alloc(need * 5 / 4); }
        else t.cell_cols.release();
        *rows = t.cell_rows.p; *cols = t.cell_cols.p;
    });
    HIPCHK(hipStreamSynchronize(s));
    t.n_cells = total;
    return total;
}
// MODE 0: the NULL cells of columns d_cols (want_cols: with their columns);  MODE 1: the rows of d_mask;  MODE 2: k_detect's cells
template <int MODE>
long long compact(rgbm_table& t, const uint8_t* d_mask, const int32_t* d_cols, int ncols, bool want_cols, hipStream_t s,
                  const DetDesc* d_desc = nullptr, const unsigned long long* d_bits = nullptr) {
    const Ballots b = table_ballots(t, ncols);
    if constexpr (MODE == 2)
        hipLaunchKernelGGL(k_detect, dim3((unsigned)b.nblk, (unsigned)ncols), dim3(PB), 0, s, t.codes.p, d_desc, d_bits, t.n, b.nblk, b.ballots, b.bcount);
    else
        hipLaunchKernelGGL(k_flag<MODE>, dim3((unsigned)b.nblk, (unsigned)ncols), dim3(PB), 0, s, t.codes.p, d_mask, d_cols, t.n, b.nblk, b.ballots, b.bcount);
    return emit_to_table(t, b, want_cols ? d_cols : nullptr, s);
}

// the m ascending violating rows in t.cell_rows -> rows x cell_cols (column-major): a constraint reports every given attribute of a row
void rows_to_cells(rgbm_table& t, long long m, const int32_t* cell_cols, int n_cell_cols, hipStream_t s, int64_t* n_rows_out, int64_t* n_cells_out) {
    if (n_rows_out) *n_rows_out = m;
    if (n_cell_cols > 0) {
        const size_t tot = (size_t)std::max<long long>(m * n_cell_cols, 1);
        DevBuf<long long> rows_r(tot); DevBuf<int32_t> cols_r(tot);
        const int32_t* d_cc = scr_upload<int32_t>(t, SCR_COLS, cell_cols, (size_t)n_cell_cols, s);
        if (m > 0) hipLaunchKernelGGL(k_replicate, dim3(nblocks(m, 256)), dim3(256), 0, s, t.cell_rows.p, m, d_cc, n_cell_cols, rows_r.p, cols_r.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        t.cell_rows.swap(rows_r);
        t.cell_cols.swap(cols_r);
        t.n_cells = m * n_cell_cols;
    }
    *n_cells_out = t.n_cells;
}

// an entry point with nothing to look at: the table's cell list becomes empty (row_list: as a list without columns)
int no_cells(rgbm_table& t, bool row_list, int64_t* n_rows_out, int64_t* n_cells_out) {
    t.n_cells = 0; *n_cells_out = 0;
    if (row_list) t.cell_cols.release();
    if (n_rows_out) *n_rows_out = 0;
    return RGBM_OK;
}

// the key of the columns `cols` (at most 12): radix = codes + 1 for NULL; a span of 2^63 combinations or more is refused under `entry`'s name
KeySpec key_spec(const rgbm_table& t, const int32_t* cols, int ncols, const char* entry, unsigned __int128* span_out) {
    KeySpec ks; memset(&ks, 0, sizeof(ks)); ks.ncols = ncols;
    unsigned __int128 span = 1;
    for (int i = 0; i < ncols; ++i) {
        ks.col[i] = cols[i]; ks.radix[i] = (unsigned long long)std::max<int32_t>(t.n_codes[cols[i]], 0) + 1ull;
        span *= ks.radix[i];
        if (span >= ((unsigned __int128)1 << 63)) throw std::invalid_argument(std::string(entry) + ": the EQ attributes span more than 2^63 value combinations");
    }
    *span_out = span;
    return ks;
}
// slots of an open-addressing table for n rows: a power of two, at least 1024 and twice the keys there can be (n, or `span` if smaller)
unsigned long long table_capacity(long long n, unsigned __int128 span = ~(unsigned __int128)0) {
    unsigned long long want = (unsigned long long)n * 2ull;
    if (span < (unsigned __int128)want) want = (unsigned long long)span * 2ull;
    unsigned long long cap = 1024; while (cap < want) cap <<= 1;
    return cap;
}
// appends the first nbits bits of `src` to `words` as whole 64-bit words, the bits beyond them cleared; returns the offset, *n_words the count
long long append_bitset(std::vector<unsigned long long>& words, const uint64_t* src, long long nbits, int32_t* n_words) {
    const long long off = (long long)words.size(), nw = (nbits + 63) / 64;
    words.insert(words.end(), src, src + nw);
    if (nbits % 64) words.back() &= (1ull << (nbits % 64)) - 1ull;
    *n_words = (int32_t)nw;
    return off;
}
void check_cols(const rgbm_table& t, const int32_t* cols, int n, const char* what) {
    for (int i = 0; i < n; ++i) if (cols[i] < 0 || cols[i] >= t.c) throw std::invalid_argument(std::string(what) + ": column index out of range");
}
// the RGBM_ERR_ARG refusals of the detectors' column lists (check_cols throws, which gives RGBM_ERR_PARAM): every column inside the table;
// `once`: none listed twice; `bitsets`: each with one.  RGBM_OK or the refusal.
int refuse_cols(const rgbm_table& t, const int32_t* cols, int n, bool once, const uint64_t* const* bitsets, const char* entry) {
    std::vector<uint8_t> seen(once ? (size_t)t.c : 0, 0);
    for (int i = 0; i < n; ++i) {
        if (cols[i] < 0 || cols[i] >= t.c) return fail(RGBM_ERR_ARG, std::string(entry) + ": column index out of range");
        if (once && seen[cols[i]]) return fail(RGBM_ERR_ARG, std::string(entry) + ": a column is listed twice");
        if (bitsets && !bitsets[i]) return fail(RGBM_ERR_ARG, std::string(entry) + ": a column without a bitset");
        if (once) seen[cols[i]] = 1;
    }
    return RGBM_OK;
}

// string pool offsets: start at 0, never decrease (every read of the distance kernels stays inside [0, off[n]))
void check_pool_offsets(const int64_t* off, int64_t n, const int32_t* cp, const char* entry, const char* which) {
    if (n == 0) return;
    if (off[0] != 0) throw std::invalid_argument(std::string(entry) + ": " + which + "_off[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) throw std::invalid_argument(std::string(entry) + ": " + which + "_off must not decrease");
    if (off[n] > 0 && !cp) throw std::invalid_argument(std::string(entry) + ": " + which + "_cp missing");
}

// Levenshtein matrix [n_a][n_b] of two checked, non-empty string pools (host memory) into `d_dist` (device memory); the pools and
// the scratch of the long pairs live until the kernels are done (the stream is synchronised before returning).
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
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); struct { hipStream_t s; } sg{table_stream(*t)};
        const int32_t* d_tc = scr_upload<int32_t>(*t, SCR_COLS, &target_col, 1, sg.s);
        const long long cells = compact<0>(*t, nullptr, d_tc, 1, false, sg.s);      // ascending rows whose target cell is NULL
        *n_cells_out = cells;
        if (cells == 0) return RGBM_OK;
        if (cells > cap) throw std::invalid_argument(std::string(entry) + ": output capacity too small (n_cells_out holds the needed size)");
        if (!rows_out || !class_out || !prob_out) throw std::invalid_argument(std::string(entry) + ": output arrays missing");
        if (cost_row)
            for (long long i = 0; i < cells; ++i)
                if (cost_row[i] < -1 || cost_row[i] >= n_cost_rows) throw std::invalid_argument(std::string(entry) + ": cost_row out of range");
        // the cells' rows as a small code block, scored in one go
        DevBuf<int32_t> sub((size_t)cells * t->c);
        hipLaunchKernelGGL(k_gather_rows, dim3(nblocks(cells, 256), (unsigned)t->c), dim3(256), 0, sg.s, t->codes.p, (long long)t->n, sub.p, cells, t->cell_rows.p);
        DevBuf<int32_t> d_fc((size_t)f); d_fc.upload(feat_cols, (size_t)f, sg.s);
        DevBuf<double> proba((size_t)cells * K);
        predict_proba_device(m, t->device, sg.s, sub.p, cells, d_fc.p, proba.p);
        DevBuf<int32_t> d_cls((size_t)cells * top_k); DevBuf<double> d_pr((size_t)cells * top_k);
        DevBuf<int32_t> d_cur, d_row; DevBuf<double> d_cp, d_cost, d_tc1;
        if (cur_prob_out) { d_cp.alloc((size_t)cells); if (cur_code) { d_cur.alloc((size_t)cells); d_cur.upload(cur_code, (size_t)cells, sg.s); } }
        if (cost) { d_cost.alloc((size_t)(n_cost_rows + 1) * K); d_cost.upload(cost, (size_t)(n_cost_rows + 1) * K, sg.s); }
        if (cost_row) { d_row.alloc((size_t)cells); d_row.upload(cost_row, (size_t)cells, sg.s); }
        if (top1_cost_out) d_tc1.alloc((size_t)cells);
        hipLaunchKernelGGL(k_weighted_pmf, dim3(nblocks(cells, 4)), dim3(256), 0, sg.s, proba.p, cells, (int)K, (int)top_k, threshold,
                           d_cur.p, d_row.p, d_cost.p, (long long)n_cost_rows, weight, renormalise ? 1 : 0, d_cls.p, d_pr.p, d_cp.p, d_tc1.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rows_out, t->cell_rows.p, (size_t)cells * 8, hipMemcpyDeviceToHost, sg.s));
        d_cls.download(class_out, (size_t)cells * top_k, sg.s);
        d_pr.download(prob_out, (size_t)cells * top_k, sg.s);
        if (cur_prob_out) d_cp.download(cur_prob_out, (size_t)cells, sg.s);
        if (top1_cost_out) d_tc1.download(top1_cost_out, (size_t)cells, sg.s);
        HIPCHK(hipStreamSynchronize(sg.s));
        return RGBM_OK;
    });
}

}  // namespace

extern "C" {

// scratch slots held together: COLS | BALLOTS BCOUNT BOFF
RGBM_EXPORT int rgbm_table_detect_nulls(rgbm_table* t, const int32_t* cols, int32_t n_cols, int64_t* n_cells_out) {
    if (!t || !n_cells_out || n_cols < 0 || (n_cols > 0 && !cols)) return fail(RGBM_ERR_ARG, "rgbm_table_detect_nulls: bad argument");
    return guarded([&]() {
        use_device(t->device);
        check_cols(*t, cols, n_cols, "rgbm_table_detect_nulls");
        if (n_cols == 0) return no_cells(*t, false, nullptr, n_cells_out);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const int32_t* d_cols = scr_upload<int32_t>(*t, SCR_COLS, cols, (size_t)n_cols, s);
        *n_cells_out = compact<0>(*t, nullptr, d_cols, n_cols, true, s);
        return RGBM_OK;
    });
}

// scratch slots held together: COLS TABLE_A (descriptors) TABLE_B (bitsets) | BALLOTS BCOUNT BOFF
RGBM_EXPORT int rgbm_table_detect_cells(rgbm_table* t, const int32_t* cols, int32_t n_cols, const uint8_t* null_is_error,
                                        const int32_t* keep_lo, const int32_t* keep_hi, const uint64_t* const* flag_bits, int64_t* n_cells_out) {
    if (!t || !n_cells_out || n_cols < 0 || (n_cols > 0 && (!cols || !null_is_error || !keep_lo || !keep_hi)))
        return fail(RGBM_ERR_ARG, "rgbm_table_detect_cells: bad argument");
    if (const int rc = refuse_cols(*t, cols, n_cols, true, nullptr, "rgbm_table_detect_cells")) return rc;
    return guarded([&]() {
        use_device(t->device);
        if (n_cols == 0 || t->n == 0) return no_cells(*t, false, nullptr, n_cells_out);
        // one descriptor per column; the bitsets one after the other, bits at and beyond n_codes cleared
        std::vector<DetDesc> desc((size_t)n_cols);
        std::vector<unsigned long long> bits;
        for (int i = 0; i < n_cols; ++i) {
            DetDesc& d = desc[i];
            d.col = cols[i]; d.null_is_error = null_is_error[i] ? 1 : 0; d.keep_lo = keep_lo[i]; d.keep_hi = keep_hi[i];
            d.bit_off = -1; d.n_words = 0; d.pad = 0;
            const uint64_t* fb = flag_bits ? flag_bits[i] : nullptr;
            if (!fb) continue;
            d.bit_off = append_bitset(bits, fb, std::max<long long>(t->n_codes[cols[i]], 0), &d.n_words);
        }
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const int32_t* d_cols = scr_upload<int32_t>(*t, SCR_COLS, cols, (size_t)n_cols, s);
        const DetDesc* d_desc = scr_upload<DetDesc>(*t, SCR_TABLE_A, desc.data(), desc.size(), s);
        const unsigned long long* d_bits = scr_upload<unsigned long long>(*t, SCR_TABLE_B, bits.data(), bits.size(), s);
        *n_cells_out = compact<2>(*t, nullptr, d_cols, n_cols, true, s, d_desc, d_bits);
        return RGBM_OK;
    });
}

// scratch slots held together: TABLE_A (keys) TABLE_B (state) ROW_MASK | BALLOTS BCOUNT BOFF | COLS (the cell columns, rows_to_cells)
RGBM_EXPORT int rgbm_table_detect_constraint(rgbm_table* t, const int32_t* eq_cols, int32_t n_eq, int32_t iq_col,
                                             const int32_t* cell_cols, int32_t n_cell_cols, int64_t* n_rows_out, int64_t* n_cells_out) {
    if (!t || n_eq < 0 || n_eq > 12 || (n_eq > 0 && !eq_cols) || n_cell_cols < 0 || (n_cell_cols > 0 && !cell_cols) || !n_cells_out)
        return fail(RGBM_ERR_ARG, "rgbm_table_detect_constraint: bad argument (at most 12 EQ attributes)");
    return guarded([&]() {
        use_device(t->device);
        check_cols(*t, eq_cols, n_eq, "rgbm_table_detect_constraint");
        check_cols(*t, cell_cols, n_cell_cols, "rgbm_table_detect_constraint");
        if (iq_col < 0 || iq_col >= t->c) throw std::invalid_argument("rgbm_table_detect_constraint: IQ column out of range");
        unsigned __int128 span = 1;
        const KeySpec ks = key_spec(*t, eq_cols, n_eq, "rgbm_table_detect_constraint", &span);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const long long n = t->n;
        const unsigned long long cap = table_capacity(n, span);
        unsigned long long* keys = scr<unsigned long long>(*t, SCR_TABLE_A, (size_t)cap);
        unsigned* state = scr<unsigned>(*t, SCR_TABLE_B, (size_t)cap);
        uint8_t* mask = scr<uint8_t>(*t, SCR_ROW_MASK, (size_t)n);
        HIPCHK(hipMemsetAsync(keys, 0xFF, (size_t)cap * 8, s));
        HIPCHK(hipMemsetAsync(state, 0, (size_t)cap * 4, s));
        const unsigned nb = nblocks(n, 256);
        hipLaunchKernelGGL(k_ht_insert, dim3(nb), dim3(256), 0, s, t->codes.p, n, ks, iq_col, keys, state, cap - 1);
        hipLaunchKernelGGL(k_ht_lookup, dim3(nb), dim3(256), 0, s, t->codes.p, n, ks, keys, state, cap - 1, mask);
        const long long m = compact<1>(*t, mask, nullptr, 1, false, s);     // ascending violating rows
        rows_to_cells(*t, m, cell_cols, n_cell_cols, s, n_rows_out, n_cells_out);
        return RGBM_OK;
    });
}

// scratch slots held together: ROW_MASK IN_ROWS | BALLOTS BCOUNT BOFF
RGBM_EXPORT int rgbm_table_rows_of_cells(rgbm_table* t, const int64_t* rows, int64_t n_cells, int64_t* n_rows_out) {
    if (!t || !n_rows_out || n_cells < 0 || (n_cells > 0 && !rows)) return fail(RGBM_ERR_ARG, "rgbm_table_rows_of_cells: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        uint8_t* mask = scr<uint8_t>(*t, SCR_ROW_MASK, (size_t)t->n);
        HIPCHK(hipMemsetAsync(mask, 0, (size_t)t->n, s));
        static_assert(sizeof(long long) == sizeof(int64_t), "row positions are 64-bit");
        const long long* d_rows = scr_upload<long long>(*t, SCR_IN_ROWS, reinterpret_cast<const long long*>(rows), (size_t)n_cells, s);
        if (n_cells > 0) hipLaunchKernelGGL(k_mark_rows, dim3(nblocks(n_cells, 256)), dim3(256), 0, s, mask, (long long)t->n, d_rows, (long long)n_cells);
        *n_rows_out = compact<1>(*t, mask, nullptr, 1, false, s);
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_cells_fetch(const rgbm_table* t, int64_t* rows_out, int32_t* cols_out) {
    if (!t) return fail(RGBM_ERR_ARG, "rgbm_table_cells_fetch: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        if (t->n_cells > 0) {
            if (rows_out) HIPCHK(hipMemcpy(rows_out, t->cell_rows.p, (size_t)t->n_cells * 8, hipMemcpyDeviceToHost));
            if (cols_out) {
                if (!t->cell_cols.p) throw std::invalid_argument("rgbm_table_cells_fetch: the last result is a row list (no columns)");
                HIPCHK(hipMemcpy(cols_out, t->cell_cols.p, (size_t)t->n_cells * 4, hipMemcpyDeviceToHost));
            }
        }
        return RGBM_OK;
    });
}

// scratch slots held together: COLS (is-target bytes) IN_ROWS IN_COLS
RGBM_EXPORT int rgbm_table_null_cells(rgbm_table* t, const int64_t* rows, const int32_t* cols, int64_t n_cells,
                                      const int32_t* target_cols, int32_t n_targets) {
    if (!t || n_cells < 0 || (n_cells > 0 && (!rows || !cols)) || n_targets < 0 || (n_targets > 0 && !target_cols))
        return fail(RGBM_ERR_ARG, "rgbm_table_null_cells: bad argument");
    return guarded([&]() {
        use_device(t->device);
        rgh::ViewWrite view_wr(t);
        check_cols(*t, target_cols, n_targets, "rgbm_table_null_cells");
        if (n_cells == 0 || n_targets == 0) return RGBM_OK;
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        std::vector<uint8_t> is_t((size_t)t->c, 0);
        for (int i = 0; i < n_targets; ++i) is_t[target_cols[i]] = 1;
        const uint8_t* d_t = scr_upload<uint8_t>(*t, SCR_COLS, is_t.data(), is_t.size(), s);
        const long long* d_rows = scr_upload<long long>(*t, SCR_IN_ROWS, reinterpret_cast<const long long*>(rows), (size_t)n_cells, s);
        const int32_t* d_cols = scr_upload<int32_t>(*t, SCR_IN_COLS, cols, (size_t)n_cells, s);
        hipLaunchKernelGGL(k_null_cells, dim3(nblocks(n_cells, 256)), dim3(256), 0, s, t->codes.p, (long long)t->n, (int)t->c, d_rows, d_cols,
                           (long long)n_cells, d_t);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));      // is_t and the caller's arrays are read by the async copies
        return RGBM_OK;
    });
}

// scratch slots held together: IN_ROWS IN_COLS VALS
RGBM_EXPORT int rgbm_table_write_cells(rgbm_table* t, const int64_t* rows, const int32_t* cols, const int32_t* codes, int64_t n_cells) {
    if (!t || n_cells < 0 || (n_cells > 0 && (!rows || !cols || !codes))) return fail(RGBM_ERR_ARG, "rgbm_table_write_cells: bad argument");
    return guarded([&]() {
        use_device(t->device);
        rgh::ViewWrite view_wr(t);
        if (n_cells == 0) return RGBM_OK;
        for (int64_t i = 0; i < n_cells; ++i)
            if (cols[i] >= 0 && cols[i] < t->c && codes[i] >= t->n_codes[cols[i]]) throw std::invalid_argument("rgbm_table_write_cells: code outside the column's dictionary");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const long long* d_rows = scr_upload<long long>(*t, SCR_IN_ROWS, reinterpret_cast<const long long*>(rows), (size_t)n_cells, s);
        const int32_t* d_cols = scr_upload<int32_t>(*t, SCR_IN_COLS, cols, (size_t)n_cells, s);
        const int32_t* d_vals = scr_upload<int32_t>(*t, SCR_VALS, codes, (size_t)n_cells, s);
        hipLaunchKernelGGL(k_write_cells, dim3(nblocks(n_cells, 256)), dim3(256), 0, s, t->codes.p, (long long)t->n, (int)t->c, d_rows, d_cols, d_vals, (long long)n_cells);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

// scratch slots held together: IN_ROWS IN_COLS VALS
RGBM_EXPORT int rgbm_table_read_cells(const rgbm_table* t, const int64_t* rows, const int32_t* cols, int64_t n_cells, int32_t* codes_out) {
    if (!t || n_cells < 0 || (n_cells > 0 && (!rows || !cols || !codes_out))) return fail(RGBM_ERR_ARG, "rgbm_table_read_cells: bad argument");
    return guarded([&]() {
        use_device(t->device);
        if (n_cells == 0) return RGBM_OK;
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const long long* d_rows = scr_upload<long long>(*t, SCR_IN_ROWS, reinterpret_cast<const long long*>(rows), (size_t)n_cells, s);
        const int32_t* d_cols = scr_upload<int32_t>(*t, SCR_IN_COLS, cols, (size_t)n_cells, s);
        int32_t* d_out = scr<int32_t>(*t, SCR_VALS, (size_t)n_cells);
        hipLaunchKernelGGL(k_read_cells, dim3(nblocks(n_cells, 256)), dim3(256), 0, s, t->codes.p, (long long)t->n, (int)t->c, d_rows, d_cols,
                           (long long)n_cells, d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(codes_out, d_out, (size_t)n_cells * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

// scratch slots held together: IN_ROWS
RGBM_EXPORT int rgbm_table_gather_rows(const rgbm_table* t, const int64_t* rows, int64_t n_rows, rgbm_table** out) {
    if (!t || !out || n_rows <= 0 || !rows) return fail(RGBM_ERR_ARG, "rgbm_table_gather_rows: bad argument (at least one row)");
    return guarded([&]() {
        use_device(t->device);
        for (int64_t i = 0; i < n_rows; ++i) if (rows[i] < 0 || rows[i] >= t->n) throw std::invalid_argument("rgbm_table_gather_rows: row position out of range");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        std::unique_ptr<rgbm_table> o(new rgbm_table());
        o->device = t->device; o->n = n_rows; o->c = t->c; o->n_codes = t->n_codes; o->col_values = t->col_values; o->col_kind = t->col_kind;
        o->codes.alloc((size_t)n_rows * t->c);
        const long long* d_rows = scr_upload<long long>(*t, SCR_IN_ROWS, reinterpret_cast<const long long*>(rows), (size_t)n_rows, s);
        hipLaunchKernelGGL(k_gather_rows, dim3(nblocks(n_rows, 256), (unsigned)t->c), dim3(256), 0, s, t->codes.p, (long long)t->n, o->codes.p,
                           (long long)n_rows, d_rows);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        *out = o.release();
        return RGBM_OK;
    });
}

// scratch slots held together: VALS
RGBM_EXPORT int rgbm_table_count_codes(const rgbm_table* t, int32_t col, int64_t* counts_out, int64_t* n_null_out) {
    if (!t || !counts_out || col < 0 || col >= t->c) return fail(RGBM_ERR_ARG, "rgbm_table_count_codes: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const int nc = t->n_codes[col];
        unsigned long long* d_cnt = scr<unsigned long long>(*t, SCR_VALS, (size_t)nc + 1);
        HIPCHK(hipMemsetAsync(d_cnt, 0, ((size_t)nc + 1) * 8, s));
        const unsigned nb = std::min<unsigned>(nblocks(t->n, 256 * 16), 256u * 8u);
        hipLaunchKernelGGL(k_count_codes, dim3(std::max(nb, 1u)), dim3(256), 0, s, t->codes.p + (size_t)col * t->n, (long long)t->n, nc, d_cnt);
        HIPCHK(hipGetLastError());
        std::vector<unsigned long long> h((size_t)nc + 1);
        HIPCHK(hipMemcpyAsync(h.data(), d_cnt, h.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < nc; ++i) counts_out[i] = (int64_t)h[i];
        if (n_null_out) *n_null_out = (int64_t)h[nc];
        return RGBM_OK;
    });
}

// scratch slots held together: TABLE_A (column descriptors) TABLE_B (the six numbers per column) COLS (edges) IN_COLS (length LUTs) VALS (counts)
RGBM_EXPORT int rgbm_table_column_stats(const rgbm_table* t, const int32_t* cols, int32_t n_cols, const int32_t* const* len_lut, int32_t n_bins,
                                        int64_t* stats_out, int32_t* edges_out) {
    if (!t || !cols || !stats_out || n_cols < 1) return fail(RGBM_ERR_ARG, "rgbm_table_column_stats: bad argument (at least one column)");
    if (n_bins < 0 || n_bins > CS_MAX_BINS) return fail(RGBM_ERR_PARAM, "rgbm_table_column_stats: n_bins must be 0 or 1..254");
    if (n_bins > 0 && !edges_out) return fail(RGBM_ERR_ARG, "rgbm_table_column_stats: edges_out is NULL with n_bins > 0");
    if (n_cols > 65535) return fail(RGBM_ERR_PARAM, "rgbm_table_column_stats: more than 65535 listed columns");
    if (const int rc = refuse_cols(*t, cols, n_cols, false, nullptr, "rgbm_table_column_stats")) return rc;
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        std::vector<CsDesc> desc((size_t)n_cols);
        long long n_cnt = 0, n_lut = 0;
        for (int j = 0; j < n_cols; ++j) {
            const int nc = t->n_codes[cols[j]];
            const bool has_lut = len_lut && len_lut[j];
            desc[j] = CsDesc{n_cnt, has_lut ? n_lut : -1, cols[j], nc};
            n_cnt += nc; if (has_lut) n_lut += nc;
        }
        const CsDesc* d_desc = scr_upload<CsDesc>(*t, SCR_TABLE_A, desc.data(), desc.size(), s);
        int32_t* d_luts = scr<int32_t>(*t, SCR_IN_COLS, (size_t)n_lut);           // every LUT goes from the caller's array to its place
        for (int j = 0; j < n_cols; ++j)
            if (desc[j].lut_off >= 0) HIPCHK(hipMemcpyAsync(d_luts + desc[j].lut_off, len_lut[j], (size_t)desc[j].n_codes * 4, hipMemcpyHostToDevice, s));
        unsigned long long* d_cnt = scr<unsigned long long>(*t, SCR_VALS, (size_t)n_cnt);
        long long* d_stats = scr<long long>(*t, SCR_TABLE_B, (size_t)n_cols * CS_STATS);
        int32_t* d_edges = n_bins > 0 ? scr<int32_t>(*t, SCR_COLS, (size_t)n_cols * (n_bins + 1)) : nullptr;
        HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)n_cnt * 8, s));
        HIPCHK(hipMemsetAsync(d_stats, 0, (size_t)n_cols * CS_STATS * 8, s));
        const unsigned nb = std::max(std::min<unsigned>(nblocks(t->n, 256 * CS_UNROLL * 4), 256u * 8u), 1u);
        hipLaunchKernelGGL(k_colstat_count, dim3(nb, (unsigned)n_cols), dim3(256), 0, s, t->codes.p, (long long)t->n, d_desc, d_cnt,
                           reinterpret_cast<unsigned long long*>(d_stats));
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_colstat_reduce, dim3((unsigned)n_cols), dim3(256), 0, s, d_desc, d_cnt, d_luts, (long long)t->n, (int)n_bins, d_stats, d_edges);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(stats_out, d_stats, (size_t)n_cols * CS_STATS * 8, hipMemcpyDeviceToHost, s));
        if (d_edges) HIPCHK(hipMemcpyAsync(edges_out, d_edges, (size_t)n_cols * (n_bins + 1) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_create_dict(const int32_t* idx_colmajor, int64_t n, int32_t c, const int32_t* const* remap,
                                       const int32_t* dict_size, int32_t device_id, rgbm_table** out) {
    if (!idx_colmajor || !remap || !dict_size || !out || n <= 0 || c <= 0) return fail(RGBM_ERR_ARG, "rgbm_table_create_dict: bad argument");
    return guarded([&]() {
        use_device(device_id);
        StreamGuard sg;
        std::vector<long long> roff((size_t)c); std::vector<int32_t> flat; std::vector<int32_t> ncodes((size_t)c);
        for (int j = 0; j < c; ++j) {
            if (dict_size[j] < 0 || (dict_size[j] > 0 && !remap[j])) throw std::invalid_argument("rgbm_table_create_dict: bad dictionary");
            roff[j] = (long long)flat.size();
            int mx = -1;
            for (int v = 0; v < dict_size[j]; ++v) {
                const int r = remap[j][v];
                if (r < -1) throw std::invalid_argument("rgbm_table_create_dict: remap entries must be codes >= 0 or -1 (NULL)");
                flat.push_back(r); mx = std::max(mx, r);
            }
            ncodes[j] = std::max(mx + 1, 1);      // an all-NULL column still counts as a one-code domain (repair.encode does the same)
        }
        std::unique_ptr<rgbm_table> t(new rgbm_table());
        t->device = device_id; t->n = n; t->c = c; t->n_codes = ncodes;
        t->codes.alloc((size_t)n * c);
        DevBuf<int32_t> d_idx((size_t)n * c); HIPCHK(hipMemcpyAsync(d_idx.p, idx_colmajor, (size_t)n * c * 4, hipMemcpyHostToDevice, sg.s));
        DevBuf<int32_t> d_flat(std::max<size_t>(flat.size(), 1)); d_flat.upload(flat.data(), flat.size(), sg.s);
        DevBuf<long long> d_off((size_t)c); d_off.upload(roff.data(), roff.size(), sg.s);
        DevBuf<int32_t> d_ds((size_t)c); d_ds.upload(dict_size, (size_t)c, sg.s);
        hipLaunchKernelGGL(k_encode_dict, dim3(nblocks(n, 256), (unsigned)c), dim3(256), 0, sg.s, d_idx.p, (long long)n, d_flat.p, d_off.p, d_ds.p, t->codes.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(sg.s));
        *out = t.release();
        return RGBM_OK;
    });
}

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

RGBM_EXPORT int rgbm_table_shape(const rgbm_table* t, int64_t* n_out, int32_t* c_out, int32_t* n_codes_out) {
    if (!t) return fail(RGBM_ERR_ARG, "rgbm_table_shape: bad argument");
    if (n_out) *n_out = t->n;
    if (c_out) *c_out = t->c;
    if (n_codes_out) for (int j = 0; j < t->c; ++j) n_codes_out[j] = t->n_codes[j];
    return RGBM_OK;
}

}  // extern "C"

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
namespace {

constexpr int PC_B = 512;                                   // threads per workgroup
constexpr int PC_MAXC = 16;                                 // distinct columns a group stages per row tile
constexpr int PC_TILE_BYTES = PC_MAXC * PC_B * 2;           // uint16 bins [PC_MAXC][PC_B]
constexpr int PC_LDS_CELLS = (160 * 1024 - 2048 - PC_TILE_BYTES) / 4;      // 32-bit counters of one group
constexpr long long PC_ROWS_PER_WG_MAX = 1ll << 30;
constexpr long long PC_MAX_CELLS_PAIR = 1ll << 24, PC_MAX_CELLS = 1ll << 25;   // dense cells of one pair / of a call
constexpr int DOM_MAXK = 8;                                 // correlated attributes of one cell-domain call

struct PcPair { int32_t sx, sy, dy1; uint32_t lds_off, cells; long long out_off; };
struct PcGroup { int32_t col_begin, ncols, pair_begin, npairs; uint32_t cells; };
struct DomAttr { long long off, sn, sv, min_cnt; int32_t col, d_c; };

// bin of (row r, column col): the code through the column's LUT (if any); NULL / out of range -> slot d = nbins
__device__ __forceinline__ int pc_bin(const int32_t* __restrict__ codes, long long n, int col, long long r, const int32_t* __restrict__ colinfo,
                                      const long long* __restrict__ lut_off, const int32_t* __restrict__ luts) {
    int v = codes[(long long)col * n + r];
    const int nc = colinfo[2 * col], d = colinfo[2 * col + 1];
    if (v < 0 || v >= nc) return d;
    const long long lo = lut_off[col];
    if (lo >= 0) v = luts[lo + v];
    return (v < 0 || v >= d) ? d : v;
}

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
    const long long r = rows[i];
    const bool inside = r >= 0 && r < n;
    const unsigned long long* base[DOM_MAXK]; long long sn[DOM_MAXK], mc[DOM_MAXK];
    // the fold  IF(ISNOTNULL(domain), CONCAT(domain, d), d):  an attribute whose element list is NULL (value NULL / no group above the
    // threshold) wipes what came before it, so only the attributes after the last such one contribute
    int j0 = k;
    if (inside) {
        j0 = 0;
#pragma unroll
        for (int j = 0; j < DOM_MAXK; ++j) {
            if (j >= k) break;
            const DomAttr a = attrs[j];
            const int v = pc_bin(codes, n, a.col, r, colinfo, lut_off, luts);
            base[j] = joint + a.off + (long long)(v < a.d_c ? v : 0) * a.sv; sn[j] = a.sn; mc[j] = a.min_cnt;
            bool has = false;
            if (v < a.d_c) for (int c = 0; c < d_a; ++c) if ((long long)base[j][(long long)c * a.sn] > a.min_cnt) { has = true; break; }
            if (!has) j0 = j + 1;
        }
    }
    auto score = [&](int c) -> double {
        double s = 0.0;
        if (!single_ok[c]) return s;
#pragma unroll
        for (int j = 0; j < DOM_MAXK; ++j) {
            if (j >= k) break;
            if (j < j0) continue;
            const long long cnt = (long long)base[j][(long long)c * sn[j]];
            if (cnt > mc[j]) { const double b = fmax((double)cnt - 1.0, 0.1); s = s + b / row_count; }
        }
        return s;
    };
    double den = 0.0;
    if (j0 < k) for (int c = 0; c < d_a; ++c) den = den + score(c);          // ascending code, sequential
    double best = 0.0; int bt = -1;
    for (int c = 0; c < d_a; ++c) {
        const double p = (j0 < k && den > 0.0) ? score(c) / den : 0.0;
        if (probs) probs[i * d_a + c] = p;
        if (p > best) { best = p; bt = c; }                                   // first maximum: ties by ascending code
    }
    const bool valid = bt >= 0 && best > beta;
    int cur = inside ? codes[(long long)target * n + r] : -1;
    if (cur >= d_a) cur = -1;
    weak[i] = (uint8_t)(valid && cur >= 0 && cur == bt);
    top[i] = valid ? bt : -1;
    top_prob[i] = valid ? best : 0.0;
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
        return RGBM_OK;
    });
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
        std::vector<DomAttr> attrs((size_t)std::max(k, 1));
        for (int j = 0; j < k; ++j) {
            const int p = pair_idx[j];
            if (p < 0 || p >= (int)t->pc_x.size()) throw std::invalid_argument("rgbm_table_cell_domains: pair index out of range");
            DomAttr a;
            a.off = t->pc_off[p]; a.min_cnt = std::max<long long>(min_cnt[j], 0);
            if (t->pc_x[p] == target_col) { a.col = t->pc_y[p]; a.d_c = t->pc_dy[p]; a.sn = (long long)t->pc_dy[p] + 1; a.sv = 1; }
            else if (t->pc_y[p] == target_col) { a.col = t->pc_x[p]; a.d_c = t->pc_dx[p]; a.sn = 1; a.sv = (long long)t->pc_dy[p] + 1; }
            else throw std::invalid_argument("rgbm_table_cell_domains: a pair does not hold the target column");
            attrs[j] = a;
        }
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

// =============================================================================================
// Rule-based repairs (python/repair/model.py `_build_rule_model`, `FunctionalDepModel.predict`, `PoorModel.predict`,
// `_repair_by_nearest_values`; reference model.py:44-100, 928-953, 1279-1291).
//
//   fd_map          for every code of x the single y code it occurs with over the rows where both cells are non-NULL, else -1.  Per x a
//                   (lo, hi) pair of y codes kept with integer atomicMin / atomicMax: unique iff lo == hi.  Min and max do not depend on
//                   the order of the rows, so the map is a function of the table, whatever the launch geometry.  A workgroup keeps the
//                   pairs of its row range in LDS (FD_LDS_CODES codes: 2 x 4 B each, 64 KiB, two workgroups a CU) and flushes the codes it
//                   saw with global vector atomics; more codes than that update the HBM tables directly.  A lane reads lo[x] / hi[x] first and
//                   issues the atomic only when y falls outside: lo only falls and hi only rises, so a stale read costs an atomic, never
//                   a wrong skip, and after the first rows of a low-cardinality x the loop is LDS reads (same address: broadcast).
//                   Algorithmic bytes: 8 B per row (two int32 columns), no staging: consecutive lanes load consecutive rows.
//   rule_fill       pred = lut[x] (or the constant lut[0]); NULL y cells receive pred >= 0; out_label = pred for every row.
//   row_nearest     one wave per row of a cost matrix: the minimum over the entries that are not NaN, whether it occurs once, and
//                   where; the position when the minimum is unique and <= threshold, else -1.
// =============================================================================================
namespace {

constexpr int FD_B = 512;                                   // threads per workgroup
constexpr int FD_UNROLL = 4;                                // rows a lane loads before it updates
constexpr int FD_LDS_CODES = 8192;                          // x codes whose (lo, hi) pairs a workgroup keeps in LDS
constexpr long long NV_MAX_CELLS = 1ll << 30;               // entries of one nearest-value cost matrix

__global__ void k_fd_init(int* __restrict__ lo, int* __restrict__ hi, int nx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nx) { lo[i] = 0x7FFFFFFF; hi[i] = -1; }
}

template <bool LDS>
__global__ __launch_bounds__(FD_B) void k_fd_map(const int32_t* __restrict__ x, const int32_t* __restrict__ y, long long n, int nx, int ny,
                                                 long long rows_per_wg, int* glo, int* ghi) {
    extern __shared__ int fd_smem[];                        // LDS: lo [nx], hi [nx]
    int* lo = LDS ? fd_smem : glo;
    int* hi = LDS ? fd_smem + nx : ghi;
    const int tid = threadIdx.x;
    if (LDS) {
        for (int i = tid; i < nx; i += FD_B) { lo[i] = 0x7FFFFFFF; hi[i] = -1; }
        __syncthreads();
    }
    const long long begin = (long long)blockIdx.x * rows_per_wg;
    const long long end = begin + rows_per_wg < n ? begin + rows_per_wg : n;
    for (long long base = begin; base < end; base += FD_B * FD_UNROLL) {
        int xs[FD_UNROLL], ys[FD_UNROLL];
#pragma unroll
        for (int k = 0; k < FD_UNROLL; ++k) {
            const long long r = base + (long long)k * FD_B + tid;
            xs[k] = r < end ? x[r] : -1;
            ys[k] = r < end ? y[r] : -1;
        }
#pragma unroll
        for (int k = 0; k < FD_UNROLL; ++k) {
            const int xv = xs[k], yv = ys[k];
            if (xv < 0 || xv >= nx || yv < 0 || yv >= ny) continue;        // a NULL side: the row does not take part
            if (yv < lo[xv]) atomicMin(&lo[xv], yv);
            if (yv > hi[xv]) atomicMax(&hi[xv], yv);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = tid; i < nx; i += FD_B)
            if (hi[i] >= 0) { atomicMin(&glo[i], lo[i]); atomicMax(&ghi[i], hi[i]); }
    }
}

__global__ void k_fd_finish(const int* __restrict__ lo, const int* __restrict__ hi, int nx, int32_t* __restrict__ map) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nx) map[i] = lo[i] == hi[i] ? lo[i] : -1;                      // never seen: lo = INT_MAX, hi = -1
}

__global__ void k_rule_fill(int32_t* __restrict__ codes, long long n, int y_col, int x_col, const int32_t* __restrict__ lut, int n_lut,
                            long long row_begin, long long n_rows, int32_t* __restrict__ out_label) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const long long r = row_begin + i;
    int pred;
    if (x_col < 0) pred = lut[0];
    else { const int xv = codes[(long long)x_col * n + r]; pred = (xv >= 0 && xv < n_lut) ? lut[xv] : -1; }
    if (out_label) out_label[i] = pred;
    int32_t* cell = codes + (long long)y_col * n + r;
    if (pred >= 0 && *cell < 0) *cell = pred;
}

template <typename T>
__global__ __launch_bounds__(256) void k_row_nearest(const T* __restrict__ mat, long long n_a, int n_b, double threshold,
                                                     int32_t* __restrict__ out) {
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n_a) return;
    const int lane = (int)(threadIdx.x & 63u);
    const T* m = mat + row * n_b;
    double bm = 0.0; int cnt = 0, bp = 0x7FFFFFFF;           // the least value, how often it occurs (2 = more than once), its first position
    for (int c = lane; c < n_b; c += 64) {
        const double v = (double)m[c];
        if (isnan(v)) continue;                              // NaN = None: the pair has no cost
        if (cnt == 0 || v < bm) { bm = v; cnt = 1; bp = c; }
        else if (v == bm) cnt = 2;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double om = __shfl_xor(bm, d); const int oc = __shfl_xor(cnt, d); const int op = __shfl_xor(bp, d);
        if (oc > 0) {
            if (cnt == 0 || om < bm) { bm = om; cnt = oc; bp = op; }
            else if (om == bm) { cnt = 2; bp = op < bp ? op : bp; }
        }
    }
    if (lane == 0) out[row] = (cnt == 1 && bm <= threshold) ? bp : -1;
}

}  // namespace

extern "C" {

// scratch slots held together: TABLE_A (lo) TABLE_B (hi) VALS (map)
RGBM_EXPORT int rgbm_table_fd_map(const rgbm_table* t, int32_t x_col, int32_t y_col, int32_t* map_out) {
    if (!t || !map_out || x_col < 0 || x_col >= t->c || y_col < 0 || y_col >= t->c || x_col == y_col)
        return fail(RGBM_ERR_ARG, "rgbm_table_fd_map: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const int nx = t->n_codes[x_col], ny = t->n_codes[y_col];
        if (nx <= 0) return RGBM_OK;
        const long long n = t->n;
        int* d_lo = scr<int>(*t, SCR_TABLE_A, (size_t)nx);
        int* d_hi = scr<int>(*t, SCR_TABLE_B, (size_t)nx);
        int32_t* d_map = scr<int32_t>(*t, SCR_VALS, (size_t)nx);
        hipLaunchKernelGGL(k_fd_init, dim3(nblocks(nx, 256)), dim3(256), 0, s, d_lo, d_hi, nx);
        if (n > 0) {
            // enough workgroups to fill the device a few times over, each on a whole number of load tiles
            const long long tile = (long long)FD_B * FD_UNROLL;
            const long long chunks = std::max<long long>(1, std::min<long long>((n + 4 * tile - 1) / (4 * tile), 2048));
            const long long rows_per_wg = ((n + chunks - 1) / chunks + tile - 1) / tile * tile;
            const unsigned grid = (unsigned)((n + rows_per_wg - 1) / rows_per_wg);
            const int32_t* x = t->codes.p + (size_t)x_col * n;
            const int32_t* y = t->codes.p + (size_t)y_col * n;
            if (nx <= FD_LDS_CODES)
                hipLaunchKernelGGL(k_fd_map<true>, dim3(grid), dim3(FD_B), (size_t)nx * 2 * sizeof(int), s, x, y, n, nx, ny, rows_per_wg, d_lo, d_hi);
            else
                hipLaunchKernelGGL(k_fd_map<false>, dim3(grid), dim3(FD_B), 0, s, x, y, n, nx, ny, rows_per_wg, d_lo, d_hi);
        }
        hipLaunchKernelGGL(k_fd_finish, dim3(nblocks(nx, 256)), dim3(256), 0, s, d_lo, d_hi, nx, d_map);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(map_out, d_map, (size_t)nx * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

// scratch slots held together: IN_COLS (lut) VALS (labels)
RGBM_EXPORT int rgbm_table_rule_fill(rgbm_table* t, int32_t y_col, int32_t x_col, const int32_t* lut, int32_t n_lut, int64_t row_begin,
                                     int64_t n_rows, int32_t* out_label) {
    if (!t || y_col < 0 || y_col >= t->c || x_col >= t->c || x_col == y_col || !lut || n_lut < 1 || row_begin < 0 || n_rows < 0 ||
        row_begin > t->n || n_rows > t->n - row_begin)
        return fail(RGBM_ERR_ARG, "rgbm_table_rule_fill: bad argument");
    return guarded([&]() {
        use_device(t->device);
        rgh::ViewWrite view_wr(t);
        if (n_rows == 0) return RGBM_OK;
        const int ny = t->n_codes[y_col];
        for (int i = 0; i < n_lut; ++i)
            if (lut[i] >= ny) throw std::invalid_argument("rgbm_table_rule_fill: code outside the target column's dictionary");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        const int32_t* d_lut = scr_upload<int32_t>(*t, SCR_IN_COLS, lut, (size_t)n_lut, s);
        int32_t* d_out = out_label ? scr<int32_t>(*t, SCR_VALS, (size_t)n_rows) : nullptr;
        hipLaunchKernelGGL(k_rule_fill, dim3(nblocks(n_rows, 256)), dim3(256), 0, s, t->codes.p, (long long)t->n, (int)y_col, (int)(x_col < 0 ? -1 : x_col),
                           d_lut, (int)n_lut, (long long)row_begin, (long long)n_rows, d_out);
        HIPCHK(hipGetLastError());
        if (out_label) HIPCHK(hipMemcpyAsync(out_label, d_out, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_nearest_values(int32_t device_id, const int32_t* a_cp, const int64_t* a_off, int64_t n_a, const int32_t* b_cp,
                                    const int64_t* b_off, int64_t n_b, const double* cost, double threshold, int32_t* nearest_out) {
    if (n_a < 0 || n_b < 0 || (n_a > 0 && !nearest_out) || (!cost && ((n_a > 0 && !a_off) || (n_b > 0 && !b_off))))
        return fail(RGBM_ERR_ARG, "rgbm_nearest_values: bad argument");
    return guarded([&]() {
        if (!cost) {
            check_pool_offsets(a_off, n_a, a_cp, "rgbm_nearest_values", "a");
            check_pool_offsets(b_off, n_b, b_cp, "rgbm_nearest_values", "b");
        }
        if (n_a == 0) return RGBM_OK;
        if (n_b == 0) { for (int64_t i = 0; i < n_a; ++i) nearest_out[i] = -1; return RGBM_OK; }
        if (n_b > 0x7FFFFFFF || n_a > NV_MAX_CELLS / n_b) throw std::invalid_argument("rgbm_nearest_values: the cost matrix holds more than 2^30 entries");
        use_device(device_id);
        StreamGuard sg;
        DevBuf<int32_t> d_out((size_t)n_a);
        const unsigned grid = nblocks(n_a, 4);               // one wave per row, four rows a workgroup
        if (cost) {
            DevBuf<double> d_cost((size_t)n_a * n_b);
            d_cost.upload(cost, (size_t)n_a * n_b, sg.s);
            hipLaunchKernelGGL(k_row_nearest<double>, dim3(grid), dim3(256), 0, sg.s, d_cost.p, (long long)n_a, (int)n_b, threshold, d_out.p);
            HIPCHK(hipGetLastError());
            d_out.download(nearest_out, (size_t)n_a, sg.s);
            HIPCHK(hipStreamSynchronize(sg.s));
        } else {
            DevBuf<int32_t> d_dist((size_t)n_a * n_b);       // stays in HBM: only the positions leave the device
            edit_distance_on_device(a_cp, a_off, n_a, b_cp, b_off, n_b, d_dist.p, sg.s);
            hipLaunchKernelGGL(k_row_nearest<int32_t>, dim3(grid), dim3(256), 0, sg.s, d_dist.p, (long long)n_a, (int)n_b, threshold, d_out.p);
            HIPCHK(hipGetLastError());
            d_out.download(nearest_out, (size_t)n_a, sg.s);
            HIPCHK(hipStreamSynchronize(sg.s));
        }
        return RGBM_OK;
    });
}

}  // extern "C"

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
namespace {

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

// =============================================================================================
// q-gram k-means in code space (RepairMisc.splitInputTable; the statement is repair/qgram_kmeans.py): one Lloyd assignment
// step over the resident codes.  The host hands P = -2 E C^T ([d_tot][k] float64, one row per dictionary entry of the listed columns) and
// h_k = |C_k|^2; the score of a row for cluster kk is  ((h[kk] + P[off_0 + code_0][kk]) + P[off_1 + code_1][kk]) + ...  in `cols` order,
// float64, additions only (a NULL code adds nothing); the label is the lowest kk with the least score.
//   k_kmeans_assign   one row per lane, consecutive lanes on consecutive rows (every column load coalesced), KM_UNROLL rows a lane in flight.
//                     The clusters are scored in register chunks of KM_KC: a chunk walks the columns once, so a table of k <= KM_KC clusters
//                     reads its codes once for the scores (ceil(k / KM_KC) times otherwise, the re-reads from the caches: a workgroup's
//                     tile is 16 KiB per column) and once more for the counts.  The order of the additions of one cluster never changes.
//                     One workgroup of 1024 threads per CU owns the CU's 160 KiB of LDS: 96 KiB for P and h, 56 KiB for
//                     the counters, 8 KiB left.  P and h live in LDS up to KM_LDS_P_DOUBLES doubles, a code's row padded to an ODD number of doubles so that rows of
//                     different codes start in different 8-byte bank slots; above the bound they are read where they lie (global memory).
//                     counts[kk][code]: 32-bit LDS counters up to KM_LDS_COUNTERS of them, the non-zero ones flushed with 64-bit global
//                     atomics; above that 64-bit global atomics per (row, column).  A workgroup sees at most KM_ROWS_PER_WG_MAX rows of at
//                     most KM_MAX_COLS columns: 2^30 increments, a 32-bit counter cannot wrap.  sizes / n_changed: the lanes of a wave
//                     that hold the same label add once (ballot + popcount) into LDS, one global atomic per workgroup and cluster.
//                     Every sum is an integer sum: the result does not depend on the launch geometry.
// Algorithmic bytes per row: 4 B per column (scores) + 4 B per column (counts) + 4 B previous label + 4 B new label.
// =============================================================================================
namespace {

constexpr int KM_B = 1024;                                  // threads per workgroup: the 16 waves a CU holds at this kernel's registers
constexpr int KM_UNROLL = 4;                                // rows a lane keeps in flight
constexpr int KM_KC = 8;                                    // clusters scored per register chunk
constexpr int KM_LDS_P_DOUBLES = 12288;                     // P and h in LDS: (d_tot + 1) * (k | 1) doubles at most (96 KiB)
constexpr int KM_LDS_COUNTERS = 14336;                      // counts in LDS: k * d_tot 32-bit counters at most (56 KiB)
constexpr long long KM_ROWS_PER_WG_MAX = 1ll << 20;
constexpr int KM_MAX_COLS = 1024, KM_MAX_K = 64;
constexpr long long KM_MAX_CELLS = 1ll << 27;               // d_tot * k

struct KmCol { long long off; int32_t col, n_codes; };

// p: [d_tot + 1][k], row d_tot = h.  out: sizes [k], then n_changed.
template <bool P_LDS, bool C_LDS>
__global__ __launch_bounds__(KM_B) void k_kmeans_assign(const int32_t* __restrict__ codes, long long n, const KmCol* __restrict__ cd, int ncols, int k,
                                                        const double* __restrict__ p, long long d_tot, int first, long long rows_per_wg,
                                                        int32_t* __restrict__ assign, unsigned long long* __restrict__ counts,
                                                        unsigned long long* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char km_smem[];
    const int tid = threadIdx.x;
    const int st = P_LDS ? (k | 1) : k;                                          // doubles from one code's row to the next
    const unsigned n_lp = P_LDS ? (unsigned)(d_tot + 1) * (unsigned)st : 0u;
    const unsigned n_lc = C_LDS ? (unsigned)k * (unsigned)d_tot : 0u;
    double* lp = reinterpret_cast<double*>(km_smem);
    unsigned* lc = reinterpret_cast<unsigned*>(km_smem + (size_t)n_lp * 8);
    unsigned* lsz = lc + n_lc;                                                  // [k] sizes, [k] = rows that changed their label
    if (P_LDS) {
        const unsigned tot = (unsigned)(d_tot + 1) * (unsigned)k;
        for (unsigned i = tid; i < tot; i += KM_B) lp[(i / (unsigned)k) * (unsigned)st + i % (unsigned)k] = p[i];
    }
    for (unsigned i = tid; i < n_lc + (unsigned)k + 1u; i += KM_B) lc[i] = 0;    // (lsz follows lc)
    __syncthreads();
    const double* P = P_LDS ? lp : p;
    const double* hrow = P + d_tot * st;
    const long long begin = (long long)blockIdx.x * rows_per_wg;
    const long long end = begin + rows_per_wg < n ? begin + rows_per_wg : n;
    for (long long base = begin; base < end; base += (long long)KM_B * KM_UNROLL) {
        bool in[KM_UNROLL]; int best[KM_UNROLL]; double bs[KM_UNROLL];
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) { in[u] = base + (long long)u * KM_B + tid < end; best[u] = 0; bs[u] = 0.0; }
        for (int kc = 0; kc < k; kc += KM_KC) {
            const int kn = k - kc < KM_KC ? k - kc : KM_KC;
            double s[KM_UNROLL][KM_KC];
#pragma unroll
            for (int c = 0; c < KM_KC; ++c) {
                const double hv = c < kn ? hrow[kc + c] : 0.0;
#pragma unroll
                for (int u = 0; u < KM_UNROLL; ++u) s[u][c] = hv;
            }
            for (int j = 0; j < ncols; ++j) {
                const KmCol d = cd[j];
                const int32_t* col = codes + (long long)d.col * n + base + tid;
                int v[KM_UNROLL];
#pragma unroll
                for (int u = 0; u < KM_UNROLL; ++u) v[u] = in[u] ? col[(long long)u * KM_B] : -1;      // KM_UNROLL coalesced loads in flight
#pragma unroll
                for (int u = 0; u < KM_UNROLL; ++u) {
                    if (v[u] < 0 || v[u] >= d.n_codes) continue;                                        // NULL adds nothing
                    const double* q = P + (d.off + v[u]) * st + kc;
#pragma unroll
                    for (int c = 0; c < KM_KC; ++c) if (c < kn) s[u][c] = s[u][c] + q[c];
                }
            }
#pragma unroll
            for (int u = 0; u < KM_UNROLL; ++u) {
#pragma unroll
                for (int c = 0; c < KM_KC; ++c)
                    if (c < kn && ((kc == 0 && c == 0) || s[u][c] < bs[u])) { bs[u] = s[u][c]; best[u] = kc + c; }   // ascending, strict: the lowest id wins
            }
        }
#pragma unroll
        for (int u = 0; u < KM_UNROLL; ++u) {
            const long long r = base + (long long)u * KM_B + tid;
            bool moved = false;
            if (in[u]) {
                moved = first || assign[r] != best[u];
                assign[r] = best[u];
            }
            const unsigned long long mv = __ballot(moved);
            if (lane_id() == 0 && mv) atomicAdd(&lsz[k], (unsigned)__popcll(mv));
            unsigned long long pend = __ballot(in[u]);
            while (pend) {                                                       // one LDS atomic per label the wave holds
                const int leader = __ffsll((long long)pend) - 1;
                const int lab = __shfl(best[u], leader);
                const unsigned long long same = __ballot(in[u] && best[u] == lab);
                if (lane_id() == leader) atomicAdd(&lsz[lab], (unsigned)__popcll(same));
                pend &= ~same;
            }
        }
        for (int j = 0; j < ncols; ++j) {
            const KmCol d = cd[j];
            const int32_t* col = codes + (long long)d.col * n + base + tid;
            int v[KM_UNROLL];
#pragma unroll
            for (int u = 0; u < KM_UNROLL; ++u) v[u] = in[u] ? col[(long long)u * KM_B] : -1;
#pragma unroll
            for (int u = 0; u < KM_UNROLL; ++u) {
                if (v[u] < 0 || v[u] >= d.n_codes) continue;
                const long long cell = (long long)best[u] * d_tot + d.off + v[u];
                if (C_LDS) atomicAdd(&lc[cell], 1u);
                else atomicAdd(&counts[cell], 1ull);
            }
        }
    }
    __syncthreads();
    if (C_LDS)
        for (unsigned i = tid; i < n_lc; i += KM_B) { const unsigned v = lc[i]; if (v) atomicAdd(&counts[i], (unsigned long long)v); }
    for (int i = tid; i <= k; i += KM_B) { const unsigned v = lsz[i]; if (v) atomicAdd(&out[i], (unsigned long long)v); }
}

template <bool P_LDS, bool C_LDS>
void kmeans_launch(unsigned grid, size_t lds, hipStream_t s, const int32_t* codes, long long n, const KmCol* cd, int ncols, int k, const double* p,
                   long long d_tot, int first, long long rows_per_wg, int32_t* assign, unsigned long long* counts, unsigned long long* out) {
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_kmeans_assign<P_LDS, C_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_kmeans_assign<P_LDS, C_LDS>), dim3(grid), dim3(KM_B), lds, s, codes, n, cd, ncols, k, p, d_tot, first, rows_per_wg, assign,
                       counts, out);
}

}  // namespace

extern "C" {

// scratch slots held together: TABLE_A (P, h) TABLE_B (column descriptors) VALS (counts, sizes, n_changed)
RGBM_EXPORT int rgbm_table_kmeans_assign(rgbm_table* t, const int32_t* cols, int32_t n_cols, const int64_t* code_off, int32_t k, const double* p,
                                         int64_t d_tot, const double* h, int32_t first, int64_t* counts_out, int64_t* sizes_out,
                                         int64_t* n_changed_out) {
    if (!t || !p || !h || !counts_out || !sizes_out || !n_changed_out) return fail(RGBM_ERR_ARG, "rgbm_table_kmeans_assign: bad argument");
    return guarded([&]() {
        use_device(t->device);
        if (k < 2 || k > KM_MAX_K) throw std::invalid_argument("rgbm_table_kmeans_assign: k must be 2 .. 64");
        if (n_cols < 1 || n_cols > KM_MAX_COLS || !cols || !code_off) throw std::invalid_argument("rgbm_table_kmeans_assign: 1 .. 1024 columns expected");
        check_cols(*t, cols, n_cols, "rgbm_table_kmeans_assign");
        if (d_tot < 1 || d_tot > KM_MAX_CELLS / k) throw std::invalid_argument("rgbm_table_kmeans_assign: d_tot * k must be 1 .. 2^27");
        std::vector<KmCol> cd((size_t)n_cols);
        for (int j = 0; j < n_cols; ++j) {
            const int32_t nc = std::max<int32_t>(t->n_codes[cols[j]], 0);
            if (code_off[j] < 0 || code_off[j] > d_tot - nc) throw std::invalid_argument("rgbm_table_kmeans_assign: a column's codes do not fit into d_tot");
            cd[j] = KmCol{(long long)code_off[j], cols[j], nc};
        }
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!first && !t->km_valid) throw std::invalid_argument("rgbm_table_kmeans_assign: first == 0 without a previous assignment of this table");
        const long long n = t->n;
        const size_t cells = (size_t)k * (size_t)d_tot;
        if (t->km_assign.n < (size_t)std::max<long long>(n, 1)) t->km_assign.alloc((size_t)std::max<long long>(n, 1));      // (only when there is no previous one)
        const KmCol* d_cd = scr_upload<KmCol>(*t, SCR_TABLE_B, cd.data(), cd.size(), s);
        double* d_p = scr<double>(*t, SCR_TABLE_A, cells + (size_t)k);
        HIPCHK(hipMemcpyAsync(d_p, p, cells * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_p + cells, h, (size_t)k * 8, hipMemcpyHostToDevice, s));
        unsigned long long* d_out = scr<unsigned long long>(*t, SCR_VALS, cells + (size_t)k + 1);     // counts, sizes, n_changed
        HIPCHK(hipMemsetAsync(d_out, 0, (cells + (size_t)k + 1) * 8, s));
        if (n > 0) {
            const bool p_lds = (d_tot + 1) * (long long)(k | 1) <= KM_LDS_P_DOUBLES, c_lds = (long long)cells <= KM_LDS_COUNTERS;
            const size_t lds = (p_lds ? (size_t)(d_tot + 1) * (size_t)(k | 1) * 8 : 0) + ((c_lds ? cells : 0) + (size_t)k + 1) * 4;
            // two rounds of workgroups (one per CU) over the device at most, each on a whole number of load tiles and no more than KM_ROWS_PER_WG_MAX rows
            const long long tile = (long long)KM_B * KM_UNROLL;
            long long chunks = std::min<long long>((n + tile - 1) / tile, 512);
            chunks = std::max<long long>(chunks, (n + KM_ROWS_PER_WG_MAX - 1) / KM_ROWS_PER_WG_MAX);
            const long long rows_per_wg = ((n + chunks - 1) / chunks + tile - 1) / tile * tile;
            const unsigned grid = (unsigned)((n + rows_per_wg - 1) / rows_per_wg);
            // (P in LDS implies the counters in LDS: k * d_tot < (d_tot + 1) * (k | 1) <= KM_LDS_P_DOUBLES < KM_LDS_COUNTERS)
            static_assert(KM_LDS_P_DOUBLES <= KM_LDS_COUNTERS, "a table whose P fits the LDS keeps its counters there too");
            auto go = p_lds ? kmeans_launch<true, true> : (c_lds ? kmeans_launch<false, true> : kmeans_launch<false, false>);
            go(grid, lds, s, t->codes.p, n, d_cd, (int)n_cols, (int)k, d_p, (long long)d_tot, first ? 1 : 0, rows_per_wg, t->km_assign.p, d_out, d_out + cells);
            HIPCHK(hipGetLastError());
        }
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are 64-bit");
        HIPCHK(hipMemcpyAsync(counts_out, d_out, cells * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(sizes_out, d_out + cells, (size_t)k * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(n_changed_out, d_out + cells + k, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        t->km_valid = true;
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_kmeans_read(const rgbm_table* t, int32_t* assign_out) {
    if (!t || !assign_out) return fail(RGBM_ERR_ARG, "rgbm_table_kmeans_read: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        if (!t->km_valid) throw std::invalid_argument("rgbm_table_kmeans_read: no rgbm_table_kmeans_assign result on this table");
        HIPCHK(hipMemcpyAsync(assign_out, t->km_assign.p, (size_t)t->n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return RGBM_OK;
    });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// distinct rows (rgbm_table_distinct_rows; the host statement is repair.pipeline.distinct_rows): the rows of the table grouped by
// equality over ALL columns (NULL is a value of its own), the groups in order of FIRST OCCURRENCE, a group of cnt rows kept as
// ceil(cnt / 255) consecutive copies whose multiplicities are 255, .., 255, cnt - 255 * (copies - 1).  The result is a function of the
// table alone: the hash, the slot a group lands in and the launch geometry never show in it.
//   k_dr_keys     the mixed-radix uint64 key words of every row, [W][n] (digit = code + 1, a code outside [0, n_codes) is NULL = 0;
//                 a new word starts where the next radix would pass 2^63 -- the words pipeline.distinct_rows builds)
//   k_dr_insert   open addressing over >= 2n slots.  A slot holds a ROW INDEX of its group (claimed with atomicCAS) and, once the kernel
//                 is done, the group's SMALLEST row index (integer atomicMin: order-free); count[slot] takes the group's rows (integer
//                 atomicAdd: order-free).  An occupied slot is compared word for word with the probing row's key.  Probe reads are
//                 agent-scope atomic loads (L2, never a stale L1 line); the probe loop ends after `cap` slots at the latest and then
//                 raises the error flag.  The count goes through wave_add (a table of a few distinct rows with millions of copies each);
//                 the atomicMin is skipped by every row that already sees a smaller index in the slot.
//   k_dr_mark     row i is its group's representative iff slot[row_slot[i]] == i  -> mask for the ordered compaction (k_flag<1>,
//                 k_scan_counts, k_emit: ascending representatives = groups by first occurrence)
//   k_dr_copies   copies per group; k_scan_counts over them gives every group's first output row
//   k_dr_source   per output row: the table row it copies and its multiplicity; the group's first output row is left with the
//                 representative for k_dr_inverse.  k_gather_rows then writes the codes.
// Algorithmic bytes per row: 4 B per column (keys) + 8 W (insert) + ~12 B of slot traffic + 4 B slot id, then 4 B per column and
// output row for the gather and 8 B for `inverse`.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int DR_EMPTY = 0x7F7F7F7F;              // hipMemsetAsync(0x7F); above every row index (n <= 2^30)
constexpr unsigned DR_NO_SLOT = 0xFFFFFFFFu;
constexpr int DR_WAVE_ROUNDS = 8;                 // slots a wave combines before its remaining lanes add on their own

__global__ __launch_bounds__(256) void k_dr_keys(const int32_t* __restrict__ codes, long long n, int c, const unsigned long long* __restrict__ radix,
                                                 const int32_t* __restrict__ word_of, unsigned long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long k = 0; int w = 0;
    for (int cc = 0; cc < c; ++cc) {
        if (word_of[cc] != w) { keys[(long long)w * n + i] = k; k = 0; w = word_of[cc]; }
        k = k * radix[cc] + key_digit<true>(codes[(long long)cc * n + i], radix[cc]);
    }
    keys[(long long)w * n + i] = k;
}

__global__ __launch_bounds__(256) void k_dr_insert(const unsigned long long* __restrict__ keys, long long n, int W, int* __restrict__ slots,
                                                   unsigned* __restrict__ count, unsigned long long cap, unsigned* __restrict__ row_slot,
                                                   unsigned* __restrict__ err) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;                     // no early return: every lane takes part in the ballots below
    unsigned long long slot = 0; bool found = false;
    if (valid) {
        unsigned long long h = 0;
        for (int w = 0; w < W; ++w) h = mix64(h ^ keys[(long long)w * n + i]);
        const unsigned long long cap_mask = cap - 1ull;
        slot = h & cap_mask;
        for (unsigned long long probe = 0; probe < cap; ++probe) {
            int prev = __hip_atomic_load(&slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (prev == DR_EMPTY) { prev = atomicCAS(&slots[slot], DR_EMPTY, (int)i); if (prev == DR_EMPTY) { found = true; break; } }
            if (prev < 0 || (long long)prev >= n) break;                      // never a row index: give up, the flag says so
            bool same = true;
            for (int w = 0; w < W; ++w) same = same && keys[(long long)w * n + prev] == keys[(long long)w * n + i];
            if (same) { found = true; break; }
            slot = (slot + 1ull) & cap_mask;
        }
        if (!found) atomicOr(err, 1u);
        row_slot[i] = found ? (unsigned)slot : DR_NO_SLOT;
        if (found && __hip_atomic_load(&slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (int)i) atomicMin(&slots[slot], (int)i);
    }
    wave_add<DR_WAVE_ROUNDS>(count, (unsigned)slot, found);       // (the arrival rank is of no use here)
}

__global__ __launch_bounds__(256) void k_dr_mark(const int* __restrict__ slots, const unsigned* __restrict__ row_slot, long long n,
                                                 unsigned long long cap, uint8_t* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned s = row_slot[i];
    mask[i] = ((unsigned long long)s < cap && (long long)slots[s] == i) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_dr_copies(const long long* __restrict__ rep_rows, long long G, long long n, const unsigned* __restrict__ row_slot,
                                                   const unsigned* __restrict__ count, unsigned long long cap, unsigned* __restrict__ copies) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const long long r = rep_rows[g];
    const unsigned s = (r >= 0 && r < n) ? row_slot[r] : DR_NO_SLOT;
    const unsigned cnt = (unsigned long long)s < cap ? count[s] : 1u;
    copies[g] = (cnt + 254u) / 255u;
}

__global__ __launch_bounds__(256) void k_dr_source(const long long* __restrict__ rep_rows, const long long* __restrict__ goff, const unsigned* __restrict__ copies,
                                                   long long G, long long M, long long n, const unsigned* __restrict__ row_slot,
                                                   const unsigned* __restrict__ count, unsigned long long cap, long long* __restrict__ src_row,
                                                   uint8_t* __restrict__ mult, unsigned* __restrict__ first_out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= M) return;
    long long g = p;
    if (M != G) {                                 // some group has more than one copy: the last group that starts at or before p
        long long lo = 0, hi = G;
        while (lo < hi) { const long long mid = (lo + hi) >> 1; if (goff[mid] <= p) lo = mid + 1; else hi = mid; }
        g = lo > 0 ? lo - 1 : 0;
    }
    const long long r = rep_rows[g];
    const long long k = p - goff[g];
    const unsigned cp = copies[g];
    const unsigned s = (r >= 0 && r < n) ? row_slot[r] : DR_NO_SLOT;
    const unsigned cnt = (unsigned long long)s < cap ? count[s] : 1u;
    src_row[p] = (r >= 0 && r < n) ? r : 0;
    mult[p] = (uint8_t)(k + 1 == (long long)cp ? cnt - 255u * (cp - 1u) : 255u);
    if (k == 0 && r >= 0 && r < n) first_out[r] = (unsigned)p;
}

__global__ __launch_bounds__(256) void k_dr_inverse(const int* __restrict__ slots, const unsigned* __restrict__ row_slot, const unsigned* __restrict__ first_out,
                                                    long long n, unsigned long long cap, long long* __restrict__ inverse) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned s = row_slot[i];
    const long long r = (unsigned long long)s < cap ? (long long)slots[s] : i;
    inverse[i] = (r >= 0 && r < n) ? (long long)first_out[r] : -1;
}

}  // namespace

// the one copy of the pass: rgbm_table_distinct_rows and the distinct-row view of rgbm_table_train (rgbm.hip) both run it
rgh::DistinctOut rgh::distinct_rows_device(const rgbm_table& tab, int64_t* inverse_out, int64_t max_rows) {
    const rgbm_table* t = &tab;
    if (t->n > (1ll << 30)) throw distinct_cannot("rgbm_table_distinct_rows: more than 2^30 rows");
    if (t->has_mult) throw std::invalid_argument("rgbm_table_distinct_rows: the table carries row multiplicities itself (clear them first)");
    {
        use_device(t->device);
        const long long n = t->n; const int c = t->c;
        // the key words: as few as the radices need (pipeline.distinct_rows: a new word where the next radix would pass 2^63)
        std::vector<unsigned long long> radix((size_t)c); std::vector<int32_t> word_of((size_t)c);
        int W = 1; unsigned __int128 room = 1;
        for (int j = 0; j < c; ++j) {
            radix[j] = (unsigned long long)std::max<int32_t>(t->n_codes[j], 0) + 1ull;
            if (room * radix[j] >= ((unsigned __int128)1 << 63)) { ++W; room = 1; }
            room *= radix[j];
            word_of[j] = W - 1;
        }
        const unsigned long long cap = table_capacity(n);
        // everything the call allocates, with the output table at its largest (M <= n): slots + counts (8 B a slot); per row the slot id, the key
        // words, the compaction's mask and ballots, representative, copies, group offset, source row, first output row, inverse; the output's
        // codes and multiplicities.  Above half of the device memory the call is refused; a table that passes and still does not fit (other tables
        // and fits share the device) fails in the allocator with its own message.
        const unsigned long long work = cap * 8ull + (unsigned long long)n * (4ull + 8ull * W + 2ull + 8ull + 4ull + 8ull + 8ull + 4ull + 8ull + 4ull * c + 1ull);
        size_t mem_free = 0, mem_total = 0;
        HIPCHK(hipMemGetInfo(&mem_free, &mem_total));
        if (work > mem_total / 2)
            throw distinct_cannot("rgbm_table_distinct_rows: the working set (" + std::to_string(work >> 20) + " MB) exceeds half of the device memory");
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        DevBuf<unsigned long long> d_radix((size_t)c), keys((size_t)W * n);
        DevBuf<int32_t> d_word((size_t)c);
        d_radix.upload(radix.data(), (size_t)c, s); d_word.upload(word_of.data(), (size_t)c, s);
        DevBuf<int> slots((size_t)cap); DevBuf<unsigned> count((size_t)cap), row_slot((size_t)n), err(1);
        HIPCHK(hipMemsetAsync(slots.p, 0x7F, (size_t)cap * 4, s));
        count.zero(s); err.zero(s);
        const unsigned nb = nblocks(n, 256);
        hipLaunchKernelGGL(k_dr_keys, dim3(nb), dim3(256), 0, s, t->codes.p, n, c, d_radix.p, d_word.p, keys.p);
        hipLaunchKernelGGL(k_dr_insert, dim3(nb), dim3(256), 0, s, keys.p, n, W, slots.p, count.p, cap, row_slot.p, err.p);
        HIPCHK(hipGetLastError());
        unsigned h_err = 0;
        HIPCHK(hipMemcpyAsync(&h_err, err.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (h_err) throw std::runtime_error("rgbm_table_distinct_rows: a probe sequence ran through the whole hash table");
        keys.release();
        // ascending representatives = the groups by first occurrence
        DevBuf<uint8_t> mask((size_t)n);
        hipLaunchKernelGGL(k_dr_mark, dim3(nb), dim3(256), 0, s, slots.p, row_slot.p, n, cap, mask.p);
        const long long nblk = (n + PROWS - 1) / PROWS;
        DevBuf<unsigned long long> ballots((size_t)nblk * PBAL); DevBuf<unsigned> bcount((size_t)nblk); DevBuf<long long> boff((size_t)nblk + 1);
        hipLaunchKernelGGL(k_flag<1>, dim3((unsigned)nblk, 1u), dim3(PB), 0, s, (const int32_t*)nullptr, mask.p, (const int32_t*)nullptr, n, nblk, ballots.p, bcount.p);
        DevBuf<long long> rep_rows;
        const long long G = scan_emit(ballots.p, bcount.p, boff.p, nblk, 1, nullptr, s, [&](long long g, long long** rows, int32_t**) {
            if (g < 1 || g > n) throw std::runtime_error("rgbm_table_distinct_rows: inconsistent group count");
            rep_rows.alloc((size_t)g); *rows = rep_rows.p;
        });
        // output rows per group (the 255 split) and every group's first output row
        DevBuf<unsigned> copies((size_t)G); DevBuf<long long> goff((size_t)G + 1);
        hipLaunchKernelGGL(k_dr_copies, dim3(nblocks(G, 256)), dim3(256), 0, s, rep_rows.p, G, n, row_slot.p, count.p, cap, copies.p);
        hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, copies.p, G, goff.p, goff.p + G);
        HIPCHK(hipGetLastError());
        long long M = 0;
        HIPCHK(hipMemcpyAsync(&M, goff.p + G, sizeof(long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (M < G || M > n) throw std::runtime_error("rgbm_table_distinct_rows: inconsistent output row count");
        if (max_rows >= 0 && M > max_rows) { DistinctOut res; res.rows = M; return res; }      // (the view: not worth a table)
        std::unique_ptr<rgbm_table> o(new rgbm_table());
        o->device = t->device; o->n = M; o->c = c; o->n_codes = t->n_codes; o->col_values = t->col_values; o->col_kind = t->col_kind;
        o->codes.alloc((size_t)M * c); o->mult.alloc((size_t)M);
        DevBuf<long long> src_row((size_t)M); DevBuf<unsigned> first_out((size_t)n);
        hipLaunchKernelGGL(k_dr_source, dim3(nblocks(M, 256)), dim3(256), 0, s, rep_rows.p, goff.p, copies.p, G, M, n, row_slot.p, count.p, cap, src_row.p,
                           o->mult.p, first_out.p);
        hipLaunchKernelGGL(k_gather_rows, dim3(nblocks(M, 256), (unsigned)c), dim3(256), 0, s, t->codes.p, n, o->codes.p, M, src_row.p);
        HIPCHK(hipGetLastError());
        if (inverse_out) {
            DevBuf<long long> inv((size_t)n);
            hipLaunchKernelGGL(k_dr_inverse, dim3(nb), dim3(256), 0, s, slots.p, row_slot.p, first_out.p, n, cap, inv.p);
            HIPCHK(hipGetLastError());
            static_assert(sizeof(long long) == sizeof(int64_t), "row positions are 64-bit");
            HIPCHK(hipMemcpyAsync(inverse_out, inv.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        HIPCHK(hipStreamSynchronize(s));
        o->has_mult = true; o->mult_total = n;
        DistinctOut res; res.rows = M; res.tab = std::move(o);
        return res;
    }
}

extern "C" {

RGBM_EXPORT int rgbm_table_distinct_rows(const rgbm_table* t, rgbm_table** out, int64_t* n_out, int64_t* inverse_out) {
    if (!t || !out || !n_out || t->n <= 0 || t->c <= 0) return fail(RGBM_ERR_ARG, "rgbm_table_distinct_rows: bad argument");
    return guarded([&]() {
        DistinctOut res = distinct_rows_device(*t, inverse_out, -1);
        *n_out = res.rows;
        *out = res.tab.release();
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_table_read_row_multiplicity(const rgbm_table* t, uint8_t* mult_out) {
    if (!t || !mult_out) return fail(RGBM_ERR_ARG, "rgbm_table_read_row_multiplicity: bad argument");
    return guarded([&]() {
        use_device(t->device);
        std::lock_guard<std::mutex> prep_lk(t->prep_mu);
        if (!t->has_mult) { memset(mult_out, 1, (size_t)t->n); return RGBM_OK; }
        HIPCHK(hipMemcpy(mult_out, t->mult.p, (size_t)t->n, hipMemcpyDeviceToHost));
        return RGBM_OK;
    });
}

}  // extern "C"

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
// Single tuple: one bit per (column, code) -- k_row_bits ANDs them per row in one streaming pass.
// ---------------------------------------------------------------------------------------------
namespace {

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

}  // namespace

extern "C" {

// scratch slots held together: ROW_MASK | BALLOTS BCOUNT BOFF | COLS          (its hash table and operands are DevBufs)
RGBM_EXPORT int rgbm_table_detect_dc(rgbm_table* t, const rgbm_dc_pred* preds, int32_t n_preds, const int32_t* cell_cols, int32_t n_cell_cols,
                                     int64_t max_pairs, int64_t* n_rows_out, int64_t* n_cells_out) {
    if (!t || !preds || n_preds < 2 || n_preds > DC_MAX_PREDS || n_cell_cols < 0 || (n_cell_cols > 0 && !cell_cols) || !n_cells_out)
        return fail(RGBM_ERR_ARG, "rgbm_table_detect_dc: bad argument (2 to 16 predicates)");
    // the EQ attributes (each once) and the predicates evaluated over pairs
    std::vector<int32_t> eq;
    std::vector<const rgbm_dc_pred*> others;
    for (int i = 0; i < n_preds; ++i) {
        const rgbm_dc_pred& p = preds[i];
        if (p.op < RGBM_DC_EQ || p.op > RGBM_DC_GT) return fail(RGBM_ERR_ARG, "rgbm_table_detect_dc: unknown predicate");
        if (p.left_col < 0 || p.left_col >= t->c || p.right_col < 0 || p.right_col >= t->c)
            return fail(RGBM_ERR_ARG, "rgbm_table_detect_dc: column index out of range");
        if ((p.op == RGBM_DC_EQ || p.op == RGBM_DC_IQ) && (p.left_col != p.right_col || p.left_rank || p.right_rank))
            return fail(RGBM_ERR_ARG, "rgbm_table_detect_dc: EQ / IQ take one attribute on both sides and no rank arrays");
        if (p.op != RGBM_DC_EQ) others.push_back(&p);
        else if (std::find(eq.begin(), eq.end(), p.left_col) == eq.end()) eq.push_back(p.left_col);
    }
    if (eq.size() > 12) return fail(RGBM_ERR_ARG, "rgbm_table_detect_dc: at most 12 EQ attributes");
    if (const int rc = refuse_cols(*t, cell_cols, n_cell_cols, false, nullptr, "rgbm_table_detect_dc")) return rc;
    if (t->n >= (1ll << 31)) return fail(RGBM_ERR_PARAM, "rgbm_table_detect_dc: 2^31 rows or more");
    return guarded([&]() {
        use_device(t->device);
        unsigned __int128 span = 1;
        const KeySpec ks = key_spec(*t, eq.data(), (int)eq.size(), "rgbm_table_detect_dc", &span);
        const long long n = t->n;
        const long long limit = max_pairs > 0 ? (long long)max_pairs : DC_DEFAULT_MAX_PAIRS;
        // the program: operands per pair predicate, the rank arrays one after the other
        DcProgram pg; memset(&pg, 0, sizeof(pg)); pg.np = (int32_t)others.size();
        std::vector<int32_t> ranks;
        unsigned ne_bits = 0;
        auto side = [&](int32_t col, const int32_t* rank) {
            DcSide sd; sd.col = col; sd.n_codes = std::max<int32_t>(t->n_codes[col], 0); sd.rank_off = -1;
            if (rank) { sd.rank_off = (long long)ranks.size(); ranks.insert(ranks.end(), rank, rank + sd.n_codes); }
            return sd;
        };
        for (size_t i = 0; i < others.size(); ++i) {
            pg.p[i].op = others[i]->op;
            pg.p[i].l = side(others[i]->left_col, others[i]->left_rank);
            pg.p[i].r = side(others[i]->right_col, others[i]->right_rank);
            if (others[i]->op == RGBM_DC_IQ) ne_bits |= 1u << i;
        }
        for (int32_t& v : ranks) if (v < 0) v = -1;
        std::lock_guard<std::mutex> prep_lk(t->prep_mu); hipStream_t s = table_stream(*t);
        uint8_t* mask = scr<uint8_t>(*t, SCR_ROW_MASK, (size_t)std::max<long long>(n, 1));
        if (n == 0) return no_cells(*t, true, n_rows_out, n_cells_out);
        if (pg.np == 0) {
            // EQ predicates only: t2 = t1 satisfies them, every row violates
            HIPCHK(hipMemsetAsync(mask, 1, (size_t)n, s));
        } else {
            const unsigned long long cap = table_capacity(n, span);
            DevBuf<unsigned long long> keys((size_t)cap), stats(2);
            DevBuf<unsigned> count((size_t)cap), row_slot((size_t)n), row_rank((size_t)n);
            DevBuf<long long> goff((size_t)cap + 1);
            HIPCHK(hipMemsetAsync(keys.p, 0xFF, (size_t)cap * 8, s));
            count.zero(s); stats.zero(s);
            const unsigned nb = nblocks(n, 256);
            hipLaunchKernelGGL(k_dc_slots, dim3(nb), dim3(256), 0, s, t->codes.p, n, ks, keys.p, count.p, cap - 1, row_slot.p, row_rank.p);
            hipLaunchKernelGGL(k_dc_stats, dim3((unsigned)std::min<unsigned long long>((cap + 255) / 256, 2048ull)), dim3(256), 0, s, count.p, cap, stats.p);
            HIPCHK(hipGetLastError());
            unsigned long long h_stats[2] = {0, 0};
            HIPCHK(hipMemcpyAsync(h_stats, stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (h_stats[0] > (unsigned long long)limit)
                throw std::invalid_argument("rgbm_table_detect_dc: the groups of the EQ attributes hold " + std::to_string(h_stats[0]) +
                                            " pairs, more than max_pairs = " + std::to_string(limit));
            keys.release();
            hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, count.p, (long long)cap, goff.p, goff.p + cap);
            DevBuf<int32_t> perm((size_t)n), gbeg((size_t)n), gend((size_t)n), lop((size_t)pg.np * n), rop((size_t)pg.np * n), d_ranks(std::max<size_t>(ranks.size(), 1));
            d_ranks.upload(ranks.data(), ranks.size(), s);
            hipLaunchKernelGGL(k_dc_scatter, dim3(nb), dim3(256), 0, s, t->codes.p, n, pg, d_ranks.p, row_slot.p, row_rank.p, goff.p, count.p, perm.p, gbeg.p,
                               gend.p, lop.p, rop.p);
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
                if (pg.np <= 2) launch_dc_pairs<2>(nbp, lds, s, lop.p, rop.p, gbeg.p, gend.p, perm.p, (int)n, pg.np, ne_bits, w_off, (int)window, mask);
                else if (pg.np <= 4) launch_dc_pairs<4>(nbp, lds, s, lop.p, rop.p, gbeg.p, gend.p, perm.p, (int)n, pg.np, ne_bits, w_off, (int)window, mask);
                else if (pg.np <= 8) launch_dc_pairs<8>(nbp, lds, s, lop.p, rop.p, gbeg.p, gend.p, perm.p, (int)n, pg.np, ne_bits, w_off, (int)window, mask);
                else launch_dc_pairs<16>(nbp, lds, s, lop.p, rop.p, gbeg.p, gend.p, perm.p, (int)n, pg.np, ne_bits, w_off, (int)window, mask);
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));          // the temporaries go back to the pool
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
