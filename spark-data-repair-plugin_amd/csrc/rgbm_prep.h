// rgbm_prep.h -- what the sources of the relational steps on the HBM-resident code table share (internal, never installed): rgbm_prep.hip
// defines the host functions declared here, every rgbm_<step>.hip beside it includes this header and nothing of another step (one exception:
// rgbm_domain.h, the cell-domain arithmetic as a __device__ function, which rgbm_domain.hip and rgbm_cellset.hip both compile into a kernel).
// Every source uses the ONE copy of each mechanism that this header holds -- compaction: flags_to_ballots, scan_emit (into the
// table's cell list: emit_to_table, compact<MODE>), rows_to_cells;  keys: key_digit / row_key, key_spec, table_capacity, ht_claim, wave_add;
// bitsets: append_bitset, bitset_stage / bitset_test;  scratch: enum Scr, with its rule; every entry point names its slots above its definition.
// A kernel is launched from the source that defines it (no relocatable device code): the four that a second source needs have a host
// function here, next to their definition in rgbm_prep.hip.
#pragma once
#include "rgbm_host.h"

#include <algorithm>
#include <functional>

namespace rgh {

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

constexpr int DET_LDS_WORDS = 1024;      // 64-bit words of a bitset that bitset_stage keeps in LDS (why this many: above k_detect, rgbm_prep.hip)

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

struct KeySpec { int32_t ncols; int32_t col[12]; unsigned long long radix[12]; };
constexpr unsigned long long HT_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31; return x;
}
// digit of a code in the NULL-safe mixed-radix key: code + 1, NULL (-1) -> 0.  CLAMP: a code at or above the column's dictionary (digit >=
// radix) or below -1 counts as NULL, so distinct keys never collide.  Neither rgbm_table_create nor rgbm_table_write_cells refuses such
// codes, and on them the unclamped digit gives other (colliding) keys: rgbm_table_detect_constraint, which has always used it, keeps it
// (CLAMP = false), so that its result stays what it was on every table; the two forms are the same wherever codes lie in [-1, n_codes).
// Unclamped keys are not bounded by the span of the dictionaries: a hash table for them is sized by the rows alone (table_capacity(n)).
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

constexpr int CC_LDS = 8192;              // codes whose 32-bit counters a workgroup keeps in LDS (k_count_codes, k_colstat_count)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline unsigned nblocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

hipStream_t table_stream(const rgbm_table& t);
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
    SCR_COUNTS = 10,      // dense 32-bit counters that workgroups flush into: the joint tables of the fd measures
    SCR_FREE_11 = 11      // nobody's yet
};

// scratch buffer `slot` of the table, at least `count` elements of T (grown with a quarter of headroom, never shrunk).  Under RGBM_GUARD the
// buffer is exactly the bytes asked for, made anew whenever the request differs: the guard zone then begins where the entry's own use must end,
// not a quarter or many times beyond it.  With RGBM_POISON as well it is made anew on EVERY fetch, so that a call of the same size as the
// one before it starts on 0xA5 bytes and not on what that call left (a row mask of n bytes, say); under the guard alone such a repeat keeps
// the earlier content.  Both rest on the rule above: no entry point fetches a slot twice in one call (the earlier pointer would dangle), and
// the previous call's use ended with its synchronise.
template <typename T>
T* scr(const rgbm_table& t, Scr slot, size_t count) {
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (guard_on()) { if (t.scratch[slot].n != bytes || poison_on()) t.scratch[slot].alloc(bytes); }
    else if (t.scratch[slot].n < bytes) t.scratch[slot].alloc(bytes + bytes / 4);
    return reinterpret_cast<T*>(t.scratch[slot].p);
}
template <typename T>
T* scr_upload(const rgbm_table& t, Scr slot, const T* host, size_t count, hipStream_t s) {
    T* d = scr<T>(t, slot, count);
    if (count) HIPCHK(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
}

// The kernels of rgbm_prep.hip that another source needs, enqueued on s (the caller checks hipGetLastError):
// k_flag<1>: the ballots and counts of mask [n] (nblk blocks of PROWS rows, one column)
void launch_flag_rows(const uint8_t* mask, long long n, long long nblk, unsigned long long* ballots, unsigned* bcount, hipStream_t s);
// k_scan_counts: off [m] = exclusive scan of cnt [m], *total = their sum (device memory, all of it)
void launch_scan_counts(const unsigned* cnt, long long m, long long* off, long long* total, hipStream_t s);
// k_gather_rows: out [c][n_out] = the rows `rows` of in [c][n_in]
void launch_gather_rows(const int32_t* in, long long n_in, int c, int32_t* out, long long n_out, const long long* rows, hipStream_t s);

// The ordered compaction behind every flag kernel.  The ballots and counts of nblk x ncols blocks are written: scan the counts, read the total (one
// synchronise), let dest(total, &rows, &cols) size the output (cols stays null for a row list), emit (left in flight).  Returns the total.
long long scan_emit(const unsigned long long* ballots, const unsigned* bcount, long long* off, long long nblk, int ncols, const int32_t* d_cols,
                    hipStream_t s, const std::function<void(long long, long long**, int32_t**)>& dest);

// the table's own compaction buffers (a flag kernel fills ballots and bcount) and scan_emit into its cell list: (row, column) cells when
// d_cols is given, a row list otherwise; returns the cell count
struct Ballots { unsigned long long* ballots; unsigned* bcount; long long* off; long long nblk; int ncols; };
Ballots table_ballots(const rgbm_table& t, int ncols);
long long emit_to_table(rgbm_table& t, const Ballots& b, const int32_t* d_cols, hipStream_t s);
// MODE 0: the NULL cells of columns d_cols (want_cols: with their columns);  MODE 1: the rows of d_mask;  MODE 2: k_detect's cells
// (instantiated in rgbm_prep.hip, where DetDesc and k_detect are)
struct DetDesc;
template <int MODE>
long long compact(rgbm_table& t, const uint8_t* d_mask, const int32_t* d_cols, int ncols, bool want_cols, hipStream_t s,
                  const DetDesc* d_desc = nullptr, const unsigned long long* d_bits = nullptr);

// the m ascending violating rows in t.cell_rows -> rows x cell_cols (column-major): a constraint reports every given attribute of a row
void rows_to_cells(rgbm_table& t, long long m, const int32_t* cell_cols, int n_cell_cols, hipStream_t s, int64_t* n_rows_out, int64_t* n_cells_out);

// an entry point with nothing to look at: the table's cell list becomes empty (row_list: as a list without columns)
int no_cells(rgbm_table& t, bool row_list, int64_t* n_rows_out, int64_t* n_cells_out);

// the key of the columns `cols` (at most 12): radix = codes + 1 for NULL; a span of 2^63 combinations or more is refused under `entry`'s name
KeySpec key_spec(const rgbm_table& t, const int32_t* cols, int ncols, const char* entry, unsigned __int128* span_out);
// slots of an open-addressing table for n rows: a power of two, at least 1024 and twice the keys there can be (n, or `span` if smaller)
unsigned long long table_capacity(long long n, unsigned __int128 span = ~(unsigned __int128)0);
// appends the first nbits bits of `src` to `words` as whole 64-bit words, the bits beyond them cleared; returns the offset, *n_words the count
long long append_bitset(std::vector<unsigned long long>& words, const uint64_t* src, long long nbits, int32_t* n_words);
void check_cols(const rgbm_table& t, const int32_t* cols, int n, const char* what);
// the RGBM_ERR_ARG refusals of the detectors' column lists (check_cols throws, which gives RGBM_ERR_PARAM): every column inside the table;
// `once`: none listed twice; `bitsets`: each with one.  RGBM_OK or the refusal.
int refuse_cols(const rgbm_table& t, const int32_t* cols, int n, bool once, const uint64_t* const* bitsets, const char* entry);

// string pool offsets: start at 0, never decrease (every read of the distance kernels stays inside [0, off[n]))
void check_pool_offsets(const int64_t* off, int64_t n, const int32_t* cp, const char* entry, const char* which);

// Levenshtein matrix [n_a][n_b] of two checked, non-empty string pools (host memory) into `d_dist` (device memory); the pools and
// the scratch of the long pairs live until the kernels are done (the stream is synchronised before returning).  Defined in rgbm_pmf.hip.
void edit_distance_on_device(const int32_t* a_cp, const int64_t* a_off, int64_t n_a, const int32_t* b_cp, const int64_t* b_off, int64_t n_b,
                             int32_t* d_dist, hipStream_t s);

}  // namespace rgh
