"""The cases of `rgbm_table_recode` (tests/test_fitted_cpu.py holds `repair.recode_codes.recode` to a plain restatement on them,
tests/test_fitted_gpu.py the device entry to that statement; tests/test_fitted_gpu_guarded.py runs the small ones once more under guard zones).

A case is dict(codes [C][n] int32, n_codes, luts, n_codes_out, routes): `routes` is what `Table.recode_report()` must say -- 0 identity,
1 a LUT of at most RECODE_LDS_CODES entries (staged in LDS), 2 a larger one (gathered from global memory) -- with the constant read from
the source.  Rows 1 .. 1025 cross the kernel's cuts: the 16-byte head and tail of a column (n % 4 != 0 with two or more columns gives
unaligned column bases), one wave, one workgroup's step of 2 x 256 int4, more than one step.  The LUT sizes sit on both sides of the LDS
limit, the contents are all -1, a permutation, many-to-one, and the input holds -1, -7, n_codes, n_codes + 5 and INT32_MAX."""
import numpy as np

from tests.helpers import csrc_constant

ROWS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
COLS = [1, 2, 3, 17]
GUARDED_ROWS = 257          # the cases up to here run once more under guard zones
INT32_MAX = 2 ** 31 - 1


def lds_codes():
    return csrc_constant("RECODE_LDS_CODES")


def _lut(rng, n_in, n_out, kind):
    if kind == 0:
        return np.full(n_in, -1, np.int32)                               # nothing survives
    if kind == 1:                                                        # a permutation of what fits, -1 beyond it
        lut = np.full(n_in, -1, np.int32)
        m = min(n_in, n_out)
        lut[rng.permutation(n_in)[:m]] = rng.permutation(n_out)[:m].astype(np.int32)
        return lut
    return rng.integers(-1, max(n_out // 3, 1), n_in).astype(np.int32)   # many-to-one, with holes


def make_case(n, sizes, seed, n_out=None):
    """sizes[j]: the dictionary size of column j, negative = an identity column of -sizes[j] codes.  n_out[j]: output size of a LUT column
    (default: cycles through 1, the input size, twice the input size)."""
    rng = np.random.default_rng(seed)
    L = lds_codes()
    C = len(sizes)
    codes = np.zeros((C, n), np.int32)
    n_codes, luts, n_codes_out, routes = [], [], [], []
    for j, s in enumerate(sizes):
        k = abs(int(s))
        v = rng.integers(-1, k, n).astype(np.int32)
        special = np.array([-1, -7, k, k + 5, INT32_MAX, k - 1, 0], np.int32)
        at = rng.permutation(n)[:len(special)]
        v[at] = special[:len(at)]
        codes[j] = v
        n_codes.append(k)
        if s < 0:
            luts.append(None); n_codes_out.append(k); routes.append(0)
        else:
            ko = int(n_out[j]) if n_out is not None else (1, k, 2 * k)[(seed + j) % 3]
            luts.append(_lut(rng, k, ko, (seed + j) % 3)); n_codes_out.append(ko); routes.append(1 if k <= L else 2)
    return dict(codes=codes, n_codes=np.asarray(n_codes, np.int32), luts=luts, n_codes_out=np.asarray(n_codes_out, np.int32), routes=routes)


def edge_sizes():
    L = lds_codes()
    return [1, 2, L - 1, L, L + 1]


def case_ids():
    return ["r%dc%d" % (n, c) for n in ROWS for c in COLS] + ["identity_between_luts", "all_identity", "n_codes_out_1"]


def case(cid):
    """The case of an id of `case_ids()` (made on demand: 55 cases of up to 17 x 1025 cells and LUTs of up to RECODE_LDS_CODES + 1 entries)."""
    E = edge_sizes()
    if cid == "identity_between_luts":
        return make_case(1025, [E[3], -E[4], E[4]], 901)
    if cid == "all_identity":
        return make_case(259, [-3, -E[2]], 902)
    if cid == "n_codes_out_1":
        return make_case(1023, [2, E[2], E[4]], 903, n_out=[1, 1, 1])
    n, c = (int(x) for x in cid[1:].split("c"))
    k = ROWS.index(n) * len(COLS) + COLS.index(c)
    # every column takes the next edge size; every fifth column of the wide cases is an identity column
    sizes = [(-E[(k + j) % 5] if (c >= 3 and j % 5 == 1) else E[(k + j) % 5]) for j in range(c)]
    return make_case(n, sizes, 100 + k)


def big_case():
    """One 200 003 x 6 table (n % 4 == 3: every column base but the first is unaligned) with a column of more than 100 000 codes."""
    L = lds_codes()
    return make_case(200003, [L, 100003, -7, 2, L + 1, 31], 77)
