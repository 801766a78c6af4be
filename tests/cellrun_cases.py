"""The cases of tests/test_cellrun_gpu.py and the ONE driver that walks a table through them, shared with tests/test_cellrun_cpu.py (which
holds every generator to its purpose on the restatement alone) -- no device, no code of the product.  `drive` runs the same calls on any
table with the cell set's methods and returns what each call gave, so the device table and tests/cellrun_restatement.CellrunTable are
compared record by record."""
import numpy as np

C, K = 17, 6
PROWS = 4096                                                   # rows per compaction block (asserted against the source by the GPU file)
SIZES = [1, 63, 64, 65, PROWS - 1, PROWS, PROWS + 1, 2 * PROWS + 1]
# sets of 1, 2, 16 and all 17 columns in non-ascending order; each holds the pruned target (column 1)
SETS = {"one": [1], "two": [2, 1], "sixteen": [16, 0, 15, 1, 14, 2, 13, 3, 12, 4, 11, 5, 10, 6, 9, 7],
        "all": [8, 16, 0, 15, 1, 14, 2, 13, 3, 12, 4, 11, 5, 10, 6, 9, 7]}
BETA = 0.5


def table(n, seed=0, noise=0.1):
    """C columns of K codes.  Column 0 = a, column 1 = a % 3 and column 2 = a // 2 but for `noise` of the rows (and NULL in a few): the
    cell domain of a consistent row's cell in column 1 or 2 has its current value on top (a weak label), that of a noisy row has not.
    The other columns are random with NULLs.  Returns (codes, n_codes, dict(flip1, flip2): the noisy rows)."""
    rng = np.random.default_rng(seed * 977 + n)
    codes = rng.integers(0, K, (C, n)).astype(np.int32)
    codes[rng.random((C, n)) < 0.2] = -1
    a = rng.integers(0, 6, n).astype(np.int32)
    codes[0], codes[1], codes[2] = a, a % 3, a // 2
    flip1, flip2 = rng.random(n) < noise, rng.random(n) < noise
    codes[1, flip1] = (codes[1, flip1] + 1) % 3
    codes[2, flip2] = (codes[2, flip2] + 1) % 3
    codes[[5, 9], 0] = -1                                      # a NULL for the detector part of `generic_case`, whatever the size
    null1 = rng.random(n) < 0.03
    codes[1, null1] = -1
    return codes, np.full(C, K, np.int32), dict(flip1=flip1 | null1, flip2=flip2)


def given_cells(n, set_cols, seed=0, m=200):
    """Host-given cells as a user would never send them: shuffled, with duplicates, with rows outside the table (-1, n, n + 7) and columns
    outside the set or the table, and with the first-row and the last-row cell of the set's first and last column."""
    rng = np.random.default_rng(seed + 5 * n)
    rows = rng.integers(0, n, m).astype(np.int64)
    cols = rng.integers(0, C, m).astype(np.int32)
    edge_r = np.array([0, n - 1, 0, n - 1, -1, n, n + 7, 0, n - 1], np.int64)
    edge_c = np.array([set_cols[0], set_cols[0], set_cols[-1], set_cols[-1], set_cols[0], set_cols[0], set_cols[-1], -1, C], np.int32)
    rows, cols = np.concatenate([rows, edge_r, rows[:m // 2]]), np.concatenate([cols, edge_c, cols[:m // 2]])
    order = rng.permutation(len(rows))
    return rows[order], cols[order]


def domain_args(target, attrs, n, single_ok=None, min_cnt=None):
    """What `pair_counts` and `cellset_drop_weak` / `cell_domains` take for one target: the target on the y side of even pairs, on the x
    side of odd ones."""
    pairs = [(int(a), int(target)) if j % 2 == 0 else (int(target), int(a)) for j, a in enumerate(attrs)]
    return dict(target=int(target), pairs=pairs, min_cnt=list(min_cnt) if min_cnt is not None else [0] * len(attrs),
                single_ok=np.ones(K, np.uint8) if single_ok is None else np.asarray(single_ok, np.uint8), beta=BETA, row_count=int(n))


def generic_case(n, which, seed=0):
    """Every entry once on an n-row table and the set `which`: NULL cells of columns inside and outside the set from a detector, then the
    given cells, then (from 64 rows on) the pruning of column 1 on two attributes, the null-out and the rows."""
    codes, n_codes, _ = table(n, seed)
    set_cols = SETS[which]
    ok = np.ones(K, np.uint8)
    ok[4] = 0
    return dict(codes=codes, n_codes=n_codes, set_cols=set_cols, null_parts=[[1, 5, 9]], given=[given_cells(n, set_cols, seed)],
                prune=[domain_args(1, [0, 3], n, single_ok=ok, min_cnt=[0, 1])] if n >= 64 else [])


PRUNE_N = 2 * PROWS + 1
PRUNE_KINDS = ("some_weak", "two_in_one_word", "first_and_last_word", "all_weak", "none_weak", "several_targets")


def prune_case(kind, n=PRUNE_N, seed=3):
    """The pruning cases: the cells are GIVEN, chosen among the consistent rows (weak labels) and the noisy ones (not weak).  `expect`
    {target: 'some' | 'all' | 'none'} and `weak_rows` {target: rows that must be pruned} say what the case is for."""
    codes, n_codes, info = table(n, seed)
    good1, bad1 = np.flatnonzero(~info["flip1"]), np.flatnonzero(info["flip1"])
    good2, bad2 = np.flatnonzero(~info["flip2"]), np.flatnonzero(info["flip2"])
    set_cols, targets, weak_rows = [2, 1], [1], {}
    if kind == "some_weak":
        rows, expect = np.concatenate([good1[::7], bad1[::3]]), {1: "some"}
    elif kind == "two_in_one_word":
        w = next(w for w in range(2, n // 64) if (~info["flip1"][64 * w:64 * w + 64]).sum() >= 2 and info["flip1"][64 * w:64 * w + 64].any())
        inside = np.arange(64 * w, 64 * w + 64)
        rows, expect = inside, {1: "some"}                     # a whole word of cells: the weak ones among them share it
        weak_rows[1] = inside[~info["flip1"][inside]][:2]
    elif kind == "first_and_last_word":
        codes[1, [0, n - 1]] = codes[0, [0, n - 1]] % 3        # both consistent
        rows, expect = np.concatenate([[0, n - 1], bad1[:5]]), {1: "some"}
        weak_rows[1] = np.array([0, n - 1])
    elif kind == "all_weak":
        rows, expect = good1[::5], {1: "all"}
    elif kind == "none_weak":
        rows, expect = bad1, {1: "none"}
    elif kind == "several_targets":
        rows, expect, targets = np.concatenate([good1[::11], bad1[::2]]), {1: "some", 2: "some"}, [1, 2]
    else:
        raise KeyError(kind)
    rows = np.asarray(rows, np.int64)
    given = [(rows, np.full(len(rows), 1, np.int32))]
    if 2 in targets:
        rows2 = np.concatenate([good2[::13], bad2[::2]]).astype(np.int64)
        given.append((rows2, np.full(len(rows2), 2, np.int32)))
    return dict(codes=codes, n_codes=n_codes, set_cols=set_cols, null_parts=[], given=given, expect=expect, weak_rows=weak_rows,
                prune=[domain_args(t, [0], n) for t in targets])


def rows_case(kind, n=PRUNE_N):
    """`cellset_rows`: an empty set, every row, and rows at the block edges (the last row of a block and the first of the next, in
    different columns, and a row two columns share)."""
    codes, n_codes, _ = table(n, 1)
    set_cols = [9, 2, 5]
    if kind == "empty":
        given = []
    elif kind == "every_row":
        half = np.arange(n, dtype=np.int64)
        given = [(half[::2], np.full(len(half[::2]), 9, np.int32)), (half[1::2], np.full(len(half[1::2]), 5, np.int32)), (half[::3], np.full(len(half[::3]), 2, np.int32))]
    elif kind == "block_edges":
        r = np.array([0, 63, 64, PROWS - 1, PROWS, PROWS, 2 * PROWS - 1, 2 * PROWS, n - 1], np.int64)
        given = [(r, np.array([9, 2, 5, 9, 2, 5, 5, 9, 2], np.int32))]
    else:
        raise KeyError(kind)
    return dict(codes=codes, n_codes=n_codes, set_cols=set_cols, null_parts=[], given=given, prune=[])


def many_blocks_case(n=200003):
    """Three overlapping detectors (NULLs, a code predicate, a functional dependency), given cells and the pruning of two targets."""
    codes, n_codes, info = table(n, 11, noise=0.02)
    codes[3] = np.random.default_rng(12).integers(0, K, n)
    bad = np.flatnonzero(info["flip1"])
    given = [(np.concatenate([bad[::2], np.arange(0, n, 101)]).astype(np.int64), None)]
    given[0] = (given[0][0], np.full(len(given[0][0]), 1, np.int32))
    return dict(codes=codes, n_codes=n_codes, set_cols=[4, 2, 1], null_parts=[[1, 2, 3]],
                cell_parts=[([2, 4], [1, 0], [0, 3], [-1, 4], None)], constraint_parts=[([0], 1, [1, 2])],
                given=given, prune=[domain_args(1, [0], n), domain_args(2, [0], n)])


def drive(tab, case):
    """The whole sequence on `tab` (the device table or the restated one); returns [(what, value)] in call order."""
    out = []
    n_bins = {j: K for j in range(C)}

    def emit(what):
        got = tab.cellset_emit()
        out.extend((what + "." + k, v) for k, v in zip(("rows", "cols", "codes", "counts"), got))
        return got

    tab.cellset_open(case["set_cols"])
    for cols in case.get("null_parts", ()):
        out.append(("nulls", tab.detect_nulls(cols, fetch=False)))
        tab.cellset_add()
    for cols, null, lo, hi, bits in case.get("cell_parts", ()):
        out.append(("cells", tab.detect_cells(cols, null, lo, hi, bits, fetch=False)))
        tab.cellset_add()
    for eq, iq, cc in case.get("constraint_parts", ()):
        out.append(("constraint", tab.detect_constraint(eq, iq, cell_cols=cc, fetch=False)))
        tab.cellset_add()
    detected = emit("detected")
    tab.cellset_add_cells(np.zeros(0, np.int64), np.zeros(0, np.int32))          # empty input adds nothing ...
    out.append(("cell list after the empty add", tab._fetch_cells(len(detected[0]), True)[0]))     # ... and the cell list stays
    emit("after the empty add")
    for rows, cols in case["given"]:
        tab.cellset_add_cells(rows, cols)
    emit("with the given cells")
    if case["prune"]:
        pairs = [p for d in case["prune"] for p in d["pairs"]]
        tab.pair_counts(pairs, n_bins=n_bins)
        at = 0
        for d in case["prune"]:
            pidx = list(range(at, at + len(d["pairs"])))
            at += len(d["pairs"])
            cells, weak = tab.cellset_drop_weak(d["target"], pidx, d["min_cnt"], d["single_ok"], d["beta"], d["row_count"])
            rows, cols = tab._fetch_cells(cells, True)             # the examined cells, as after a detect call
            flags = tab.cell_domains(d["target"], rows, pidx, d["min_cnt"], d["single_ok"], d["beta"], d["row_count"])[0]
            out += [("drop_weak %d.cells" % d["target"], cells), ("drop_weak %d.weak" % d["target"], weak),
                    ("drop_weak %d.rows" % d["target"], rows), ("drop_weak %d.cols" % d["target"], cols),
                    ("drop_weak %d.flags of cell_domains" % d["target"], np.asarray(flags, np.uint8))]
            emit("after drop_weak %d" % d["target"])
    out.append(("null.cells", tab.cellset_null()))
    out.append(("null.table", np.stack([tab.read_column(j) for j in range(tab.c)])))
    emit("after null")
    out.append(("rows", tab.cellset_rows()))
    out.append(("rows.count", tab.cellset_rows(fetch=False)))
    tab.cellset_close()
    return out


def same(got, want):
    """Record by record: names, dtypes of arrays, values."""
    assert [k for k, _ in got] == [k for k, _ in want]
    for (k, g), (_, w) in zip(got, want):
        if isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k
        else:
            assert g == w, (k, g, w)


def purpose(case, rec):
    """What a record of `drive` must show for the case to be worth running."""
    rec = dict(rec)
    for t, expect in case.get("expect", {}).items():
        cells, weak = rec["drop_weak %d.cells" % t], rec["drop_weak %d.weak" % t]
        flags = rec["drop_weak %d.flags of cell_domains" % t]
        assert cells > 0 and weak == int(flags.sum())
        assert {"some": 0 < weak < cells, "all": weak == cells, "none": weak == 0}[expect], (t, expect, weak, cells)
        rows = rec["drop_weak %d.rows" % t]
        for r in case.get("weak_rows", {}).get(t, ()):
            assert flags[np.searchsorted(rows, r)] == 1 and rows[np.searchsorted(rows, r)] == r, (t, r)
