"""ctypes binding of librepairgbm.so (include/rgbm.h) -- the only door to the HIP engine.

There is deliberately no fallback: if the shared library is missing or no HIP device is usable
the calls raise ``RepairGbmError`` (the caller in train.py turns a failed build into
``PoorModel(None)`` exactly like the reference does, python/repair/train.py:227-229).

The C signature of every entry point is written down once, in ``SIGNATURES`` below; ``lib()`` hands it to ctypes, which converts and
checks the arguments of every call.  A new entry point is declared in include/rgbm.h and in that table, nowhere else.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "..", "lib", "librepairgbm.so")


class RepairGbmError(RuntimeError):
    pass


class RgbmParams(C.Structure):
    _fields_ = [
        ("objective", C.c_int32), ("num_class", C.c_int32),
        ("n_estimators", C.c_int32), ("num_leaves", C.c_int32), ("max_depth", C.c_int32), ("max_bin", C.c_int32),
        ("min_data_in_leaf", C.c_int32), ("min_data_in_bin", C.c_int32), ("bagging_freq", C.c_int32), ("seed", C.c_int32),
        ("device_id", C.c_int32), ("reserved", C.c_int32),
        ("learning_rate", C.c_double), ("lambda_l1", C.c_double), ("lambda_l2", C.c_double), ("min_gain_to_split", C.c_double),
        ("min_sum_hessian_in_leaf", C.c_double), ("bagging_fraction", C.c_double), ("feature_fraction", C.c_double),
    ]


class RgbmTrainStats(C.Structure):
    _fields_ = [
        ("hist_ms", C.c_double), ("total_ms", C.c_double), ("hist_launches", C.c_int64), ("hist_rows", C.c_int64),
        ("hist_bytes", C.c_int64), ("root_rows", C.c_int64), ("root_ms", C.c_double), ("trees", C.c_int64),
        ("route_ms", C.c_double), ("route_launches", C.c_int64), ("root_atomics_per_row", C.c_int64), ("level_atomics_per_row", C.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RgbmFitSpec(C.Structure):
    _fields_ = [("table", C.c_void_p), ("target_col", C.c_int32), ("n_features", C.c_int32), ("feat_cols", C.POINTER(C.c_int32)),
                ("y_value", C.POINTER(C.c_double)), ("class_weight", C.POINTER(C.c_double)), ("params", C.POINTER(RgbmParams)),
                ("valid_table", C.c_void_p), ("valid_label_out", C.POINTER(C.c_int32)), ("valid_value_out", C.POINTER(C.c_double))]


class DcPred(C.Structure):
    """``rgbm_dc_pred`` of include/rgbm.h."""
    _fields_ = [("op", C.c_int32), ("left_col", C.c_int32), ("right_col", C.c_int32), ("reserved", C.c_int32),
                ("left_rank", C.POINTER(C.c_int32)), ("right_rank", C.POINTER(C.c_int32))]


class RxSeg(C.Structure):
    """``rgbm_rx_seg`` of include/rgbm.h."""
    _fields_ = [("kind", C.c_int32), ("min", C.c_int32), ("max", C.c_int32), ("cls", C.c_uint32 * 4), ("const_off", C.c_int32),
                ("const_len", C.c_int32)]


PARAM_DEFAULTS = dict(objective=1, num_class=2, n_estimators=300, num_leaves=31, max_depth=7, max_bin=255,
                      min_data_in_leaf=20, min_data_in_bin=3, bagging_freq=0, seed=42, device_id=0, reserved=0,
                      learning_rate=0.01, lambda_l1=0.0, lambda_l2=0.0, min_gain_to_split=0.0,
                      min_sum_hessian_in_leaf=1e-3, bagging_fraction=1.0, feature_fraction=1.0)


FLAG_ROW_SHARDED = 1
FLAG_NO_MODEL = 2
FLAG_WHOLE_TABLE = 4
VIEW_STATES = ("none", "built", "not worth it", "cannot")


def make_params(**kw):
    d = dict(PARAM_DEFAULTS)
    kw = dict(kw)
    if kw.pop("row_sharded", False):
        d["reserved"] = d.get("reserved", 0) | FLAG_ROW_SHARDED
    if kw.pop("whole_table", False):
        d["reserved"] = d.get("reserved", 0) | FLAG_WHOLE_TABLE
    if not kw.pop("want_model", True):
        d["reserved"] = d.get("reserved", 0) | FLAG_NO_MODEL
    for k, v in kw.items():
        if k not in d:
            raise TypeError("unknown parameter %r" % k)
        d[k] = v
    return RgbmParams(**d)


# ---- the C signatures of include/rgbm.h (tests/test_abi_signatures.py holds this table to the header, type by type).
# H: an opaque handle (rgbm_table*, rgbm_model*, a group) or any void*;  HP: where a handle is returned, or an array of handles.
INT, I32, I64, F64, SIZE, H = C.c_int, C.c_int32, C.c_int64, C.c_double, C.c_size_t, C.c_void_p
I32P, I64P, F64P, U8P, U64P, SIZEP, HP = (C.POINTER(t) for t in (I32, I64, F64, C.c_uint8, C.c_uint64, SIZE, H))
I32PP, U64PP = C.POINTER(I32P), C.POINTER(U64P)                         # const int32_t* const*, const uint64_t* const*
PARAMS, STATS, FITS, PREDS, SEGS = (C.POINTER(t) for t in (RgbmParams, RgbmTrainStats, RgbmFitSpec, DcPred, RxSeg))

SIGNATURES = {        # name: (restype, argtypes), in the order of the header
    "rgbm_device_count": (INT, ()),
    "rgbm_release_cache": (INT, ()),
    "rgbm_last_error": (C.c_char_p, ()),
    "rgbm_version": (INT, ()),
    "rgbm_train": (INT, (I32P, I64, I32, I32P, I32P, I32, F64P, F64P, F64P, PARAMS, HP, STATS)),
    "rgbm_predict": (INT, (H, I32P, I64, I32, I32, F64P)),
    "rgbm_repair_chain": (INT, (HP, I32, I32P, I32P, I32P, I32P, I32P, I32P, I64, I32, I32, I32P, F64P)),
    "rgbm_table_create": (INT, (I32P, I64, I32, I32P, I32, HP)),
    "rgbm_table_set_column_kind": (INT, (H, I32, I32)),
    "rgbm_table_set_column_values": (INT, (H, I32, F64P, I32)),
    "rgbm_host_alloc": (INT, (SIZE, HP)),
    "rgbm_host_free": (None, (H,)),
    "rgbm_table_free": (None, (H,)),
    "rgbm_table_train": (INT, (H, I32, I32P, I32, F64P, F64P, PARAMS, HP, STATS)),
    "rgbm_table_set_row_multiplicity": (INT, (H, U8P)),
    "rgbm_table_read_row_multiplicity": (INT, (H, U8P)),
    "rgbm_table_distinct_rows": (INT, (H, HP, I64P, I64P)),
    "rgbm_table_distinct_view_info": (INT, (H, I32P, I64P, I64P)),
    "rgbm_distinct_view_eligible": (INT, (I64, I32, PARAMS, I32, I64)),
    "rgbm_table_train_batch": (INT, (FITS, I32, HP, I32P)),
    "rgbm_table_train_batch_report": (INT, (I32P, I32)),
    "rgbm_table_repair_chain": (INT, (H, HP, I32, I32P, I32P, I32P, I64, I64, I32P, F64P)),
    "rgbm_table_read_column": (INT, (H, I32, I32P)),
    "rgbm_table_detect_nulls": (INT, (H, I32P, I32, I64P)),
    "rgbm_table_detect_cells": (INT, (H, I32P, I32, U8P, I32P, I32P, U64PP, I64P)),
    "rgbm_table_detect_constraint": (INT, (H, I32P, I32, I32, I32P, I32, I64P, I64P)),
    "rgbm_table_detect_dc": (INT, (H, PREDS, I32, I32P, I32, I64, I64P, I64P)),
    "rgbm_table_detect_dc_scan": (INT, (H, PREDS, I32, I32P, I32, I64P, I64P)),
    "rgbm_table_detect_row_bits": (INT, (H, I32P, I32, U64PP, I32P, I32, I64P, I64P)),
    "rgbm_table_rows_of_cells": (INT, (H, I64P, I64, I64P)),
    "rgbm_table_cells_fetch": (INT, (H, I64P, I32P)),
    "rgbm_table_cellset_open": (INT, (H, I32P, I32)),
    "rgbm_table_cellset_add": (INT, (H,)),
    "rgbm_table_cellset_emit": (INT, (H, I64P, I64P)),
    "rgbm_table_cells_fetch_codes": (INT, (H, I32P)),
    "rgbm_table_cellset_close": (INT, (H,)),
    "rgbm_table_cellset_add_cells": (INT, (H, I64P, I32P, I64)),
    "rgbm_table_cellset_drop_weak": (INT, (H, I32, I32P, I32, I64P, U8P, F64, I64, I64P, I64P)),
    "rgbm_table_cellset_null": (INT, (H, I64P)),
    "rgbm_table_cellset_rows": (INT, (H, I64P)),
    "rgbm_table_null_cells": (INT, (H, I64P, I32P, I64, I32P, I32)),
    "rgbm_table_read_cells": (INT, (H, I64P, I32P, I64, I32P)),
    "rgbm_table_write_cells": (INT, (H, I64P, I32P, I32P, I64)),
    "rgbm_table_gather_rows": (INT, (H, I64P, I64, HP)),
    "rgbm_table_concat": (INT, (HP, I32, HP)),
    "rgbm_table_smoten": (INT, (H, I32, I32P, I32, I64P, I64, I32, I32P, I32, I64P, I64P, I64P, HP)),
    "rgbm_table_count_codes": (INT, (H, I32, I64P, I64P)),
    "rgbm_table_column_stats": (INT, (H, I32P, I32, I32PP, I32, I64P, I32P)),
    "rgbm_table_fd_measures": (INT, (H, I32P, I32, I32P, I32, I64P, I64P, I64P, I64P)),
    "rgbm_table_fd_measures_report": (INT, (H, I32P, I32)),
    "rgbm_table_recode": (INT, (H, I32PP, I32P, HP, I64P)),
    "rgbm_table_recode_report": (INT, (H, I32P, I32)),
    "rgbm_table_create_dict": (INT, (I32P, I64, I32, I32PP, I32P, I32, HP)),
    "rgbm_table_repair_pmf": (INT, (H, H, I32, I32P, I32, I32, F64, I32P, I64, I64P, I64P, I32P, F64P, F64P)),
    "rgbm_table_repair_pmf_weighted": (INT, (H, H, I32, I32P, I32, I32, F64, I32P, I32P, F64P, I64, F64, I32, I64, I64P, I64P, I32P, F64P,
                                             F64P, F64P)),
    "rgbm_edit_distance": (INT, (I32, I32P, I64P, I64, I32P, I64P, I64, I32P)),
    "rgbm_table_pair_counts": (INT, (H, I32P, I32, I32PP, I32P, I64P)),
    "rgbm_table_pair_counts_report": (INT, (H, I64P, I32P, I32)),
    "rgbm_table_cell_domains": (INT, (H, I32, I64P, I64, I32P, I32, I64P, U8P, F64, I64, U8P, I32P, F64P, F64P)),
    "rgbm_table_fd_map": (INT, (H, I32, I32, I32P)),
    "rgbm_table_rule_fill": (INT, (H, I32, I32, I32P, I32, I64, I64, I32P)),
    "rgbm_nearest_values": (INT, (I32, I32P, I64P, I64, I32P, I64P, I64, F64P, F64, I32P)),
    "rgbm_regex_structure": (INT, (I32, SEGS, I32, I32, I32P, I32, I32P, I64P, I64, U8P, I64P, I32P, I64P)),
    "rgbm_lof_1d": (INT, (I32, F64P, I64P, I32, I32, F64, F64P, U64P, I64P)),
    "rgbm_table_kmeans_assign": (INT, (H, I32P, I32, I64P, I32, F64P, I64, F64P, I32, I64P, I64P, I64P)),
    "rgbm_table_kmeans_bisect": (INT, (H, I32P, I32, I64P, I64, I32P, I32, I32, I32P, F64P, F64P, I32, I64P, I64P, I64P)),
    "rgbm_table_kmeans_read": (INT, (H, I32P)),
    "rgbm_table_shape": (INT, (H, I64P, I32P, I32P)),
    "rgbm_comm_unique_id": (INT, (H,)),
    "rgbm_comm_init": (INT, (H, I32, I32, I32)),
    "rgbm_comm_finalize": (INT, ()),
    "rgbm_comm_info": (INT, (I32P,)),
    "rgbm_comm_count": (INT, (I32P,)),
    "rgbm_comm_all_gather_sizes": (INT, (I64P, I32, I64P)),
    "rgbm_comm_all_gather_bytes": (INT, (H, I64, I64, H)),
    "rgbm_table_repair_chain_gather": (INT, (H, HP, I32, I32P, I32P, I32P, I64, I64, I64, I32P, F64P)),
    "rgbm_comm_gather_stats": (INT, (I64P,)),
    "rgbm_local_group_create": (INT, (I32, I32, HP)),
    "rgbm_local_group_free": (None, (H,)),
    "rgbm_comm_init_local": (INT, (H, I32)),
    "rgbm_fusion_create": (INT, (I32, HP)),
    "rgbm_fusion_join": (INT, (H, I32)),
    "rgbm_fusion_leave": (INT, (I32,)),
    "rgbm_fusion_info": (INT, (H, I64P)),
    "rgbm_fusion_free": (INT, (H,)),
    "rgbm_model_save": (INT, (H, H, SIZEP)),
    "rgbm_model_load": (INT, (H, SIZE, HP)),
    "rgbm_model_free": (None, (H,)),
    "rgbm_model_info": (INT, (H, I32P)),
    "rgbm_model_predict_form": (INT, (H, I32P)),
    "rgbm_level_pass_plan": (INT, (I32P, I32, I64, I32, I32, I32, F64P, I32, I32P)),
    "rgbm_model_importance": (INT, (H, I32, F64P)),
}
EXPORTED_SYMBOLS = list(SIGNATURES)

_lib = None


def lib():
    """Load librepairgbm.so (fails loudly when it has not been built) and give every entry point its signature."""
    global _lib
    if _lib is None:
        path = os.path.abspath(os.environ.get("RGBM_LIB_PATH") or LIB_PATH)   # RGBM_LIB_PATH: A/B runs of differently built libraries
        if not os.path.exists(path):
            raise RepairGbmError("librepairgbm.so is not built (%s); run `python __graft_entry__.py` or `make -C "
                                 "spark-data-repair-plugin_amd/csrc`" % path)
        l = C.CDLL(path)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(l, name, None)           # (an older build under RGBM_LIB_PATH lacks the newer entries: `_call` names the one that is asked for)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _lib = l
    return _lib


def _check(rc, what):
    if rc != 0:
        err = RepairGbmError("%s failed (%d): %s" % (what, rc, lib().rgbm_last_error().decode("utf-8", "replace")))
        err.code = rc                      # the RGBM_ERR_* value of include/rgbm.h
        raise err


def _call(name, *args):
    """Call the entry point ``name`` of ``SIGNATURES`` and raise as `_check` does when it returns an error code.  A numpy array among
    ``args`` goes through `_p` with the element type the table declares for its place; everything else is ctypes' to convert."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RepairGbmError("%s is not exported by %s" % (name, lib()._name))
    args = list(args)
    for i, a in enumerate(args):
        if isinstance(a, np.ndarray):
            args[i] = _p(a, fn.argtypes[i]._type_)
    _check(fn(*args), name)


_DTYPE = {t: np.dtype(t) for t in (C.c_int32, C.c_int64, C.c_double, C.c_uint8, C.c_uint64)}      # (np.dtype(ctype) costs microseconds per call)


def _p(a, t):
    """The array ``a`` as a ``POINTER(t)`` argument (None: NULL).  TypeError for an array of another dtype or one that is not C-contiguous:
    the library would read other numbers than the caller's.  A zero-length array has no address of its own; where NULL means
    something else to the library (a LUT column: identity) the caller passes one element in its place."""
    if a is None:
        return None
    if a.dtype != (_DTYPE.get(t) or np.dtype(t)) or not a.flags.c_contiguous:
        raise TypeError("a C-contiguous %s array expected, not %s%s" % (np.dtype(t), a.dtype, "" if a.flags.c_contiguous else " (not contiguous)"))
    return a.ctypes.data_as(C.POINTER(t))


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, np.float64)


def _flat(a, dtype):
    """``a`` as a C-contiguous 1-d array of ``dtype`` (a copy only where one is needed)."""
    return np.ascontiguousarray(a, dtype).reshape(-1)


COMM_ID_BYTES = 128


def comm_unique_id():
    """128 opaque bytes (an ncclUniqueId) created on one rank; every rank passes them to ``comm_init``."""
    buf = (C.c_ubyte * COMM_ID_BYTES)()
    _call("rgbm_comm_unique_id", buf)
    return bytes(buf)


def comm_init(uid, rank, nranks, device_id=0):
    """RCCL communicator of the calling thread for row-sharded training (include/rgbm.h)."""
    buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(bytes(uid))
    _call("rgbm_comm_init", buf, rank, nranks, device_id)


def comm_finalize():
    _call("rgbm_comm_finalize")


def comm_info():
    a = np.zeros(3, np.int32)
    _call("rgbm_comm_info", a)
    return dict(kind=int(a[0]), rank=int(a[1]), nranks=int(a[2]))


def model_trees(blob):
    """The trees of a serialised model (rgbm_model_save), in (iteration, class tree) order: dicts of the arrays the blob stores -- feat, theta,
    dleft, left, right (child >= 0: internal node, < 0: ~leaf), gain, leaf_value, leaf_count.  Returns (K, n_iter, trees)."""
    import struct
    hdr = struct.unpack_from("7i", blob, 0)
    ver, K, n_iter, F = hdr[1], hdr[4], hdr[5], hdr[6]
    p = 28
    for _ in range(F):
        _, V, _ = struct.unpack_from("3i", blob, p); p += 12 + 4 * V
        if ver == 2:
            nw, = struct.unpack_from("i", blob, p); p += 4 + 4 * nw
    trees = []
    for _ in range(K * n_iter):
        L, = struct.unpack_from("i", blob, p); p += 4
        n = L - 1
        t = {}
        for name in ("feat", "theta", "dleft", "left", "right"):
            t[name] = np.frombuffer(blob, np.int32, n, p); p += 4 * n
        t["gain"] = np.frombuffer(blob, np.float64, n, p); p += 8 * n
        t["leaf_value"] = np.frombuffer(blob, np.float64, L, p); p += 8 * L
        t["leaf_count"] = np.frombuffer(blob, np.int32, L, p); p += 4 * L
        trees.append(t)
    return K, n_iter, trees


def needed_built_rows(blob, max_depth):
    """Rows whose (g, h) the FINISHED trees of a model needed in a histogram below the root: for every split whose children can still be
    split (depth + 1 < max_depth) the rows of its smaller child (LightGBM constructs the smaller leaf and derives the sibling by
    subtraction) -- what a grower that knew the final trees in advance would accumulate.  The level grower expands a superset."""
    _, _, trees = model_trees(blob)
    total = 0
    for tr in trees:
        n = len(tr["feat"])
        if n == 0:
            continue
        left, right, lc = tr["left"], tr["right"], tr["leaf_count"]
        cnt = np.zeros(n, np.int64)
        for j in range(n - 1, -1, -1):          # children have larger indices than their parent (Tree::Split numbering)
            a, b = int(left[j]), int(right[j])
            cnt[j] = (cnt[a] if a >= 0 else int(lc[~a])) + (cnt[b] if b >= 0 else int(lc[~b]))
        depth = np.zeros(n, np.int32)
        for j in range(n):
            a, b = int(left[j]), int(right[j])
            if a >= 0:
                depth[a] = depth[j] + 1
            if b >= 0:
                depth[b] = depth[j] + 1
            if depth[j] + 1 < max_depth:
                ca = cnt[a] if a >= 0 else int(lc[~a]); cb = cnt[b] if b >= 0 else int(lc[~b])
                total += int(min(ca, cb))
    return total


def comm_count():
    """Ranks the calling thread's communicator really spans (ncclCommCount); 1 without a communicator."""
    n = C.c_int32(0)
    _call("rgbm_comm_count", C.byref(n))
    return int(n.value)


def comm_all_gather_sizes(values):
    """Every rank of the calling thread's communicator contributes the int64 vector `values`; returns [nranks][len(values)]."""
    v = _flat(values, np.int64)
    out = np.zeros((max(1, comm_info()["nranks"]), v.size), np.int64)
    _call("rgbm_comm_all_gather_sizes", v, v.size, out)
    return out


def comm_all_gather_bytes(payload):
    """Variable-size all-gather of byte strings over the calling thread's communicator (device buffers + ncclAllGather inside the library:
    include/rgbm.h "C1 / C2"): returns the list of every rank's payload, in rank order."""
    mine = np.frombuffer(bytes(payload), np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
    sizes = comm_all_gather_sizes([mine.size])[:, 0]
    block = int(max(int(sizes.max()), 1))
    recv = np.zeros((len(sizes), block), np.uint8)
    _call("rgbm_comm_all_gather_bytes", _p(mine, C.c_uint8) if mine.size else None, mine.size, block, _p(recv, C.c_uint8))
    return [recv[r, :int(sizes[r])].copy() for r in range(len(sizes))]


def comm_gather_stats():
    a = np.zeros(3, np.int64)
    _call("rgbm_comm_gather_stats", a)
    return dict(bytes=int(a[0]), seconds=float(a[1]) * 1e-9, collectives=int(a[2]))


class FusionGroup:
    """The row-sharded training calls this rank makes AT THE SAME TIME (include/rgbm.h "Fusion group"): created on the thread that holds
    the rank's communicator, which moves into the group until ``close()``.  Every member thread runs ``with group.member(j): ...`` around its
    ``Table.train(..., row_sharded=True)`` calls (the same j on every rank); the i-th collective of all members is one all-reduce."""

    def __init__(self, n_members):
        self.h = C.c_void_p()
        _call("rgbm_fusion_create", n_members, C.byref(self.h))
        self.n_members = n_members

    class _Member:
        def __init__(self, group, j):
            self.group, self.j = group, j

        def __enter__(self):
            _call("rgbm_fusion_join", self.group.h, self.j)
            return self

        def __exit__(self, et, ev, tb):
            lib().rgbm_fusion_leave(0 if et is None else 1)
            return False

    def member(self, j):
        return FusionGroup._Member(self, j)

    def info(self):
        a = np.zeros(4, np.int64)
        _call("rgbm_fusion_info", self.h, a)
        return dict(collectives=int(a[0]), parts=int(a[1]), members_in=int(a[2]), broken=bool(a[3]))

    def close(self):
        """Hands the communicator back to the calling thread (call it on the thread that created the group, after every member left)."""
        if self.h:
            _call("rgbm_fusion_free", self.h)
            self.h = C.c_void_p()


class LocalGroup:
    """Test transport: ``nranks`` host threads of this process act as the ranks of a row-sharded job on one device."""

    def __init__(self, nranks, device_id=0):
        self.h = C.c_void_p()
        _call("rgbm_local_group_create", nranks, device_id, C.byref(self.h))
        self.nranks = nranks

    def join(self, rank):
        """Call from the thread that plays ``rank``; pair with ``comm_finalize()`` in the same thread."""
        _call("rgbm_comm_init_local", self.h, rank)

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h and _lib is not None:
            _lib.rgbm_local_group_free(h)


def device_count():
    return int(lib().rgbm_device_count())


def release_cache():
    """Return the device blocks parked in the library's caching pool to the driver (include/rgbm.h)."""
    _call("rgbm_release_cache")


class Model:
    """Owning handle of an ``rgbm_model`` (host-resident trees; device mirrors are lazy)."""

    def __init__(self, handle):
        self.h = handle

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h and _lib is not None:
            _lib.rgbm_model_free(h)

    def info(self):
        a = np.zeros(5, np.int32)
        _call("rgbm_model_info", self.h, a)
        return dict(objective=int(a[0]), num_class=int(a[1]), K=int(a[2]), n_iter=int(a[3]), F=int(a[4]))

    def save(self):
        n = C.c_size_t(0)
        _call("rgbm_model_save", self.h, None, C.byref(n))
        buf = bytearray(max(n.value, 1))
        _call("rgbm_model_save", self.h, (C.c_char * len(buf)).from_buffer(buf), C.byref(n))
        return bytes(buf[:n.value]) if n.value != len(buf) else bytes(buf)

    @staticmethod
    def load(b):
        h = C.c_void_p()
        arr = np.frombuffer(b, np.uint8)
        _call("rgbm_model_load", arr.ctypes.data_as(C.c_void_p), len(b), C.byref(h))
        return Model(h)

    def importance(self, kind="gain"):
        out = np.zeros(self.info()["F"], np.float64)
        _call("rgbm_model_importance", self.h, 0 if kind == "split" else 1, out)
        return out

    def predict_form(self):
        """The kernel the predictor runs for this model (rgbm_model_predict_form; needs no device): form "fixed" | "dynamic" | "walk",
        MW mask words per table entry, TW padded mask words per tree (fixed form), tb trees per LDS stage, lds bytes per workgroup."""
        a = np.zeros(5, np.int32)
        _call("rgbm_model_predict_form", self.h, a)
        return dict(form=("fixed", "dynamic", "walk")[int(a[0])], MW=int(a[1]), TW=int(a[2]), tb=int(a[3]), lds=int(a[4]))

    def predict(self, X, device_id=0):
        """X: [F][n] int32 codes (column-major). Returns [n][ncol] float64 (regression: [n][1])."""
        X = _i32(X)
        F, n = X.shape
        inf = self.info()
        ncol = 1 if inf["objective"] == 2 else inf["num_class"]
        out = np.zeros((n, ncol), np.float64)
        _call("rgbm_predict", self.h, X, n, F, device_id, out)
        return out


def train(X, n_codes, y_code, n_y_codes, y_value=None, class_weight=None, sample_weight=None, want_stats=False, **params):
    """Fit one model from host arrays. X: [F][N] int32 column-major codes."""
    X = _i32(X)
    F, N = X.shape
    n_codes, y_code = _i32(n_codes), _i32(y_code)
    yv, cw, sw = _f64(y_value), _f64(class_weight), _f64(sample_weight)
    p = make_params(**params)
    h = C.c_void_p()
    st = RgbmTrainStats()
    _call("rgbm_train", X, N, F, n_codes, y_code, n_y_codes, yv, cw, sw, C.byref(p), C.byref(h), C.byref(st) if want_stats else None)
    m = Model(h)
    return (m, st.as_dict()) if want_stats else m


def level_pass_plan(nbins, rows, K, max_depth=7, with_mult=False):
    """The launch plan of the level grower's passes for a table shape (rgbm_level_pass_plan; no device needed; honours the RGBM_* switches of the
    environment): dict(root_gx, part_items, root_workgroups, root_t_fix_us, root_t_rows_us, launches=[dict(level, ch, slot0, nslots, route, T, G, gx,
    acc2, rot, t_fix_us, t_rows_us)]) -- t_fix_us / t_rows_us: the modelled fixed and row-loop time of one workgroup the grid rule ranks by."""
    nb = _i32(nbins)
    out = np.zeros(6 + 12 * 4096, np.float64)      # (<= 6 levels x 16 chunks x 32 windows of built slots)
    n = C.c_int32(0)
    _call("rgbm_level_pass_plan", nb, len(nb), rows, K, max_depth, 1 if with_mult else 0, out, len(out), C.byref(n))
    keys = ("level", "ch", "slot0", "nslots", "route", "T", "G", "gx", "acc2", "rot")
    launches = []
    for i in range(int(out[2])):
        v = out[6 + 12 * i: 18 + 12 * i]
        launches.append(dict({k: int(x) for k, x in zip(keys, v)}, t_fix_us=float(v[10]), t_rows_us=float(v[11])))
    return dict(root_gx=int(out[0]), part_items=int(out[1]), root_workgroups=int(out[3]), root_t_fix_us=float(out[4]), root_t_rows_us=float(out[5]), launches=launches)


def distinct_view_eligible(rows, f, table_has_mult=False, min_rows=0, **params):
    """Whether a Table.train of this shape MAY use the table's distinct-row view (rgbm_distinct_view_eligible; no device needed)."""
    p = make_params(**params)
    r = lib().rgbm_distinct_view_eligible(rows, f, C.byref(p), 1 if table_has_mult else 0, min_rows)
    if r < 0:
        _check(r, "rgbm_distinct_view_eligible")
    return bool(r)


def train_batch(fits):
    """Many fits in one go (include/rgbm.h rgbm_table_train_batch): ``fits`` is a list of dicts with the arguments of
    ``Table.train`` plus ``table`` -- dict(table=Table, target_col=int, feat_cols=[...], y_value=None, class_weight=None, **params).
    Returns one entry per fit: the ``Model``, or the ``RepairGbmError`` of a fit that failed (a failing fit does not fail the
    batch: the reference turns a failing build into PoorModel, python/repair/train.py:227-229).  Every model is the one
    ``Table.train`` returns for the same arguments, bit for bit.
    A fit with ``valid_table=Table`` is scored on that table WHILE it trains (cross_val_score, train.py:171-172, without a predictor):
    its entry is ``(Model, labels [rows] int32, values [rows] float64)`` -- what ``repair_chain`` of the model gives for those rows;
    with ``want_model=False`` no model is built for such a fit (``None`` in its place)."""
    n = len(fits)
    if n == 0:
        return []
    specs = (RgbmFitSpec * n)()
    keep = []
    for i, f in enumerate(fits):
        f = dict(f)
        tab = f.pop("table")
        fc = _i32(f.pop("feat_cols"))
        yv, cw = _f64(f.pop("y_value", None)), _f64(f.pop("class_weight", None))
        target = int(f.pop("target_col"))
        vtab = f.pop("valid_table", None)
        vlab = np.zeros(vtab.n, np.int32) if vtab is not None else None
        vval = np.zeros(vtab.n, np.float64) if vtab is not None else None
        f.setdefault("device_id", tab.device_id)
        p = make_params(**f)
        keep.append((tab, fc, yv, cw, p, vtab, vlab, vval))
        specs[i].valid_table = vtab.h if vtab is not None else None
        specs[i].valid_label_out = _p(vlab, C.c_int32)
        specs[i].valid_value_out = _p(vval, C.c_double)
        specs[i].table = tab.h
        specs[i].target_col = target
        specs[i].n_features = len(fc)
        specs[i].feat_cols = _p(fc, C.c_int32)
        specs[i].y_value = _p(yv, C.c_double)
        specs[i].class_weight = _p(cw, C.c_double)
        specs[i].params = C.pointer(p)
    handles = (C.c_void_p * n)()
    status = np.zeros(n, np.int32)
    _call("rgbm_table_train_batch", specs, n, handles, status)
    out = []
    # rgbm_last_error() is ONE thread-local string: it describes the LAST failing fit of the batch; the others report their status code only
    failing = [i for i in range(n) if status[i] != 0]
    last_msg = lib().rgbm_last_error().decode("utf-8", "replace") if failing else ""
    for i in range(n):
        if status[i] == 0 and (handles[i] or (keep[i][5] is not None and keep[i][4].reserved & FLAG_NO_MODEL)):
            m = Model(C.c_void_p(handles[i])) if handles[i] else None          # want_model=False: a CV fold, wanted for its scores only
            out.append(m if keep[i][5] is None else (m, keep[i][6], keep[i][7]))
        else:
            why = last_msg if (failing and i == failing[-1]) else ("status %d" % int(status[i]) if status[i] != 0 else "no model returned")
            out.append(RepairGbmError("fit %d of the batch failed (%d): %s" % (i, int(status[i]), why)))
    return out


BATCH_ROUTES = ("none", "fused", "single: not eligible", "single: one eligible fit", "single: LDS")


def train_batch_report(n):
    """What this thread's last ``train_batch`` call of ``n`` fits did with each fit (rgbm_table_train_batch_report): a list of
    dict(route, scan_waves, nchunk, lds_bytes) -- route 0 failed before a route was chosen, 1 fused kernels, 2 single-fit trainer (not
    eligible), 3 single-fit trainer (one eligible fit in the batch), 4 single-fit trainer (LDS); scan_waves 0 = one wave per feature."""
    a = np.zeros((max(int(n), 1), 4), np.int32)
    _call("rgbm_table_train_batch_report", a, n)
    return [dict(route=int(r[0]), scan_waves=int(r[1]), nchunk=int(r[2]), lds_bytes=int(r[3])) for r in a[:int(n)]]


def pair_counts_limits():
    """The two limits that close a group of ``Table.pair_counts`` (rgbm_table_pair_counts_report without a table; needs no device):
    dict(lds_cells = 32-bit counters of a group, max_cols = distinct columns of a group)."""
    head = np.zeros(6, np.int64)
    _call("rgbm_table_pair_counts_report", None, head, None, 0)
    return dict(lds_cells=int(head[4]), max_cols=int(head[5]))


def fd_measures_limits():
    """The two limits of ``Table.fd_measures`` (rgbm_table_fd_measures_report without a table; needs no device): dict(lds_cells = 32-bit
    counters of a dense joint table on the LDS route, max_lhs = columns of a left-hand side)."""
    out = np.zeros(2, np.int32)
    _call("rgbm_table_fd_measures_report", None, out, 0)
    return dict(lds_cells=int(out[0]), max_lhs=int(out[1]))


def recode_limits():
    """The limit of ``Table.recode`` (rgbm_table_recode_report without a table; needs no device): dict(lds_codes = the largest LUT that a
    workgroup stages in LDS)."""
    out = np.zeros(1, np.int32)
    _call("rgbm_table_recode_report", None, out, 0)
    return dict(lds_codes=int(out[0]))


def _chain_args(models, feat_cols, class_codes):
    T = len(models)
    arr = (C.c_void_p * max(T, 1))(*[m.h for m in models])
    fo = np.zeros(T + 1, np.int32)
    co = np.zeros(T + 1, np.int32)
    for t in range(T):
        fo[t + 1] = fo[t] + len(feat_cols[t])
        if class_codes is not None:
            co[t + 1] = co[t] + len(class_codes[t])
    fc = _i32(np.concatenate([np.asarray(f, np.int32) for f in feat_cols])) if T else np.zeros(1, np.int32)
    cc = None
    if class_codes is not None:
        cc = _i32(np.concatenate([np.asarray(c, np.int32) for c in class_codes] + [np.zeros(1, np.int32)]))
    return arr, fc, fo, cc, co


def repair_chain(models, target_col, feat_cols, class_codes, table, device_id=0):
    """Host-array chained repair. table: [C][n] int32, modified in place."""
    T = len(models)
    Cc, n = table.shape
    assert table.dtype == np.int32 and table.flags.c_contiguous
    arr, fc, fo, cc, co = _chain_args(models, feat_cols, class_codes)
    tc = _i32(target_col)
    lab = np.zeros((T, n), np.int32)
    prob = np.zeros((T, n), np.float64)
    _call("rgbm_repair_chain", arr, T, tc, fc, fo, cc, co, table, n, Cc, device_id, lab, prob)
    return lab, prob


class _PinnedBlock:
    """Owner of a page-locked host block (rgbm_host_alloc); the numpy view keeps it alive through `.base`."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        _call("rgbm_host_alloc", nbytes, C.byref(p))
        self.p, self.nbytes = p, nbytes
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (p.value, False), "version": 3}

    def __del__(self):
        if getattr(self, "p", None):
            lib().rgbm_host_free(self.p)
            self.p = None


def pinned_empty(shape, dtype=np.int32):
    """Uninitialised numpy array in page-locked host memory: encoders that fill it hand rgbm_table_create a block the copy engine
    reads directly (no pageable staging)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.asarray(_PinnedBlock(max(n, 1)))[:n].view(dtype).reshape(shape)


def pack_code_points(strings):
    """Python strings -> (int32 Unicode code points, int64 offsets [len + 1]): the string pools of rgbm_edit_distance.  Code points,
    not UTF-8 bytes: Python's str indexes code points, so the distances are those of repair.costs.edit_distance."""
    strings = [str(s) for s in strings]
    off = np.zeros(len(strings) + 1, np.int64)
    if strings:
        np.cumsum([len(s) for s in strings], out=off[1:])
    cp = np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.int32)
    return cp, off


def edit_distance(a, b, device_id=0):
    """Levenshtein distance of every pair of two lists of strings on the device: int32 [len(a)][len(b)] (include/rgbm.h)."""
    a_cp, a_off = pack_code_points(a)
    b_cp, b_off = pack_code_points(b)
    out = np.zeros((len(a_off) - 1, len(b_off) - 1), np.int32)
    _call("rgbm_edit_distance", device_id, a_cp, a_off, len(a_off) - 1, b_cp, b_off, len(b_off) - 1, out)
    return out


def nearest_values(a=None, b=None, cost=None, threshold=0.0, device_id=0):
    """Per string of ``a`` the position in ``b`` of the closest string when its cost is <= ``threshold`` and strictly below every other
    cost of the row, else -1 (include/rgbm.h rgbm_nearest_values): int32 [len(a)].  ``cost`` None: Levenshtein distances of the two
    lists of strings, computed and reduced on the device; else a float64 [n_a][n_b] matrix (NaN = no cost) and the strings are not read."""
    if cost is not None:
        m = _f64(cost)
        if m.ndim != 2:
            raise ValueError("cost must be a [n_a][n_b] matrix")
        out = np.full(m.shape[0], -1, np.int32)
        _call("rgbm_nearest_values", device_id, None, None, m.shape[0], None, None, m.shape[1], m, threshold, out)
        return out
    a_cp, a_off = pack_code_points(a)
    b_cp, b_off = pack_code_points(b)
    out = np.full(len(a_off) - 1, -1, np.int32)
    _call("rgbm_nearest_values", device_id, a_cp, a_off, len(a_off) - 1, b_cp, b_off, len(b_off) - 1, None, threshold, out)
    return out


def lof_1d(values, counts, k=20, threshold=1.5, want_scores=True, device_id=0):
    """The local outlier factor of every entry of a sorted dictionary (include/rgbm.h rgbm_lof_1d; the statement is
    repair.lof_codes.lof_codes): ``values`` float64 [d] ascending, ``counts`` rows per entry -> (scores float64 [d] or None,
    flag words uint64 [ceil(d / 64)], n_ties, n_near)."""
    v = _f64(values).reshape(-1)
    m = _flat(counts, np.int64)
    if len(v) != len(m):
        raise ValueError("values and counts must have one length")
    score = np.zeros(len(v), np.float64) if want_scores else None
    bits = np.zeros((len(v) + 63) // 64, np.uint64)
    info = np.zeros(2, np.int64)
    _call("rgbm_lof_1d", device_id, v, m, len(v), int(k), threshold, score, bits, info)
    return score, bits, int(info[0]), int(info[1])


RX_WORD_MAX_CP = 63           # the longest string one lane matches
RX_WAVE_MAX_CP = 4095         # RGBM_RX_WAVE_MAX_CP: the longest string the device matches


def regex_structure_raw(segs, anchors, const_cp, cp, off, device_id=0):
    """rgbm_regex_structure as it is (include/rgbm.h): ``segs`` rows of (kind, min, max, (4 class words), const_off, const_len), a pool of
    int32 code points and int64 offsets -> (state uint8 [n], out_off int64 [n + 1], out_cp int32 [out_off[n]], info int64 [4])."""
    arr = (RxSeg * max(len(segs), 1))()
    for i, (kind, mn, mx, cls, c_off, c_len) in enumerate(segs):
        arr[i] = RxSeg(int(kind), int(mn), int(mx), (C.c_uint32 * 4)(*[int(w) for w in cls]), int(c_off), int(c_len))
    const_cp, cp, off = _flat(const_cp, np.int32), _flat(cp, np.int32), _flat(off, np.int64)
    n = len(off) - 1
    state = np.zeros(max(n, 0), np.uint8)
    out_off = np.zeros(max(n, 0) + 1, np.int64)
    out = np.zeros(max(int(off[-1]) + n * len(const_cp), 1) if n > 0 else 1, np.int32)
    info = np.zeros(4, np.int64)
    _call("rgbm_regex_structure", device_id, arr, len(segs), int(anchors), const_cp, len(const_cp), cp, off, n, state, out_off, out, info)
    return state, out_off, out[:int(out_off[-1])], info


def regex_structure(program, strings, device_id=0, want_info=False):
    """Regex-structure repair of a list of strings on the device (include/rgbm.h rgbm_regex_structure; the statement is
    repair.regex_structure.repair_values): a list of the repaired string or None.  A string beyond the device's cap (state 2) is evaluated
    with the statement.  ``want_info``: also the int64 [4] route report."""
    from repair.regex_structure import program_arrays, repair_value
    strings = list(strings)
    a = program_arrays(program)
    cp, off = pack_code_points(strings)
    state, out_off, out, info = regex_structure_raw(a["segs"], a["anchors"], a["const_cp"], cp, off, device_id)
    text = out.astype("<u4").tobytes().decode("utf-32-le", "surrogatepass")
    res = [text[out_off[i]:out_off[i + 1]] if state[i] == 1 else (repair_value(program, strings[i]) if state[i] == 2 else None)
           for i in range(len(strings))]
    return (res, info) if want_info else res


class Table:
    """An int32 code table resident in HBM (``rgbm_table``)."""

    def __init__(self, codes, n_codes, device_id=0):
        codes = _i32(codes)
        self.c, self.n = codes.shape
        self.n_codes = _i32(n_codes)
        self.device_id = device_id
        h = C.c_void_p()
        _call("rgbm_table_create", codes, self.n, self.c, self.n_codes, device_id, C.byref(h))
        self.h = h

    @classmethod
    def _adopt(cls, handle, device_id):
        """Wrap a table the library has just created (gather_rows / from_dictionaries)."""
        t = cls.__new__(cls)
        t.h, t.device_id = handle, device_id
        n, c = C.c_int64(0), C.c_int32(0)
        _call("rgbm_table_shape", handle, C.byref(n), C.byref(c), None)
        t.n, t.c = int(n.value), int(c.value)
        t.n_codes = np.zeros(t.c, np.int32)
        _call("rgbm_table_shape", handle, None, None, t.n_codes)
        return t

    @classmethod
    def from_dictionaries(cls, indices, remaps, device_id=0):
        """Encode on the device: ``indices`` [C][n] int32 dictionary indices (< 0 = NULL), ``remaps[c][i]`` = code of
        dictionary entry i of column c (its rank among the sorted distinct values; -1 = NULL)."""
        idx = _i32(indices)
        c, n = idx.shape
        maps = [np.ascontiguousarray(m, np.int32) for m in remaps]
        if len(maps) != c:
            raise ValueError("one remap table per column expected")
        ptrs = (C.POINTER(C.c_int32) * c)(*[_p(m if len(m) else np.zeros(1, np.int32), C.c_int32) for m in maps])
        sizes = np.asarray([len(m) for m in maps], np.int32)
        h = C.c_void_p()
        _call("rgbm_table_create_dict", idx, n, c, ptrs, sizes, device_id, C.byref(h))
        return cls._adopt(h, device_id)

    # ---- relational steps around the models (csrc/rgbm_prep.hip and the rgbm_<step>.hip sources beside it)
    def _fetch_cells(self, n, want_cols, fetch=True):
        if not fetch:            # the result stays in the table's cell list (for `cellset_add`); the count is all that leaves the device
            return n
        rows = np.zeros(n, np.int64)
        cols = np.zeros(n, np.int32) if want_cols else None
        if n:
            _call("rgbm_table_cells_fetch", self.h, rows, cols)
        return (rows, cols) if want_cols else rows

    def detect_nulls(self, cols, fetch=True):
        """NULL cells of ``cols`` as (rows, cols), ordered by position in ``cols`` then row (ErrorDetectorApi.scala:128-157)."""
        cc = _flat(cols, np.int32)
        n = C.c_int64(0)
        _call("rgbm_table_detect_nulls", self.h, cc, len(cc), C.byref(n))
        return self._fetch_cells(int(n.value), True, fetch)

    def detect_cells(self, cols, null_is_error, keep_lo, keep_hi, flag_bits=None, fetch=True):
        """Cells of ``cols`` flagged by per-column CODE predicates (rgbm_table_detect_cells; repair.detect_codes builds them from the
        regex / value-domain / outlier detectors) as (rows, cols), ordered by position in ``cols`` then row.  Per column j: NULL cells
        when ``null_is_error[j]``; codes outside [keep_lo[j], keep_hi[j]] unless keep_lo[j] > keep_hi[j]; codes whose bit is set in
        ``flag_bits[j]`` (uint64 [ceil(n_codes / 64)], or None)."""
        cc = _flat(cols, np.int32)
        k = len(cc)
        ne = np.ascontiguousarray(np.asarray(null_is_error).reshape(-1) != 0, np.uint8)
        lo, hi = _flat(keep_lo, np.int32), _flat(keep_hi, np.int32)
        fb = list(flag_bits) if flag_bits is not None else [None] * k
        if not (len(ne) == len(lo) == len(hi) == len(fb) == k):
            raise ValueError("detect_cells: one predicate per column")
        keep, ptrs = [], (C.POINTER(C.c_uint64) * max(k, 1))()
        for j in range(k):
            if fb[j] is None:
                continue
            w = _flat(fb[j], np.uint64)
            if 0 <= cc[j] < self.c and len(w) != (int(self.n_codes[cc[j]]) + 63) // 64:
                raise ValueError("detect_cells: the bitset of column %d holds %d words, its %d codes need %d"
                                 % (cc[j], len(w), int(self.n_codes[cc[j]]), (int(self.n_codes[cc[j]]) + 63) // 64))
            keep.append(w)
            ptrs[j] = _p(w, C.c_uint64)
        n = C.c_int64(0)
        _call("rgbm_table_detect_cells", self.h, cc, k, ne, lo, hi, ptrs, C.byref(n))
        return self._fetch_cells(int(n.value), True, fetch)

    def detect_constraint(self, eq_cols, iq_col, cell_cols=(), fetch=True):
        """Rows violating  EQ(eq_cols...) & IQ(iq_col)  (ErrorDetectorApi.scala:189-244).  Returns the ascending violating rows
        when ``cell_cols`` is empty, else the cells (rows, cols) = violating rows x cell_cols, column-major."""
        eq, cc = _flat(eq_cols, np.int32), _flat(cell_cols, np.int32)
        nr, nc = C.c_int64(0), C.c_int64(0)
        _call("rgbm_table_detect_constraint", self.h, eq, len(eq), iq_col, cc, len(cc), C.byref(nr), C.byref(nc))
        return self._fetch_cells(int(nc.value), len(cc) > 0, fetch)

    def _dc_preds(self, preds, who):
        """``preds`` of `detect_dc` as an ``rgbm_dc_pred`` array, and the rank arrays it points into (keep them until the call returns)."""
        ops = dict(EQ=0, IQ=1, LT=2, GT=3)
        arr = (DcPred * max(len(preds), 1))()
        keep = []
        for k, (op, lc, rc, lr, rr) in enumerate(preds):
            arr[k].op, arr[k].left_col, arr[k].right_col, arr[k].reserved = ops[op], int(lc), int(rc), 0
            for name, col, r in (("left_rank", lc, lr), ("right_rank", rc, rr)):
                if r is None:
                    continue
                r = _flat(r, np.int32)
                if 0 <= int(col) < self.c and len(r) != int(self.n_codes[int(col)]):
                    raise ValueError("%s: the rank array of column %d holds %d entries, its dictionary %d" % (who, col, len(r), int(self.n_codes[int(col)])))
                keep.append(r)
                setattr(arr[k], name, _p(r, C.c_int32))
        return arr, keep

    def detect_dc(self, preds, cell_cols=(), max_pairs=0, fetch=True):
        """Rows violating a two-tuple denial constraint (rgbm_table_detect_dc; repair.dc_codes lowers a parsed constraint to this).
        ``preds``: 2 to 16 tuples (op, left_col, right_col, left_rank, right_rank) with op in 'EQ' / 'IQ' / 'LT' / 'GT' and the ranks int32
        [n_codes[col]] arrays (an entry < 0 = the value has no number) or None.  ``max_pairs`` <= 0: the library default; a table
        whose EQ groups hold more pairs raises RepairGbmError with code -2.  Returns as ``detect_constraint`` does."""
        arr, keep = self._dc_preds(preds, "detect_dc")
        cc = _flat(cell_cols, np.int32)
        nr, nc = C.c_int64(0), C.c_int64(0)
        _call("rgbm_table_detect_dc", self.h, arr, len(preds), cc, len(cc), int(max_pairs), C.byref(nr), C.byref(nc))
        return self._fetch_cells(int(nc.value), len(cc) > 0, fetch)

    def detect_dc_scan(self, preds, cell_cols=(), fetch=True):
        """`detect_dc` for an ORDER constraint, by sort and scan instead of pairs (rgbm_table_detect_dc_scan): ``preds`` as there, EQ
        predicates plus one or two LT / GT and no IQ (`repair.dc_codes.scan_eligible`; anything else raises RepairGbmError with code -2).
        No pair is evaluated, so there is no ``max_pairs``: the result is that of `detect_dc` without a limit."""
        arr, keep = self._dc_preds(preds, "detect_dc_scan")
        cc = _flat(cell_cols, np.int32)
        nr, nc = C.c_int64(0), C.c_int64(0)
        _call("rgbm_table_detect_dc_scan", self.h, arr, len(preds), cc, len(cc), C.byref(nr), C.byref(nc))
        return self._fetch_cells(int(nc.value), len(cc) > 0, fetch)

    def detect_row_bits(self, cols, bits, cell_cols=(), fetch=True):
        """Rows whose code has its bit set in EVERY listed column (rgbm_table_detect_row_bits: single-tuple constraints).  ``bits[k]``:
        uint64 [ceil((n_codes[cols[k]] + 1) / 64)], bit v = the predicates on the column hold for code v, the last bit for NULL."""
        cols_ = _flat(cols, np.int32)
        k = len(cols_)
        if len(bits) != k:
            raise ValueError("detect_row_bits: one bitset per column")
        keep, ptrs = [], (C.POINTER(C.c_uint64) * max(k, 1))()
        for j in range(k):
            w = _flat(bits[j], np.uint64)
            if 0 <= cols_[j] < self.c and len(w) != (int(self.n_codes[cols_[j]]) + 1 + 63) // 64:
                raise ValueError("detect_row_bits: the bitset of column %d holds %d words, its %d codes and NULL need %d"
                                 % (cols_[j], len(w), int(self.n_codes[cols_[j]]), (int(self.n_codes[cols_[j]]) + 64) // 64))
            keep.append(w)
            ptrs[j] = _p(w, C.c_uint64)
        cc = _flat(cell_cols, np.int32)
        nr, nc = C.c_int64(0), C.c_int64(0)
        _call("rgbm_table_detect_row_bits", self.h, cols_, k, ptrs, cc, len(cc), C.byref(nr), C.byref(nc))
        return self._fetch_cells(int(nc.value), len(cc) > 0, fetch)

    def rows_of_cells(self, rows):
        """Ascending positions of the rows that hold at least one of the given cells (the dirty rows, model.py:549-553)."""
        r = np.ascontiguousarray(rows, np.int64)
        n = C.c_int64(0)
        _call("rgbm_table_rows_of_cells", self.h, r, len(r), C.byref(n))
        return self._fetch_cells(int(n.value), False)

    # ---- the cell set (csrc/rgbm_cellset.hip): the union of detector results, kept on the device.  Every `detect_*` method takes
    # ``fetch=False``: the result then stays in the table's cell list for `cellset_add` and the method returns its cell count.
    def cellset_open(self, cols):
        """A zeroed cell set over the distinct columns ``cols`` (rgbm_table_cellset_open); a second open replaces it."""
        cc = _flat(cols, np.int32)
        _call("rgbm_table_cellset_open", self.h, cc, len(cc))
        self._cellset_cols = len(cc)

    def cellset_add(self):
        """ORs the cell list the last ``detect_*`` call left into the set; cells of columns outside the set are skipped."""
        _call("rgbm_table_cellset_add", self.h)

    def cellset_emit(self, fetch=True):
        """The set as (rows, cols, codes, counts): ordered by position in the set's columns, then ascending row; ``codes`` are the codes the
        cells hold now, ``counts[j]`` the cells of the set's j-th column.  The set stays open.  ``fetch=False``: the cells stay in the
        table's cell list and ``counts`` alone is returned."""
        k = getattr(self, "_cellset_cols", 0)
        n, counts = C.c_int64(0), np.zeros(max(k, 1), np.int64)
        _call("rgbm_table_cellset_emit", self.h, C.byref(n), counts)
        if not fetch:
            return counts[:k]
        rows, cols = self._fetch_cells(int(n.value), True)
        return rows, cols, self.cells_fetch_codes(int(n.value)), counts[:k]

    def cells_fetch_codes(self, n):
        """The codes of the last `cellset_emit` (rgbm_table_cells_fetch_codes; refused once another result replaced its cell list)."""
        codes = np.zeros(n, np.int32)
        _call("rgbm_table_cells_fetch_codes", self.h, codes)
        return codes

    def cellset_close(self):
        _call("rgbm_table_cellset_close", self.h)
        self._cellset_cols = 0

    # ---- the repair run on the open set: given cells in, weak labels out, null-out and dirty rows straight from the matrix
    def cellset_add_cells(self, rows, cols):
        """ORs host-given cells (any order, duplicates allowed) into the open set; cells outside the table or the set's columns are skipped."""
        r, c2 = _flat(rows, np.int64), _flat(cols, np.int32)
        if len(r) != len(c2):
            raise ValueError("rows and cols must have the same length")
        _call("rgbm_table_cellset_add_cells", self.h, r, c2, len(r))

    def cellset_drop_weak(self, target_col, pair_idx, min_cnt, single_ok, beta, row_count):
        """Clears the weak-labelled cells of the set's column ``target_col``: the `weak` flag of ``cell_domains`` on the same rows, evaluated
        on the device.  The examined cells stay behind as the table's cell list.  Returns (cells examined, cells cleared)."""
        pi, mc, ok = _flat(pair_idx, np.int32), _flat(min_cnt, np.int64), _flat(single_ok, np.uint8)
        if len(pi) != len(mc):
            raise ValueError("one min_cnt per pair")
        last = getattr(self, "_pc_last", None)            # (without one the library refuses the call before it reads single_ok)
        if last is not None and 0 <= int(target_col) < self.c and len(ok) != int(last[1][int(target_col)]):
            raise ValueError("single_ok must hold one entry per bin of the target (%d), not %d" % (int(last[1][int(target_col)]), len(ok)))
        cells, weak = C.c_int64(0), C.c_int64(0)
        _call("rgbm_table_cellset_drop_weak", self.h, target_col, pi, len(pi), mc, ok, beta, row_count, C.byref(cells), C.byref(weak))
        return int(cells.value), int(weak.value)

    def cellset_null(self):
        """NULL into every cell of the open set, in place in HBM (`null_cells` without a cell list); returns the number of cells."""
        n = C.c_int64(0)
        _call("rgbm_table_cellset_null", self.h, C.byref(n))
        return int(n.value)

    def cellset_rows(self, fetch=True):
        """Ascending positions of the rows that hold a cell of the open set (`rows_of_cells` without an upload); ``fetch=False``: their number."""
        n = C.c_int64(0)
        _call("rgbm_table_cellset_rows", self.h, C.byref(n))
        return self._fetch_cells(int(n.value), False, fetch)

    def null_cells(self, rows, cols, target_cols):
        """convertErrorCellsToNull (RepairApi.scala:171-211), in place in HBM."""
        r, c2, tc = np.ascontiguousarray(rows, np.int64), _i32(cols), _flat(target_cols, np.int32)
        if len(r) != len(c2):
            raise ValueError("rows and cols must have the same length")
        _call("rgbm_table_null_cells", self.h, r, c2, len(r), tc, len(tc))

    def read_cells(self, rows, cols):
        r, c2 = np.ascontiguousarray(rows, np.int64), _i32(cols)
        out = np.zeros(len(r), np.int32)
        _call("rgbm_table_read_cells", self.h, r, c2, len(r), out)
        return out

    def set_column_kind(self, col, categorical=True):
        """CATEGORICAL column: codes that no training row of a model holds are missing for that model (per-model dictionaries)."""
        _call("rgbm_table_set_column_kind", self.h, col, 1 if categorical else 0)

    def set_column_values(self, col, values):
        """NUMERIC column: the ascending distinct values behind its codes (bin bounds at value midpoints)."""
        v = np.ascontiguousarray(values, np.float64)
        _call("rgbm_table_set_column_values", self.h, col, v, len(v))

    def write_cells(self, rows, cols, codes):
        r, c2, v = np.ascontiguousarray(rows, np.int64), _i32(cols), _i32(codes)
        _call("rgbm_table_write_cells", self.h, r, c2, v, len(r))

    def gather_rows(self, rows):
        r = np.ascontiguousarray(rows, np.int64)
        h = C.c_void_p()
        _call("rgbm_table_gather_rows", self.h, r, len(r), C.byref(h))
        return Table._adopt(h, self.device_id)

    @staticmethod
    def concat(parts):
        """The rows of the tables `parts` one after the other (same columns, dictionaries and device): kinds and values inherited."""
        parts = list(parts)
        hs = (C.c_void_p * len(parts))(*[p.h for p in parts])
        h = C.c_void_p()
        _call("rgbm_table_concat", hs, len(parts), C.byref(h))
        return Table._adopt(h, parts[0].device_id)

    def smoten(self, target_col, feat_cols, fit_rows, classes, pick_off, picks, k=5, want_nn=False):
        """SMOTEN in code space (include/rgbm.h rgbm_table_smoten; the statement is `repair.rebalance_codes.smoten_codes`): the metric is
        fitted on `fit_rows`; for class classes[i] (ascending) the rows pick_off[i] .. pick_off[i + 1] - 1 of the new table are grown from
        the class's rows `picks` (positions within the class's fit rows).  Returns the table of the synthetic rows, with `want_nn`
        (table, [nn [m][k] per class]): the neighbour lists as positions within the class's rows."""
        fc, fr = _i32(feat_cols), np.ascontiguousarray(fit_rows, np.int64)
        cl, po, pk = _i32(classes), np.ascontiguousarray(pick_off, np.int64), np.ascontiguousarray(picks, np.int64)
        if len(po) != len(cl) + 1 or (len(po) and len(pk) != int(po[-1])):
            raise ValueError("pick_off holds one entry more than classes and ends at len(picks)")
        nn = None
        if want_nn:
            y = self.read_cells(fr, np.full(len(fr), target_col, np.int32)) if len(fr) else np.zeros(0, np.int32)
            m = [int((y == c).sum()) for c in cl]
            nn = np.full((max(sum(m), 1), int(k)), -1, np.int64)
        h = C.c_void_p()
        _call("rgbm_table_smoten", self.h, target_col, fc, len(fc), fr, len(fr), k, cl, len(cl), po, pk if len(pk) else np.zeros(1, np.int64), nn,
              C.byref(h))
        tab = Table._adopt(h, self.device_id)
        if not want_nn:
            return tab
        off = np.concatenate([[0], np.cumsum(m)])
        return tab, [nn[off[i]:off[i + 1]] for i in range(len(cl))]

    def repair_pmf(self, model, target_col, feat_cols, top_k=32, threshold=0.0, cur_codes=None, want_cur_prob=False):
        """Candidate distributions of the NULL cells of ``target_col`` (model.py:1196-1212).  Returns
        (rows [m], classes [m][top_k] (-1 padded), probs [m][top_k] (0 padded)[, cur_prob [m]])."""
        fc = _i32(feat_cols)
        _, n_null = self.count_codes(target_col)
        rows = np.zeros(n_null, np.int64)
        cls = np.zeros((n_null, top_k), np.int32)
        pr = np.zeros((n_null, top_k), np.float64)
        cur = _i32(cur_codes)
        if cur is not None and len(cur) != n_null:
            raise ValueError("cur_codes must hold one code per NULL cell of the target (%d)" % n_null)
        cp = np.zeros(n_null, np.float64) if (want_cur_prob or cur is not None) else None
        n = C.c_int64(0)
        _call("rgbm_table_repair_pmf", self.h, model.h, target_col, fc, len(fc), top_k, threshold, cur, n_null, C.byref(n), rows, cls, pr, cp)
        assert int(n.value) == n_null
        return (rows, cls, pr, cp) if cp is not None else (rows, cls, pr)

    def repair_pmf_weighted(self, model, target_col, feat_cols, top_k=32, threshold=0.0, cur_codes=None, cost_rows=None, cost=None,
                            weight=0.0, renormalise=False):
        """`repair_pmf` with the update costs of the probability modes (model.py `_compute_repair_pmf`; include/rgbm.h
        rgbm_table_repair_pmf_weighted).  ``cost`` [R + 1][K] float64 (NaN = no cost; the last row: each class against itself),
        ``cost_rows`` [m] int32 per NULL cell (-1 = leave the cell alone).  Returns (rows, classes, probs, cur_prob, top1_cost)."""
        fc = _i32(feat_cols)
        _, n_null = self.count_codes(target_col)
        cur, crow = _i32(cur_codes), _i32(cost_rows)
        for name, a in (("cur_codes", cur), ("cost_rows", crow)):
            if a is not None and len(a) != n_null:
                raise ValueError("%s must hold one entry per NULL cell of the target (%d)" % (name, n_null))
        cst = None if cost is None else np.ascontiguousarray(np.atleast_2d(cost), np.float64)
        if crow is not None and cst is None:
            raise ValueError("cost_rows without a cost matrix")
        n_cost_rows = 0 if cst is None else cst.shape[0] - 1
        rows = np.zeros(n_null, np.int64)
        cls = np.zeros((n_null, top_k), np.int32)
        pr = np.zeros((n_null, top_k), np.float64)
        cp = np.zeros(n_null, np.float64)
        tc = np.full(n_null, np.nan, np.float64)
        n = C.c_int64(0)
        _call("rgbm_table_repair_pmf_weighted", self.h, model.h, target_col, fc, len(fc), top_k, threshold, cur, crow, cst, n_cost_rows, weight,
              1 if renormalise else 0, n_null, C.byref(n), rows, cls, pr, cp, tc)
        assert int(n.value) == n_null
        return rows, cls, pr, cp, tc

    def count_codes(self, col):
        """(rows per code [n_codes[col]], NULL rows) of one column."""
        out = np.zeros(int(self.n_codes[col]), np.int64)
        nn = C.c_int64(0)
        _call("rgbm_table_count_codes", self.h, col, out, C.byref(nn))
        return out, int(nn.value)

    def column_stats(self, cols, len_luts=None, n_bins=0):
        """Column statistics of the listed columns in one call (include/rgbm.h rgbm_table_column_stats), exactly the integers of
        ``repair.table_stats.column_stats``: a dict of int64 [len(cols)] arrays ``nulls``, ``distinct``, ``min_code``, ``max_code``,
        ``len_sum``, ``len_max`` and ``edges`` (int32 [len(cols)][n_bins + 1], None when n_bins == 0).  ``len_luts``: per listed column an
        int32 [n_codes] array (the length of every dictionary entry) or None; a column may be listed more than once."""
        from repair.table_stats import FIELDS
        cc = _flat(cols, np.int32)
        luts = [None] * len(cc) if len_luts is None else [None if l is None else _flat(l, np.int32) for l in len_luts]
        if len(luts) != len(cc):
            raise ValueError("one length LUT (or None) per listed column expected")
        for c, l in zip(cc, luts):
            if l is not None and 0 <= c < self.c and len(l) != int(self.n_codes[c]):
                raise ValueError("the length LUT of column %d must hold one entry per code (%d)" % (c, int(self.n_codes[c])))
        ptrs = (C.POINTER(C.c_int32) * max(len(cc), 1))(*[_p(l, C.c_int32) for l in luts])
        stats = np.zeros((len(cc), len(FIELDS)), np.int64)
        edges = np.full((len(cc), n_bins + 1), -1, np.int32) if n_bins > 0 else None
        _call("rgbm_table_column_stats", self.h, cc, len(cc), ptrs if any(l is not None for l in luts) else None, n_bins, stats, edges)
        out = {f: stats[:, i].copy() for i, f in enumerate(FIELDS)}
        out["edges"] = edges
        return out

    def fd_measures(self, lhs, rhs_cols):
        """The measures of X -> Y for one left-hand side ``lhs`` (0 .. 11 columns) against the right-hand sides ``rhs_cols`` in one call
        (include/rgbm.h rgbm_table_fd_measures), exactly the integers of ``repair.fd_codes.fd_measures``: dict(groups = int64, kept,
        violating, xy_groups = int64 [len(rhs_cols)])."""
        lc, rc = _flat(lhs, np.int32), _flat(rhs_cols, np.int32)
        g, kept, viol, xy = (np.zeros(1, np.int64),) + tuple(np.zeros(max(len(rc), 1), np.int64) for _ in range(3))
        _call("rgbm_table_fd_measures", self.h, lc, len(lc), rc, len(rc), g, kept, viol, xy)
        self._fd_last = len(rc)                           # the right-hand sides of the call whose routes the table now holds
        return dict(groups=np.int64(g[0]), kept=kept[:len(rc)], violating=viol[:len(rc)], xy_groups=xy[:len(rc)])

    def fd_measures_report(self):
        """The routes the last successful ``fd_measures`` call on this table took (include/rgbm.h rgbm_table_fd_measures_report):
        dict(routes = one per right-hand side, 0 = LDS counters, 1 = hash tables; lds_cells, max_lhs = the two limits)."""
        n_rhs = getattr(self, "_fd_last", 0)
        out = np.zeros(n_rhs + 2, np.int32)
        _call("rgbm_table_fd_measures_report", self.h, out, n_rhs)
        return dict(routes=[int(r) for r in out[:n_rhs]], lds_cells=int(out[n_rhs]), max_lhs=int(out[n_rhs + 1]))

    def recode(self, luts, n_codes_out, want_unmapped=True):
        """This table in ANOTHER CODE SPACE (include/rgbm.h rgbm_table_recode), exactly the integers of ``repair.recode_codes.recode``:
        ``luts[j]`` is None (the codes of column j stay; ``n_codes_out[j]`` must be its dictionary size) or int32 [n_codes[j]] with
        entries in [-1, n_codes_out[j]).  Returns (a new resident Table of the same rows with the dictionary sizes ``n_codes_out`` and NO
        column kinds, values or multiplicities; int64 [c]: the cells per column that held a value and are NULL now, or None)."""
        luts = list(luts)
        if len(luts) != self.c:
            raise ValueError("one LUT (or None) per column expected")
        maps = [None if m is None else np.ascontiguousarray(m, np.int32) for m in luts]
        for j, m in enumerate(maps):
            if m is not None and len(m) != int(self.n_codes[j]):
                raise ValueError("the LUT of column %d has %d entries, its dictionary %d" % (j, len(m), int(self.n_codes[j])))
        # (an empty array has no address of its own: a LUT column never passes NULL, which would mean identity)
        keep = [None if m is None else (m if len(m) else np.zeros(1, np.int32)) for m in maps]
        ptrs = (C.POINTER(C.c_int32) * max(self.c, 1))(*[_p(m, C.c_int32) for m in keep])
        nco = _flat(n_codes_out, np.int32)
        if len(nco) != self.c:
            raise ValueError("one output dictionary size per column expected")
        un = np.zeros(max(self.c, 1), np.int64) if want_unmapped else None
        h = C.c_void_p()
        _call("rgbm_table_recode", self.h, ptrs, nco, C.byref(h), un)
        return Table._adopt(h, self.device_id), (un[:self.c] if want_unmapped else None)

    def recode_report(self):
        """The route each column took in the last successful ``recode`` call on this table (include/rgbm.h rgbm_table_recode_report):
        dict(routes = one per column, 0 = identity copy, 1 = LDS LUT, 2 = global LUT, -1 before any call; lds_codes = the limit)."""
        out = np.zeros(self.c + 1, np.int32)
        _call("rgbm_table_recode_report", self.h, out, self.c)
        return dict(routes=[int(r) for r in out[:self.c]], lds_codes=int(out[self.c]))

    def fd_map(self, x, y):
        """The rule model of the functional dependency x -> y (include/rgbm.h rgbm_table_fd_map): int32 [n_codes[x]], the single y code
        each x code occurs with over the rows where both are non-NULL, -1 for none or several."""
        out = np.full(int(self.n_codes[x]), -1, np.int32)
        _call("rgbm_table_fd_map", self.h, x, y, out)
        return out

    def rule_fill(self, y, x, lut, row_begin=0, n_rows=None, want_labels=True):
        """One rule step of the chained repair (include/rgbm.h rgbm_table_rule_fill): pred = lut[x code] (x = -1: the constant lut[0]);
        NULL cells of column y in the row range receive pred >= 0.  Returns pred per row (int32 [n_rows]) or None."""
        n_rows = self.n - row_begin if n_rows is None else n_rows
        l = _flat(lut, np.int32)
        out = np.full(n_rows, -1, np.int32) if want_labels else None
        _call("rgbm_table_rule_fill", self.h, y, x, l, len(l), row_begin, n_rows, out)
        return out

    def pair_counts(self, pairs, luts=None, n_bins=None):
        """Dense joint counts of column pairs, one pass over the rows (include/rgbm.h rgbm_table_pair_counts): a list of int64
        [(n_bins[x] + 1)][(n_bins[y] + 1)] arrays, NULL in the last slot of each side.  ``luts``: {column: int32 [n_codes] code -> bin};
        ``n_bins``: {column: bins} (default: the column's codes are its bins).  The result stays on the device for ``cell_domains``."""
        pc = _i32(np.asarray(pairs, np.int32).reshape(-1, 2))
        nb = np.asarray(self.n_codes, np.int32).copy()
        for c, d in dict(n_bins or {}).items():
            nb[int(c)] = int(d)
        keep = {int(c): _i32(l) for c, l in dict(luts or {}).items() if l is not None}
        for c, l in keep.items():
            if len(l) != int(self.n_codes[c]):
                raise ValueError("the LUT of column %d must hold one bin per code (%d)" % (c, int(self.n_codes[c])))
        ptrs = (C.POINTER(C.c_int32) * self.c)(*[_p(keep[c] if len(keep[c]) else np.zeros(1, np.int32), C.c_int32) if c in keep else None
                                                 for c in range(self.c)])
        shapes = [(int(nb[x]) + 1, int(nb[y]) + 1) for x, y in pc]
        out = np.zeros(int(sum(a * b for a, b in shapes)), np.int64)
        _call("rgbm_table_pair_counts", self.h, pc, len(pc), ptrs if keep else None, nb, out)
        self._pc_last = (len(pc), nb)                     # what the table now holds: the pairs and the bins per column of this call
        res, at = [], 0
        for a, b in shapes:
            res.append(out[at:at + a * b].reshape(a, b)); at += a * b
        return res

    def pair_counts_report(self):
        """The plan the last ``pair_counts`` call on this table took (include/rgbm.h rgbm_table_pair_counts_report): dict(pairs = one
        dict(group, slot_x, slot_y) per pair, group -1 = the HBM kernel; groups, max_group_cells, grid_x, rows_per_wg; lds_cells, max_cols =
        the two limits that close a group)."""
        n_pairs = getattr(self, "_pc_last", (0, None))[0]
        head, rows = np.zeros(6, np.int64), np.zeros((max(n_pairs, 1), 3), np.int32)
        _call("rgbm_table_pair_counts_report", self.h, head, rows, n_pairs)
        return dict(pairs=[dict(group=int(r[0]), slot_x=int(r[1]), slot_y=int(r[2])) for r in rows[:n_pairs]], groups=int(head[0]),
                    max_group_cells=int(head[1]), grid_x=int(head[2]), rows_per_wg=int(head[3]), lds_cells=int(head[4]), max_cols=int(head[5]))

    def cell_domains(self, target_col, rows, pair_idx, min_cnt, single_ok, beta, row_count, want_probs=False):
        """Domains / weak labels of the error cells (``rows``) of one discrete target on the tables of the last ``pair_counts`` call
        (include/rgbm.h rgbm_table_cell_domains).  Returns (weak [m] uint8, top [m] int32, top_prob [m] float64, probs [m][d] or None)."""
        r = np.ascontiguousarray(rows, np.int64)
        pi, mc, ok = _flat(pair_idx, np.int32), _flat(min_cnt, np.int64), _flat(single_ok, np.uint8)
        if len(pi) != len(mc):
            raise ValueError("one min_cnt per pair")
        last = getattr(self, "_pc_last", None)            # (without one the library refuses the call before it reads single_ok)
        if last is not None and 0 <= int(target_col) < self.c and len(ok) != int(last[1][int(target_col)]):
            raise ValueError("single_ok must hold one entry per bin of the target (%d), not %d" % (int(last[1][int(target_col)]), len(ok)))
        m = len(r)
        weak, top, tp = np.zeros(m, np.uint8), np.full(m, -1, np.int32), np.zeros(m, np.float64)
        probs = np.zeros((m, len(ok)), np.float64) if want_probs else None
        _call("rgbm_table_cell_domains", self.h, target_col, r, m, pi, len(pi), mc, ok, beta, row_count, weak, top, tp, probs)
        return weak, top, tp, probs

    def kmeans_assign(self, cols, code_off, p, h, first):
        """One Lloyd assignment step of the q-gram k-means in code space (include/rgbm.h rgbm_table_kmeans_assign; the statement is
        repair.qgram_kmeans.assign_step).  ``p`` float64 [d_tot][k], ``h`` float64 [k], ``code_off[j]`` = start of column cols[j]'s dictionary
        among the d_tot entries.  Returns (counts int64 [k][d_tot], sizes int64 [k], n_changed); the labels stay on the device (``kmeans_read``)."""
        cc, off = _flat(cols, np.int32), _flat(code_off, np.int64)
        pp, hh = np.ascontiguousarray(p, np.float64), _flat(h, np.float64)
        if pp.ndim != 2 or pp.shape[1] != len(hh) or len(off) != len(cc):
            raise ValueError("kmeans_assign: p must be [d_tot][k], h [k], one offset per column")
        d_tot, k = pp.shape
        counts, sizes, nch = np.zeros((k, d_tot), np.int64), np.zeros(k, np.int64), C.c_int64(0)
        _call("rgbm_table_kmeans_assign", self.h, cc, len(cc), off, k, pp, d_tot, hh, 1 if first else 0, counts, sizes, C.byref(nch))
        return counts, sizes, int(nch.value)

    def kmeans_bisect(self, cols, code_off, slot_of, child, p, h, first):
        """One pass of a level of the bisecting k-means in code space (include/rgbm.h rgbm_table_kmeans_bisect; the statement is
        repair.qgram_bisect.bisect_step).  ``slot_of`` int32 [n_nodes] (-1 = the node is not being split), ``child`` int32 [2m], ``p`` float64
        [d_tot][2m], ``h`` float64 [2m].  Returns (counts int64 [2m][d_tot], sizes int64 [2m], n_changed); the labels (node ids) stay on the
        device (``kmeans_read``)."""
        cc, off = _flat(cols, np.int32), _flat(code_off, np.int64)
        so, ch = _flat(slot_of, np.int32), _flat(child, np.int32)
        pp, hh = np.ascontiguousarray(p, np.float64), _flat(h, np.float64)
        if pp.ndim != 2 or pp.shape[1] != len(hh) or len(hh) != len(ch) or len(ch) % 2 or len(off) != len(cc):
            raise ValueError("kmeans_bisect: p must be [d_tot][2m], h and child [2m], one offset per column")
        d_tot, k = pp.shape
        counts, sizes, nch = np.zeros((k, d_tot), np.int64), np.zeros(k, np.int64), C.c_int64(0)
        _call("rgbm_table_kmeans_bisect", self.h, cc, len(cc), off, d_tot, so, len(so), k // 2, ch, pp, hh, 1 if first else 0, counts, sizes,
              C.byref(nch))
        return counts, sizes, int(nch.value)

    def kmeans_read(self):
        """The labels the last ``kmeans_assign`` left on the device, int32 [n]."""
        out = np.zeros(self.n, np.int32)
        _call("rgbm_table_kmeans_read", self.h, out)
        return out

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h and _lib is not None:
            _lib.rgbm_table_free(h)

    __del__ = close

    def train(self, target_col, feat_cols, y_value=None, class_weight=None, want_stats=False, **params):
        fc = _i32(feat_cols)
        yv, cw = _f64(y_value), _f64(class_weight)
        params.setdefault("device_id", self.device_id)
        p = make_params(**params)
        h = C.c_void_p()
        st = RgbmTrainStats()
        _call("rgbm_table_train", self.h, target_col, fc, len(fc), yv, cw, C.byref(p), C.byref(h), C.byref(st) if want_stats else None)
        m = Model(h)
        return (m, st.as_dict()) if want_stats else m

    def repair_chain(self, models, target_col, feat_cols, row_begin=0, n_rows=None, want_prob=True):
        T = len(models)
        n_rows = self.n - row_begin if n_rows is None else n_rows
        arr, fc, fo, _, _ = _chain_args(models, feat_cols, None)
        tc = _i32(target_col)
        lab = np.zeros((T, n_rows), np.int32)
        prob = np.zeros((T, n_rows), np.float64) if want_prob else None
        _call("rgbm_table_repair_chain", self.h, arr, T, tc, fc, fo, row_begin, n_rows, lab, prob)
        return lab, prob

    def set_row_multiplicity(self, mult):
        """Row i stands for mult[i] (1..255) identical rows of a larger table (repair.pipeline.distinct_rows): every later train() on this
        table returns the model of the EXPANDED table, byte for byte.  None clears."""
        m = None if mult is None else np.ascontiguousarray(mult, np.uint8)
        if m is not None and m.shape != (self.n,):
            raise ValueError("one multiplicity per row")
        _call("rgbm_table_set_row_multiplicity", self.h, m)

    def row_multiplicity(self):
        """The multiplicities the table carries, uint8 [n] (1 everywhere when it carries none)."""
        out = np.zeros(self.n, np.uint8)
        _call("rgbm_table_read_row_multiplicity", self.h, out)
        return out

    def distinct_rows(self, want_inverse=False):
        """The distinct rows of this table as a new resident table, found on the device (rgbm_table_distinct_rows): groups in order of
        first occurrence, a group of more than 255 rows kept as several copies, the multiplicities attached -- train() on it returns
        the models of this table, byte for byte.  `want_inverse`: also int64 [n], the position of every row's group in the new table."""
        h, m = C.c_void_p(), C.c_int64(0)
        inv = np.zeros(self.n, np.int64) if want_inverse else None
        _call("rgbm_table_distinct_rows", self.h, C.byref(h), C.byref(m), inv)
        d = Table._adopt(h, self.device_id)
        return (d, inv) if want_inverse else d

    def distinct_view_info(self):
        """The distinct-row view train() keeps for this table (rgbm_table_distinct_view_info): its state ("none", "built", "not worth it",
        "cannot"), its rows, and the distinct passes run for this table object."""
        st, rows, builds = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _call("rgbm_table_distinct_view_info", self.h, C.byref(st), C.byref(rows), C.byref(builds))
        return {"state": VIEW_STATES[st.value], "rows": int(rows.value), "builds": int(builds.value)}

    def repair_chain_gather(self, models, target_col, feat_cols, row_begin=0, n_rows=None):
        """The chained repair of THIS rank's rows, the outputs all-gathered over the calling thread's communicator on the device (C2):
        returns (labels [T][sum of the ranks' rows] in rank order, probs likewise, first row of this rank, rows of every rank)."""
        T = len(models)
        n_rows = self.n - row_begin if n_rows is None else n_rows
        counts = comm_all_gather_sizes([n_rows])[:, 0]
        mx = int(max(int(counts.max()), 1))
        nr = len(counts)
        arr, fc, fo, _, _ = _chain_args(models, feat_cols, None)
        tc = _i32(target_col)
        lab = np.zeros((nr, T, mx), np.int32)
        prob = np.zeros((nr, T, mx), np.float64)
        _call("rgbm_table_repair_chain_gather", self.h, arr, T, tc, fc, fo, row_begin, n_rows, mx, lab, prob)
        labels = np.concatenate([lab[r, :, :int(counts[r])] for r in range(nr)], axis=1)
        probs = np.concatenate([prob[r, :, :int(counts[r])] for r in range(nr)], axis=1)
        me = comm_info()["rank"]
        return labels, probs, int(counts[:me].sum()), [int(x) for x in counts]

    def read_column(self, col):
        out = np.zeros(self.n, np.int32)
        _call("rgbm_table_read_column", self.h, col, out)
        return out
