"""CPU: the C-ABI library loads, exports every symbol include/rgbm.h declares, and fails loudly
(no CPU fallback) when no HIP device is present."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "rgbm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rgbm_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported():
    from repair import _native
    lib = _native.lib()
    names = _declared()
    assert len(names) >= 16
    for n in names:
        assert hasattr(lib, n), "include/rgbm.h declares %s but librepairgbm.so does not export it" % n
    assert sorted(_native.EXPORTED_SYMBOLS) == names


def test_no_oracle_symbols_or_cpu_fallback_in_product():
    from repair import _native
    lib = _native.lib()
    assert not hasattr(lib, "orc_train")
    # product sources never reference oracle/
    pkg = os.path.join(ROOT, "spark-data-repair-plugin_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "librgbm_oracle" not in txt, f


def test_fails_loudly_without_gpu():
    from repair import _native
    if _native.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_native.RepairGbmError, match="no HIP device"):
        _native.train(np.zeros((2, 10), np.int32), [1, 1], np.zeros(10, np.int32), 2, objective=0)
    with pytest.raises(_native.RepairGbmError):
        _native.Table(np.zeros((2, 10), np.int32), [1, 1])
    from repair.engine import HipEngine
    with pytest.raises(_native.RepairGbmError, match="no CPU fallback"):
        HipEngine(0)


def test_model_blob_roundtrip_and_validation():
    """rgbm_model_save/load work on the host (no GPU needed) and reject corrupt input."""
    from oracle import oracle as O
    from repair import _native
    rng = np.random.default_rng(0)
    X = rng.integers(0, 5, (3, 500)).astype(np.int32); y = (X[0] + X[1]) % 3
    blob = O.train(X, [5, 5, 5], y, 3, objective=1, num_class=3, n_estimators=5, min_data_in_leaf=5).save()
    m = _native.Model.load(blob)            # shared serialisation format
    assert m.save() == blob
    assert m.info() == dict(objective=1, num_class=3, K=3, n_iter=5, F=3)
    assert m.importance("split").sum() > 0
    with pytest.raises(_native.RepairGbmError):
        _native.Model.load(blob[:40])
    bad = bytearray(blob); bad[0] ^= 0xFF
    with pytest.raises(_native.RepairGbmError):
        _native.Model.load(bytes(bad))


def test_batch_report_refuses_a_count_that_is_not_the_last_batch():
    """rgbm_table_train_batch_report needs no device; a thread that has made no batch call holds a report of zero fits."""
    import threading
    from repair import _native
    seen = []

    def fresh_thread():
        seen.append(_native.train_batch_report(0))
        try:
            _native.train_batch_report(3)
        except _native.RepairGbmError as e:
            seen.append(str(e))
    th = threading.Thread(target=fresh_thread)
    th.start(); th.join()
    assert seen[0] == [] and len(seen) == 2 and "last rgbm_table_train_batch call" in seen[1], seen


def test_pair_counts_report_gives_its_limits_without_a_table():
    """rgbm_table_pair_counts_report needs no device for the two limits of a group; pairs without a table are a bad argument."""
    from repair import _native
    from tests.helpers import csrc_constant
    lim = _native.pair_counts_limits()
    assert lim["max_cols"] == csrc_constant("PC_MAXC") and lim["lds_cells"] > 0
    # the counters and the uint16 row tile of a group share 160 KiB of LDS less 2 KiB
    assert lim["lds_cells"] * 4 + lim["max_cols"] * csrc_constant("PC_B") * 2 == 160 * 1024 - 2048
    head, rows = np.zeros(6, np.int64), np.zeros(3, np.int32)
    rc = _native.lib().rgbm_table_pair_counts_report(None, head.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                     rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int32(1))
    assert rc == -1 and b"rgbm_table_pair_counts_report" in _native.lib().rgbm_last_error()


def test_params_struct_layout_matches_oracle():
    from oracle import oracle as O
    from repair import _native
    assert [f[0] for f in O.OrcParams._fields_] == [f[0] for f in _native.RgbmParams._fields_]
    assert ctypes.sizeof(O.OrcParams) == ctypes.sizeof(_native.RgbmParams) == 104


def test_model_load_rejects_inconsistent_headers():
    """A blob travels through pickle and the cross-rank all-gather: objective / num_class / K must agree with each other
    (the predictor sizes its score scratch by them) and the tree count must fit the buffer."""
    import struct
    from oracle import oracle as O
    from repair import _native
    rng = np.random.default_rng(1)
    X = rng.integers(0, 4, (2, 300)).astype(np.int32); y = (X[0] + X[1]) % 3
    blob = O.train(X, [4, 4], y, 3, objective=1, num_class=3, n_estimators=3, min_data_in_leaf=5).save()
    hdr = list(struct.unpack_from("7i", blob, 0))          # magic, version, objective, num_class, K, n_iter, F

    def with_header(**kw):
        h = list(hdr)
        for k, v in kw.items():
            h[dict(objective=2, num_class=3, K=4, n_iter=5)[k]] = v
        return struct.pack("7i", *h) + blob[28:]

    for bad in (with_header(objective=7), with_header(objective=-1), with_header(num_class=9), with_header(num_class=0),
                with_header(objective=0), with_header(objective=2), with_header(n_iter=1 << 28)):
        with pytest.raises(_native.RepairGbmError):
            _native.Model.load(bad)
    assert _native.Model.load(with_header()).save() == blob
