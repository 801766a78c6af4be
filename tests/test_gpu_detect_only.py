"""GPU: `RepairModel.run(detect_errors_only=True)` through the HIP engine (`error.detect_only.resident`: `pipeline.detect_frame`, the table's
cell set) against the value-space frame on the hospital fixture, and a 20 001-row order constraint without an EQ predicate, which the
value-space detector refuses and the resident table answers by sort and scan."""
import numpy as np
import pandas as pd
import pytest

from repair.errors import ConstraintErrorDetector, _to_sql_string, parse_constraint
from repair.model import RepairModel
from tests import dc_scan_cases as S
from tests.test_detect_only_cpu import ON, _hospital, _hospital_detectors, _model, _same
from tests.test_quality import HOSPITAL_TARGETS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("analysis", [False, True], ids=["plain", "domain_analysis"])
def test_hospital_equals_the_value_space_frame(analysis):
    from repair.engine import HipEngine
    df = _hospital()
    opts = {"error.domain_analysis.enabled": "true", "error.domain_threshold_beta": "0.5"} if analysis else {}
    targets = HOSPITAL_TARGETS + ["Sample"]
    slow = _model(df, _hospital_detectors(), targets, 80, **opts).run(detect_errors_only=True)
    m = _model(df, _hospital_detectors(), targets, 80, HipEngine(0), on=True, **opts)
    fast = m.run(detect_errors_only=True)
    assert m._last_detection_on_device is True and len(slow) > 0
    _same(slow, fast)
    info = m._last_resident_info
    assert info["constraint_routes"] == ["fd", "dc"] and ("weak_cells" in info) == analysis
    if analysis:
        assert info["weak_cells"] > 0 and info["noisy_cells"] - info["weak_cells"] == len(fast)


ORDER = "t1&t2&LT(t1.Salary,t2.Salary)&GT(t1.Tax,t2.Tax)"


def test_an_order_constraint_without_eq_on_20001_rows():
    from repair import dc_codes as DC
    from repair.engine import HipEngine
    from repair.frame_encoding import FrameEncoding
    n = 20001
    df = S.small_frame(n)

    def model(engine, **opts):
        m = RepairModel().setInput(df).setRowId("tid").setTargets(S.FRAME_TARGETS).setErrorDetectors([ConstraintErrorDetector(constraints=ORDER)])
        for key, val in opts.items():
            m = m.option(key, val)
        m._engine_override = engine
        return m

    with pytest.raises(ValueError, match="table too large"):                      # the value-space detector (on the CPU)
        model(None).run(detect_errors_only=True)
    m = model(HipEngine(0), **{ON: "true", "error.constraints.resident": "true", "error.constraints.order_scan": "true"})
    fast = m.run(detect_errors_only=True)
    assert m._last_detection_on_device is True and m._last_resident_info["constraint_routes"] == ["dc_scan"]
    # the cells of the numpy statement on the codes of the same encoding, with the values the frame holds there
    cols = [c for c in df.columns if c != "tid"]
    enc = FrameEncoding.of_frame(df, cols)
    codes = np.stack([np.where(enc.indices[j] >= 0, enc.remaps[j][np.maximum(enc.indices[j], 0)], -1) for j in range(len(cols))]).astype(np.int32)
    prog = DC.lower_constraint(parse_constraint(ORDER), cols, enc.dicts, {c: df[c].dtype for c in cols})
    assert prog["kind"] == "dc" and DC.scan_eligible(prog["preds"]) and not any(p[0] == "EQ" for p in prog["preds"])
    rows = S.scan_statement(codes, [max(len(d), 1) for d in enc.dicts], prog["preds"])
    assert 0 < len(rows) < n
    want = []
    for a in ("Salary", "Tax"):
        v = df[a].to_numpy()[rows]
        want.append(pd.DataFrame({"tid": df["tid"].to_numpy()[rows], "attribute": a,
                                  "current_value": np.asarray([None if np.isnan(x) else _to_sql_string(x) for x in v], object)}))
    _same(pd.concat(want, ignore_index=True), fast)
