"""CPU: `repair_frame(.., want_details=True)` against tests/golden/repair_frame_pinned.json, recorded by tools/record_repair_frame_pinned.py
at the commit before the host side of the resident pipeline was split into `repair.frame_encoding` and phase functions -- not from the
code under test.  The cases (tests/repair_frame_pinned_cases.py) are the paths on which the encoding, the held current values and the
second pass used to share state: the frame must be equal cell for cell, every details key but the timings too, the models byte for byte
(digests of the saved blobs)."""
import json
import os

import numpy as np
import pytest

from tests import repair_frame_pinned_cases as C
from tests.helpers import GOLDEN


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "repair_frame_pinned.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(c.__name__ for c in C.CASES)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.__name__)
def test_result_equals_the_recorded_one(golden, case):
    got = json.loads(json.dumps(C.snapshot(*C.run(case))))
    want = golden[case.__name__]
    assert got["frame"] == want["frame"]
    assert sorted(got["details"]) == sorted(want["details"])
    for key in want["details"]:
        assert got["details"][key] == want["details"][key], key


def test_an_encoding_that_appends_without_re_ranking_fails(golden, monkeypatch):
    """The test is live: a `write` that appends a new value behind the last dictionary entry (its code is then not its rank among the
    column's values) gives another table, other models and another frame on the case that inserts `77 patients`."""
    from repair.frame_encoding import FrameEncoding

    def append_only(self, j, rows, values):
        for v in dict.fromkeys(values):
            if v not in list(self.dicts[j]):
                self.remaps[j] = np.append(self.remaps[j], np.int32(len(self.dicts[j])))
                self.dicts[j] = np.append(self.dicts[j], np.array([v], object))
            k = list(self.dicts[j]).index(v)
            at = np.asarray(rows, np.int64)[np.asarray(values, object) == v]
            self.indices[j, at] = int(np.flatnonzero(self.remaps[j] == k)[0])

    monkeypatch.setattr(FrameEncoding, "write", append_only)
    got = json.loads(json.dumps(C.snapshot(*C.run(C.regex_new_entry_and_a_model_cell))))
    assert got != golden["regex_new_entry_and_a_model_cell"]
