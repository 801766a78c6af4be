"""CPU: bench.py's command line and what --dump-outputs writes (the GPU run itself is not exercised here)."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--full" in out and "--dump-outputs" in out


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr


def _fake_result(targets, dirty_rows, model_bytes, seed):
    g = np.random.default_rng(seed)
    return {"labels": g.integers(0, 64, (len(targets), dirty_rows), dtype=np.int32), "probs": g.random((len(targets), dirty_rows)),
            "models": {t: g.integers(0, 256, model_bytes, dtype=np.uint8).tobytes() for t in targets}}


def test_dump_outputs_is_bounded_typed_and_repeatable(tmp_path):
    targets = list(range(16))
    res = _fake_result(targets, 200_000, 700_000, seed=3)     # 38 MB of cells, 11 MB of models: both above their share -> sampled
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, targets)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["labels.npy", "models.npy", "probs.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    lab, prob, mod = (np.load(tmp_path / "a" / n) for n in ("labels.npy", "probs.npy", "models.npy"))
    assert lab.dtype == np.float32 and prob.dtype == np.float64 and mod.dtype == np.float32
    assert lab.shape == prob.shape and lab.shape[0] == len(targets) and lab.shape[1] < 200_000
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    # the sample is of the returned arrays themselves: the same columns of labels and probabilities
    cols = bench._sample(200_000, lab.shape[1])
    assert np.array_equal(lab, res["labels"][:, cols]) and np.array_equal(prob, res["probs"][:, cols])


def test_dump_outputs_small_job_is_written_whole(tmp_path):
    targets = [0, 3]
    res = _fake_result(targets, 1000, 500, seed=4)
    bench.dump_outputs(str(tmp_path), res, targets)
    assert np.array_equal(np.load(tmp_path / "labels.npy"), res["labels"].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "probs.npy"), res["probs"])
    blob = np.frombuffer(res["models"][0] + res["models"][3], np.uint8)
    assert np.array_equal(np.load(tmp_path / "models.npy"), blob.astype(np.float32))
