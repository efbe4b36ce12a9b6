"""bench.py --dump-outputs without a GPU: dump_outputs on host tensors of the shapes the workloads hand it.  Every value
comes back exactly from the float files; a batch too large for the size cap is written as one fixed, seeded sample of
rows, the same rows in every array and in every run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs(n, seed):
    g = np.random.default_rng(seed)
    return {"points": torch.from_numpy(g.integers(-2**63, 2**63 - 1, (n, 32), dtype=np.int64, endpoint=True)),
            "encodings": torch.from_numpy(g.integers(0, 255, (n, 56), dtype=np.uint8, endpoint=True)),
            "status": torch.from_numpy(g.integers(-2**31, 2**31 - 1, n, dtype=np.int32, endpoint=True))}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def _exact(files, outputs, rows):
    assert files["points"].dtype == np.float64 and files["encodings"].dtype == np.float32
    assert files["status"].dtype == np.float64
    pts = np.ascontiguousarray(files["points"].astype(np.uint32)).view(np.int64)
    assert (pts == outputs["points"].numpy()[rows]).all()
    assert (files["encodings"].astype(np.uint8) == outputs["encodings"].numpy()[rows]).all()
    assert (files["status"][:, 0].astype(np.int32) == outputs["status"].numpy()[rows]).all()


def test_a_small_batch_is_written_whole_and_exactly(tmp_path):
    n = 1000
    out = _outputs(n, 1)
    bench.dump_outputs(str(tmp_path), out, n, np, torch)
    files = _load(tmp_path)
    assert sorted(files) == ["encodings", "lanes", "points", "status"]
    assert (files["lanes"] == np.arange(n)).all()
    _exact(files, out, np.arange(n))


def test_a_large_batch_is_a_fixed_sample_under_the_cap(tmp_path):
    n = 1 << 17                                  # 2^17 rows x 808 bytes: above the cap
    out = _outputs(n, 2)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), out, n, np, torch)
    bench.dump_outputs(str(b), _outputs(n, 3), n, np, torch)
    size = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert size <= bench.DUMP_MAX_BYTES and size > bench.DUMP_MAX_BYTES * 0.9
    files = _load(a)
    rows = files["lanes"].astype(np.int64)
    assert 0 < len(rows) < n and (np.diff(rows) > 0).all() and rows[-1] < n
    assert (np.load(os.path.join(b, "lanes.npy")) == files["lanes"]).all()     # the same rows whatever the values
    _exact(files, out, rows)
