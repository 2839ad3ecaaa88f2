"""bench.py --dump-outputs / --full: the host-side logic (no GPU)."""
import json
import os

import numpy as np
import pytest


def _payload(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy"))


@pytest.fixture(scope="module")
def bench():
    # bench.py points MIOpen at its own find database when it is imported; that setting belongs to a
    # bench process, not to the rest of the test session
    had = os.environ.get("MIOPEN_USER_DB_PATH")
    import bench as mod
    if had is None:
        os.environ.pop("MIOPEN_USER_DB_PATH", None)
    return mod


def test_flags_default_off(bench):
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_whole(bench, tmp_path):
    rs = np.random.RandomState(0)
    maps = rs.standard_normal((3, 7, 5))
    mel, coeffs = rs.standard_normal((3, 4)).astype(np.float32), [rs.standard_normal((3, n)) for n in (2, 9)]
    d = str(tmp_path / "single")
    bench.dump_outputs(maps, d)
    got = np.load(os.path.join(d, "out0.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, maps)
    d = str(tmp_path / "tuple")
    bench.dump_outputs((mel, coeffs), d)
    assert np.load(os.path.join(d, "out0.npy")).dtype == np.float32
    assert np.array_equal(np.load(os.path.join(d, "out0.npy")), mel)
    for j, c in enumerate(coeffs):
        assert np.array_equal(np.load(os.path.join(d, "out1_%d.npy" % j)), c)
    index = json.load(open(os.path.join(d, "index.json")))
    assert sorted(index) == ["out0", "out1_0", "out1_1"] and not any(v["sampled"] for v in index.values())


def test_dump_sampled_is_fixed_and_within_budget(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40000)
    rs = np.random.RandomState(1)
    out = (rs.standard_normal((11, 1001)), [rs.standard_normal((11, 333)).astype(np.float32)])
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(out, a)
    bench.dump_outputs(out, b)
    index = json.load(open(os.path.join(a, "index.json")))
    for k, (name, full) in enumerate((("out0", out[0]), ("out1_0", out[1][0]))):
        u, v = np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy"))
        assert u.dtype == full.dtype and np.array_equal(u, v)            # the same sample every time
        idx = np.sort(np.random.RandomState(bench.DUMP_SEED + k).choice(full.size, u.size, replace=False))
        assert np.array_equal(u, full.reshape(-1)[idx])                     # and the documented one
        assert index[name]["sampled"] and index[name]["full_shape"] == list(full.shape)
    assert 0.9 * 40000 <= sum(np.load(os.path.join(a, n + ".npy")).nbytes for n in index) <= 40000
    assert _payload(a) <= 40000 + 2 * 128
