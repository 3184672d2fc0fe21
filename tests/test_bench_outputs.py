"""bench.py --dump-outputs / --full: the writer of the last timed step's
outputs (whole when small, a fixed seeded sample of rows when large, float32)
on the CPU, and on the GPU one plain and one --full run of the same small
arguments: the plain line carries the headline keys only, the --full line the
root check and roofline too, and both write the same level array and root --
the oracle's for the same splitmix64 values and BE64 keys."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_small_arrays_whole_float32(tmp_path):
    b = _bench()
    rng = np.random.default_rng(1)
    lv = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    st = np.arange(-3, 4, dtype=np.int32).reshape(7, 1)
    b.dump_outputs(str(tmp_path / "o"), {"levels": lv, "status": st})
    got = np.load(tmp_path / "o" / "levels.npy")
    assert got.dtype == np.float32 and np.array_equal(got, lv.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "o" / "status.npy"), st.astype(np.float32))


def test_dump_outputs_large_array_fixed_sample_within_budget(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BUDGET", 2 * 4096 * 32 * 4)  # 4096 rows for each of 2 outputs
    rows = 50000
    x = np.random.default_rng(2).integers(0, 256, (rows, 32), dtype=np.uint8)
    y = x.copy()
    y[::7] ^= 1
    b.dump_outputs(str(tmp_path / "a"), {"levels": x, "root": x[-1:]})
    b.dump_outputs(str(tmp_path / "b"), {"levels": y, "root": y[-1:]})
    ga, gb = np.load(tmp_path / "a" / "levels.npy"), np.load(tmp_path / "b" / "levels.npy")
    assert ga.shape == gb.shape and ga.shape[1] == 32 and ga.dtype == np.float32
    assert 4096 - 1280 <= ga.shape[0] <= 4096 and ga.nbytes + 32 * 4 <= b.DUMP_BUDGET
    assert np.array_equal(ga[:256], x[:256].astype(np.float32))
    # the same rows of both arrays: the sample differs exactly where the arrays do
    rows_a = {r.tobytes() for r in x.astype(np.float32)}
    assert all(r.tobytes() in rows_a for r in ga)
    assert np.array_equal(ga[-1024:], x[-1024:].astype(np.float32))  # the top of the levels
    diff = (ga != gb).any(axis=1)
    assert 0 < diff.sum() < len(diff)
    # a torch tensor is sampled the same way
    import torch
    b.dump_outputs(str(tmp_path / "c"), {"levels": torch.from_numpy(x), "root": x[-1:]})
    assert np.array_equal(np.load(tmp_path / "c" / "levels.npy"), ga)
    # and with the budget shared by 2 processes each writes half as many rows
    b.dump_outputs(str(tmp_path / "d"), {"levels": x, "root": x[-1:]}, share=2)
    assert 2048 - 1280 <= np.load(tmp_path / "d" / "levels.npy").shape[0] <= 2048


N_SMALL = 5000  # not a power of two, several workgroups, below every size threshold
ARGS = ["--gpus", "1", "--steps", "4", "--warmup", "1", "--prewarm", "0",
        "--entries", str(N_SMALL)]


def _run(extra, out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra +
                       ["--dump-outputs", out_dir], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_write_the_oracles_tree(orc, tmp_path):
    b = _bench()
    plain = _run([], str(tmp_path / "plain"))
    full = _run(["--full", "--no-cpu-baseline"], str(tmp_path / "full"))
    for line in (plain, full):
        assert all(k in line for k in HEADLINE)
        assert line["steps"] == 4 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert plain["full"] is False
    for k in ("root_check", "roofline", "single_build", "cpu_baseline"):
        assert k not in plain
    assert full["full"] is True and full["root_check"]["ok"] is True
    assert "roofline" in full and "single_build" in full
    keys, vals = b.shard_block(orc, 2, 0, 0, N_SMALL, b.VAL_LEN)
    _, lv, root = orc.build_entries_fixed(1, keys, vals, nthreads=2)
    want_lv = np.asarray(lv).reshape(-1, 32).astype(np.float32)
    want_root = np.frombuffer(root, np.uint8).astype(np.float32).reshape(1, 32)
    for d in ("plain", "full"):
        assert sorted(os.listdir(tmp_path / d)) == ["levels.npy", "root.npy"]
        got_root, got_lv = np.load(tmp_path / d / "root.npy"), np.load(tmp_path / d / "levels.npy")
        assert got_root.dtype == got_lv.dtype == np.float32
        assert np.array_equal(got_root, want_root)
        assert np.array_equal(got_lv, want_lv)
