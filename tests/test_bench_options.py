"""bench.py's command line: a plain run is lean (`--full` adds every other leg) and `--dump-outputs DIR` writes what the
last timed step computed, the same from run to run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
DUMPED = ("A_values", "A_indices", "A_indptr", "b", "domain", "inactive_dofs", "checksums", "counts")


def _bench():
    sys.path.insert(0, str(ROOT))
    import bench
    return bench


def _parse(monkeypatch, *argv):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_is_the_default_and_full_is_an_option(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out", "--no-cpu")
    assert a.full is True and a.dump_outputs == "out" and a.no_cpu is True
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_the_rank_job_inherits_full(monkeypatch):
    bench = _bench()
    a = _parse(monkeypatch, "--gpus", "2", "--full")
    assert "--full" in bench.launcher_command(a, port=1)
    assert "--full" not in bench.launcher_command(_parse(monkeypatch, "--gpus", "2"), port=1)


def test_dump_sample_positions_are_fixed_and_bounded():
    bench = _bench()
    assert np.array_equal(bench.sample_positions(10, 1), np.arange(10))
    n = 50 * bench.DUMP_SAMPLE
    p = bench.sample_positions(n, 3)
    assert p.size == bench.DUMP_SAMPLE and np.all(np.diff(p) >= 0) and p[0] >= 0 and p[-1] < n
    assert np.array_equal(p, bench.sample_positions(n, 3))
    assert not np.array_equal(p, bench.sample_positions(n, 4))
    # six sampled arrays in float64 (the classification in float32) + two short summaries stay under 64 MB
    assert 6 * 8 * bench.DUMP_SAMPLE + 8 * (6 + len(bench.DUMP_COUNTS)) < 64 * 2 ** 20


def test_dump_outputs_refuses_more_than_one_gpu_before_any_work(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--dump-outputs", str(tmp_path / "d")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--gpus 1" in p.stderr
    assert not (tmp_path / "d").exists()


def _run_plain(out_dir):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--mesh", "16", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs_repeat(tmp_path):
    d1, d2 = tmp_path / "run1", tmp_path / "run2"
    line = _run_plain(d1)
    for k in LINE_KEYS:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "DOF/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - line["config"]["active_dofs"] / (1e-3 * line["ms_per_step"])) <= 1e-6 * line["value"]
    # nothing of --full: no profile, no secondary legs, no CPU baseline, no detail file
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["detail"] is None
    assert "secondary" not in line and "phases_ms" not in line

    files = {p.stem: np.load(p) for p in d1.glob("*.npy")}
    assert set(files) == set(DUMPED)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(p.stat().st_size for p in d1.glob("*.npy")) < 64 * 2 ** 20
    counts = dict(zip(_bench().DUMP_COUNTS, files["counts"]))
    assert counts["active_dofs"] == line["config"]["active_dofs"]
    # 16^3 is small enough to dump whole: the arrays have the step's sizes
    assert files["A_values"].size == files["A_indices"].size == counts["nnz"]
    assert files["b"].size == files["A_indptr"].size - 1 == 17 ** 3
    assert files["domain"].size == 6 * 16 ** 3 and set(np.unique(files["domain"])) <= {-1.0, 0.0, 1.0}
    assert files["inactive_dofs"].size == 17 ** 3 - counts["active_dofs"]
    assert files["A_indptr"][-1] == counts["nnz"]
    assert np.isclose(files["checksums"][0], files["A_values"].sum(), rtol=1e-12)

    _run_plain(d2)
    for name in DUMPED:
        a, b = files[name], np.load(d2 / f"{name}.npy")
        assert a.shape == b.shape, name
        np.testing.assert_allclose(b, a, rtol=1e-12, atol=1e-300, err_msg=name)
