"""bench.py --dump-outputs: the flow of the last timed step as DIR/<name>.npy.

CPU: the writer itself (whole arrays, the seeded sample, shards of one output, the 64 MiB budget).
GPU: what bench.py dumps is the flow the oracle computes on the same seeded inputs, and the same from run to run.
"""
import importlib.util
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _flows(shape, seed):
    torch = pytest.importorskip("torch")
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def test_dump_whole_arrays(bench, tmp_path):
    u, v = _flows((3, 40, 50), 1)
    (tmp_path / "sample_index.npy").write_bytes(b"left over")
    assert bench.dump_outputs(str(tmp_path), {"u": [u], "v": [v]}) == ["u.npy", "v.npy"]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["u.npy", "v.npy"]
    for name, t in (("u", u), ("v", v)):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.numpy())


def test_dump_seeded_sample_of_sharded_output(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 500)
    u, v = _flows((4, 30, 70), 2)   # 8400 values per field: over the budget
    one, two = tmp_path / "one", tmp_path / "two"
    assert bench.dump_outputs(str(one), {"u": [u], "v": [v]}) == ["u.npy", "v.npy", "sample_index.npy"]
    # the same output held as uneven shards (one per GPU) gives the same files
    bench.dump_outputs(str(two), {"u": [u[:1], u[1:]], "v": [v[:3], v[3:]]})
    idx = np.load(one / "sample_index.npy")
    assert idx.dtype == np.float64 and idx.shape == (500,)
    i = idx.astype(np.int64)
    assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < u.numel()
    for name, t in (("u", u), ("v", v)):
        a = np.load(one / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.numpy().reshape(-1)[i])
        assert np.array_equal(a, np.load(two / f"{name}.npy"))
    assert np.array_equal(idx, np.load(two / "sample_index.npy"))


def test_dump_budget(bench):
    """the sample of a flow too large to dump whole stays within the 64 MiB the option promises"""
    assert bench.DUMP_SAMPLE * (4 + 4 + 8) <= bench.DUMP_BUDGET_BYTES == 64 * 2 ** 20


def _run_bench(out_dir, *args):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
           "--no-one-pair", "--no-live-traffic", "--no-parity", "--dump-outputs", str(out_dir), *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len([l for l in r.stdout.splitlines() if l.startswith("{")]) == 1, r.stdout[-2000:]


def _expected(oracle, H, W, pairs):
    """bench.py's inputs: synth_pair(H, W, i) for a few distinct i, tiled over the batch by pair index"""
    from oflk_synth import synth_pair

    n_distinct = 4 if H * W <= 1920 * 1080 else 2
    flows = [oracle.lucas_kanade_pyramidal(*synth_pair(H, W, pair_index=i), 3, 5, 3) for i in range(min(n_distinct, pairs))]
    return (np.stack([flows[b % n_distinct][0] for b in range(pairs)]),
            np.stack([flows[b % n_distinct][1] for b in range(pairs)]))


@pytest.mark.gpu
def test_bench_dumps_the_flow_whole(oracle, tmp_path):
    """a small workload: u.npy, v.npy are the whole [pairs][H][W] flow, equal to the oracle's, and equal from run to run"""
    _run_bench(tmp_path / "a", "--pairs", "5", "--height", "120", "--width", "160")
    _run_bench(tmp_path / "b", "--pairs", "5", "--height", "120", "--width", "160")
    eu, ev = _expected(oracle, 120, 160, 5)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["u.npy", "v.npy"]
    for name, e in (("u", eu), ("v", ev)):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (5, 120, 160)
        assert np.array_equal(a, e), name
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy")), name


@pytest.mark.gpu
def test_bench_dumps_a_seeded_sample_of_a_large_flow(oracle, tmp_path):
    """5 pairs of 1080p (83 MB of flow): a sample, at the recorded positions equal to the oracle's flow"""
    _run_bench(tmp_path, "--pairs", "5")
    i = np.load(tmp_path / "sample_index.npy").astype(np.int64)
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= 64 * 2 ** 20
    eu, ev = _expected(oracle, 1080, 1920, 5)
    for name, e in (("u", eu), ("v", ev)):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == i.shape
        assert np.array_equal(a, e.reshape(-1)[i]), name
