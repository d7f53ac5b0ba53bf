"""bench.py's two kinds of run: a plain one does the headline steps and reports only what its timed region yields; --full
adds every other leg (per-kernel times, the opt-in arithmetic modes, the single-scale batch, one pair per call, the CPU
baseline, the 13-pattern parity check) to the same line."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

# the objects of the line that only a --full run fills in
FULL_ONLY = ("roofline_pyr", "kernels", "contracted_arithmetic", "tolerance_mode", "single_scale_batched", "one_pair_per_call",
             "cpu_baseline", "epe_vs_reference")


def _line(*args):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--pairs", "3",
           "--height", "120", "--width", "160", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_leaves_the_other_legs_to_full():
    plain = _line()
    full = _line("--full", "--no-live-traffic", "--cpu-sample-pairs", "1")
    for j in (plain, full):
        assert j["metric"] == "Mpix/s dense flow" and j["unit"] == "Mpix/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
        assert j["steps"] == 2 and j["warmup"] == 1
        # value: pixels of the timed steps over their time, whichever kind of run
        assert abs(j["value"] - 3 * 120 * 160 * 2 / (j["ms_per_step"] * 2e-3) / 1e6) <= 2e-3 * j["value"]
        assert j["whole_call"]["algorithmic_bytes_per_step"] > 0
    assert [k for k in FULL_ONLY if plain[k] is not None] == []
    assert [k for k in FULL_ONLY if k != "roofline_pyr" and not full[k]] == []
    e = full["epe_vs_reference"]
    assert e["digests_equal"] == 26 and e["max_mean_epe"] == 0.0
    assert full["tolerance_mode"]["fields_within_1e-4"] == full["tolerance_mode"]["fields"]
    # the headline steps compute the same flow either way
    assert plain["job_stats"] == full["job_stats"]
