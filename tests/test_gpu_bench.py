"""A plain `bench.py` run (no --full) on the GPU: it times exactly --steps iterations, prints the line with the contract's keys and
nothing beyond the headline, and with --dump-outputs writes what the timed call returned in its last step - the same arrays, bit for
bit, when it is run again with the same arguments (the suite pins the exact E-step: tests/conftest.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir, steps):
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1',
                           '--workload', 'em_20k_10k_64', '--dump-outputs', str(out_dir)],
                          cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    lines = [ln for ln in done.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, done.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_dumps_the_same_outputs_again(tmp_path):
    first, again = _plain_run(tmp_path / 'a', 3), _plain_run(tmp_path / 'b', 3)
    for line in (first, again):
        for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'config'):
            assert key in line, key
        assert line['steps'] == 3 and line['warmup'] == 1 and line['unit'] == 'barcodes/s' and line['higher_is_better'] is True
        assert line['value'] == pytest.approx(20_000 * 1e3 / line['ms_per_step'], rel=1e-3)
        assert line['roofline'] is None and line['cpu_baseline'] is None
        assert 'exact_mode_ms_per_step' not in line and 'kernel_ms' not in line and 'details' not in line
    probs = np.load(tmp_path / 'a' / 'posteriors.npy')
    addition = np.load(tmp_path / 'a' / 'genotype_addition.npy')
    assert probs.dtype == addition.dtype == np.float32
    assert probs.shape == (20_000, 64) and addition.shape == (20_000, 64)   # (both under their share of the 64 MB: not sampled)
    assert np.all(np.abs(probs.sum(axis=1, dtype=np.float64) - 1) < 1e-4) and np.all(np.isfinite(addition))
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(os.listdir(tmp_path / 'b'))
    for name in os.listdir(tmp_path / 'a'):
        assert np.array_equal(np.load(tmp_path / 'a' / name), np.load(tmp_path / 'b' / name)), name
