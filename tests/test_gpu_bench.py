"""bench.py's plain run: exactly --steps timed steps, the headline line alone, and --dump-outputs with the last timed step's loss
and parameters -- the same arrays for the same arguments (the step is bitwise deterministic).  The --full legs are exercised by
tests/test_gpu_rccl.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PERSONS, ITEMS, STEPS = 100_000, 1000, 3


def _plain_bench(dump_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', '1',
           '--persons', str(PERSONS), '--items', str(ITEMS), '--dump-outputs', str(dump_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_times_the_steps_asked_for_and_dumps_the_last_step(tmp_path):
    dirs = [tmp_path / 'run0', tmp_path / 'run1']
    for d in dirs:
        line = _plain_bench(d)
        assert line['steps'] == STEPS and line['ms_per_step_blocks']['blocks'] == 1 and line['ms_per_step'] > 0
        assert line['unit'] == 'terms/s' and line['higher_is_better'] is True and line['dtype'].startswith('f32')
        assert abs(line['value'] - PERSONS * ITEMS / (line['ms_per_step'] * 1e-3)) < 1e-6 * line['value']
        assert not {'roofline', 'elbo_rel_err', 'extra', 'also', 'also_config2', 'format_p', 'cpu_baseline'} & set(line)
        loss = np.load(d / 'loss.npy')
        assert loss.dtype == np.float32 and loss.shape == ()
        assert float(loss) / (PERSONS * ITEMS) == pytest.approx(line['config']['final_loss_per_term'], rel=1e-12)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {'loss.npy', 'item_encoder.mu_lookup.weight.npy', 'ability_encoder.mlp.0.weight.npy'} <= set(names)
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
