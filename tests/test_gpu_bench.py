"""`python bench.py --gpus 1 --steps K --warmup W` on its own: exactly K timed steps, the headline line only (the secondary
legs run with --full), and --dump-outputs DIR leaves the last timed step's results -- the same ones for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
SECONDARY = ('cpu_baseline', 'per_angle', 'virtual_ranks_8', 'virtual_ranks_16', 'kernel_sweep', 'driver', 'driver_per_angle',
             'driver_epoch')


def _bench(cwd, *args):
    # a child process: the bench holds its own GPU context
    r = subprocess.run([sys.executable, '-s', BENCH] + list(args), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().split('\n')[-1])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / ('out%d' % i)
        line = _bench(tmp_path, '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(d))
        assert line['steps'] == 3 and line['warmup'] == 1
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in line, k
        assert line['unit'] == 'probe-positions/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
        assert line['ms_per_step'] > 0 and np.isclose(line['value'], 32 * 1e3 / line['ms_per_step'], rtol=1e-9)
        assert not [k for k in SECONDARY if k in line]
        assert sorted(os.listdir(d)) == ['loss.npy', 'object_sample.npy']
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        loss, obj = np.load(d / 'loss.npy'), np.load(d / 'object_sample.npy')
        assert loss.dtype == np.float64 and loss.shape == (1,) and loss[0] == line['loss_last']
        assert obj.dtype == np.float32 and obj.size == -(-256 ** 3 * 2 // 7) and np.all(np.isfinite(obj))
        runs.append((loss, obj))
    # same arguments, same inputs: the two runs agree
    np.testing.assert_allclose(runs[1][0], runs[0][0], rtol=1e-6)
    np.testing.assert_allclose(runs[1][1], runs[0][1], rtol=1e-5, atol=1e-12)
