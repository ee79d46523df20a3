"""bench.py at --gpus 1 as a subprocess: --steps is the number of timed steps and
--dump-outputs writes what the timed path returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu


def test_bench_times_exactly_steps_and_dumps_the_final_states(tmp_path):
  steps, batch = 7, 256
  out_dir = str(tmp_path / 'outputs')
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
                        '--steps', str(steps), '--warmup', '2', '--batch', str(batch),
                        '--secondary-batch', '0', '--configs', 'none', '--cpu-seconds', '0',
                        '--preheat-ms', '10', '--dump-outputs', out_dir],
                       capture_output=True, text=True, timeout=600)
  assert out.returncode == 0, out.stderr[-3000:]
  result = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
  assert result['steps'] == steps and result['reps'] == 1 and result['config']['finite']
  assert result['ms_per_step'] > 0
  assert abs(result['ms_per_step'] * steps - result['config']['timed_wall_ms']) < 1e-6
  assert os.listdir(out_dir) == ['final_states.npy']
  got = np.load(os.path.join(out_dir, 'final_states.npy'))
  # the same seeded workload through the same entry point, in this process
  import bench
  args = bench.parse_args(['--batch', str(batch), '--steps', str(steps)])
  eq, model, _, y0 = bench.build_workload(args, 0, batch)
  want = model.integrate_fixed(y0, steps, dt=eq.time_step, scheme='midpoint',
                               save_every=steps).cpu().numpy()
  assert got.dtype == np.float32 and got.shape == (1, batch, 64)
  np.testing.assert_array_equal(got, want)


def _bench_line(argv):
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + argv,
                       capture_output=True, text=True, timeout=600)
  assert out.returncode == 0, out.stderr[-3000:]
  return json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])


def test_plain_run_measures_the_headline_only():
  """Without --full the line carries the headline figure and nothing that needs
  runs of its own: no secondary batch, no extra configurations, no CPU baseline,
  no clock samples."""
  result = _bench_line(['--gpus', '1', '--steps', '7', '--warmup', '2', '--batch', '256',
                        '--preheat-ms', '10'])
  assert result['steps'] == 7 and result['reps'] == 1 and result['config']['finite']
  assert result['value'] > 0 and result['ms_per_step'] > 0
  assert result['config']['full'] is False
  for key in ('secondary', 'configs', 'cpu_baseline', 'clocks'):
    assert result[key] is None, key
  assert result['roofline']['kernel_ms_per_launch'] > 0


def test_full_run_keeps_the_extras():
  """--full adds the secondary batch, the chosen extra configurations and the
  CPU baseline to the same line."""
  result = _bench_line(['--gpus', '1', '--steps', '7', '--warmup', '2', '--batch', '256',
                        '--preheat-ms', '10', '--full', '--secondary-batch', '128',
                        '--configs', 'kdv_n64_b4096', '--config-timed-ms', '20',
                        '--cpu-seconds', '0.5'])
  assert result['config']['full'] is True and result['config']['finite']
  assert result['secondary']['batch_per_gpu'] == 128 and result['secondary']['value'] > 0
  kdv = result['configs']['kdv_n64_b4096']
  assert 'error' not in kdv and kdv['value'] > 0 and kdv['finite']
  assert result['cpu_baseline']['value'] > 0
