"""Generate tests/golden/reference_metrics.npz by running the REFERENCE's own
calculate_metrics and metrics_one_linear (training.py) on random arrays.

Run where the reference checkout is available (see make_golden.py, whose in-memory import
stubs this script uses: nothing is written to disk and nothing from the reference is
copied):

    python tests/golden/make_golden_metrics.py

Three cases of float64 labels / baseline / predictions [examples, x, channel]:
conservative Burgers (the default equation) with 3 channels, KS with 4, and KS with 6, the
last two of them integrated heads.  Per case
the inputs, the 'loss...' entries handed in, the keys and values of the returned dict and
the one-line summary are stored (no pickled objects).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

CASES = (('ConservativeBurgersEquation', 3, 5, 16), ('KSEquation', 4, 7, 12),
         ('KSEquation', 6, 4, 24))


def main():
  make_golden.install_stubs()
  if make_golden.REFERENCE_ROOT not in sys.path:
    sys.path.insert(0, make_golden.REFERENCE_ROOT)
  from pde_superresolution import equations, training
  rng = np.random.RandomState(20261018)
  out = {'num_cases': np.array(len(CASES))}
  for i, (name, channels, examples, points) in enumerate(CASES):
    equation_type = getattr(equations, name)
    labels = rng.standard_normal((examples, points, channels))
    scale = 10.0 ** rng.uniform(-2, 1, size=channels)
    baseline = labels + scale * rng.standard_normal(labels.shape)
    predictions = labels + 0.7 * scale * rng.standard_normal(labels.shape)
    # a few exact hits, so that safe_abs' epsilon is exercised
    predictions[0, :3, 0] = labels[0, :3, 0]
    baseline[1, :2, -1] = labels[1, :2, -1]
    data = {'labels': labels, 'baseline': baseline, 'predictions': predictions,
            'loss': np.float32(rng.uniform(0.1, 2.0)),
            'loss/space_derivatives': np.float32(rng.uniform(0.1, 2.0)),
            'loss/time_derivative': np.float32(rng.uniform(0.1, 2.0))}
    if channels > len(equation_type.DERIVATIVE_NAMES) + 1:
      data['loss/integrated_solution'] = np.float32(rng.uniform(0.1, 2.0))
    metrics = training.calculate_metrics(data, equation_type)
    line = training.metrics_one_linear(metrics)
    keys = sorted(metrics)
    prefix = 'case{}_'.format(i)
    out[prefix + 'equation'] = np.array(name)
    for key in ('labels', 'baseline', 'predictions'):
      out[prefix + key] = data[key]
    loss_keys = sorted(k for k in data if 'loss' in k)
    out[prefix + 'loss_keys'] = np.array(loss_keys)
    out[prefix + 'loss_values'] = np.array([data[k] for k in loss_keys], np.float32)
    out[prefix + 'keys'] = np.array(keys)
    out[prefix + 'values'] = np.array([float(metrics[k]) for k in keys], np.float64)
    out[prefix + 'one_line'] = np.array(line)
  path = os.path.join(HERE, 'reference_metrics.npz')
  np.savez_compressed(path, **out)
  print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
