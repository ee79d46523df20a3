"""The tangent-linear entry points on one GPU against the routes the library had before them,
written as one JSON object.  Default Burgers net (5 taps x 32 filters, 3 layers), N = 64.
Timed in one process, alternating:
  (i) the full Jacobian of the time derivative, 256 samples:
      (a) two ddd_result_jvp calls with 32 identity tangents each;
      (b) 64 ddd_result_vjp calls with one-hot cotangents of the time derivative.
  (ii) the tangent rollout, T = 64 midpoint steps, M = 8 tangents, 512 samples:
      (a) one ddd_tangent_rollout call;
      (b) the same recurrence composed from ddd_result_jvp calls in torch
          (model.tangent_time_evolution(fused=False)).
Device events around calls that end in a synchronise; two warm-up calls of each first; the
repetitions per window are chosen so that a window lasts about half a second; per row the
median over the rounds and their spread (min, max).  The two results are compared once per
row.

  python profiles/tools/jvp_throughput.py [--rounds 5] [--out profiles/jvp_throughput.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import ddd1d_amd   # noqa: E402
from ddd1d_amd import _lib, equations, model as model_lib, training   # noqa: E402


def timed(fn, reps):
  """Mean ms per call from device events (the caller has warmed fn up)."""
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / reps


def setup(samples, seed=0):
  hp = ddd1d_amd.create_hparams('burgers', conservative=False,
                                equation_kwargs=json.dumps({'num_points': 256}))
  _, eq = equations.from_hparams(hp)
  model = model_lib.LearnedStencilModel(eq, hp, init_seed=seed)
  rs = np.random.RandomState(seed)
  x = eq.grid.solution_x
  y = np.sum(rs.uniform(-0.5, 0.5, (samples, 4, 1)) * np.sin(
      2 * np.pi * rs.randint(1, 4, (samples, 4, 1)) * x / eq.grid.period
      + rs.uniform(0, 2 * np.pi, (samples, 4, 1))), axis=1).astype(np.float32)
  return model, torch.as_tensor(y, device='cuda'), rs


def alternate(new, old, rounds):
  for fn in (new, old, new, old):   # warm-up
    fn()
  reps = {name: int(min(50, max(2, np.ceil(500.0 / timed(fn, 2)))))
          for name, fn in (('new', new), ('old', old))}
  new_ms, old_ms = [], []
  for _ in range(rounds):
    new_ms.append(timed(new, reps['new']))
    old_ms.append(timed(old, reps['old']))
  return {
      'reps': reps, 'new_ms': new_ms, 'old_ms': old_ms,
      'new_ms_median': float(np.median(new_ms)),
      'new_ms_spread': [float(min(new_ms)), float(max(new_ms))],
      'old_ms_median': float(np.median(old_ms)),
      'old_ms_spread': [float(min(old_ms)), float(max(old_ms))],
      'old_over_new': float(np.median(old_ms) / np.median(new_ms)),
  }


def full_jacobian(samples, rounds):
  model, y, _ = setup(samples)
  n = y.shape[1]
  cfg = training._train_config(model)
  nullspace, bias = model_lib._vjp_tables(model)
  weights = torch.as_tensor(model_lib.model_weights(model), device='cuda')
  heads = cfg.num_derivatives + 1
  eye = torch.eye(n, device='cuda')
  halves = [eye[None, k:k + 32].expand(samples, 32, n).contiguous() for k in range(0, n, 32)]
  one_hot = torch.zeros(n, samples, n, heads, device='cuda')
  for i in range(n):
    one_hot[i, :, i, -1] = 1.0

  def by_jvp():   # [sample, i, j] = d f_i / d y_j
    cols = [_lib.result_jvp(cfg, weights, y, half, nullspace=nullspace, bias=bias,
                            want_predictions=False)[1][..., -1] for half in halves]
    return torch.cat(cols, dim=1).transpose(1, 2)

  def by_vjp():
    rows = [_lib.result_vjp(cfg, weights, y, one_hot[i], nullspace=nullspace, bias=bias,
                            want_grad_weights=False)[1] for i in range(n)]
    return torch.stack(rows, dim=1)

  row = alternate(by_jvp, by_vjp, rounds)
  a, b = by_jvp(), by_vjp()
  row.update(what='full Jacobian of the time derivative', samples=samples, num_points=n,
             new='2 ddd_result_jvp calls, 32 tangents each',
             old='{} ddd_result_vjp calls, one-hot cotangents'.format(n),
             rel_difference=((a - b).norm() / b.norm()).item())
  return row


def rollout(samples, steps, tangents, rounds):
  model, y, rs = setup(samples)
  n = y.shape[1]
  t0 = torch.as_tensor(rs.randn(samples, tangents, n).astype(np.float32), device='cuda')
  weights = torch.as_tensor(model_lib.model_weights(model), device='cuda')

  def fused():
    return model_lib.tangent_time_evolution(y, t0, model, steps, weights)

  def composed():
    return model_lib.tangent_time_evolution(y, t0, model, steps, weights, fused=False)

  row = alternate(fused, composed, rounds)
  a, b = fused(), composed()
  row.update(what='tangent rollout', samples=samples, num_points=n, num_steps=steps,
             tangents=tangents, new='one ddd_tangent_rollout call',
             old='{} ddd_result_jvp calls composed in torch'.format(2 * steps),
             rel_difference=max(((a[k] - b[k]).norm() / b[k].norm()).item() for k in (0, 1)))
  return row


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jvp_throughput.json'))
  args = parser.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('jvp_throughput.py needs a GPU')
  _lib.load_library()
  started = time.time()
  rows = [full_jacobian(256, args.rounds), rollout(512, 64, 8, args.rounds)]
  result = {'tool': 'jvp_throughput', 'device': torch.cuda.get_device_name(0),
            'rows': rows, 'wall_s': time.time() - started}
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1)
    f.write('\n')
  print(json.dumps(result))


if __name__ == '__main__':
  main()
