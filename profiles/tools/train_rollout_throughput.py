"""The gradient of a rollout loss on one GPU, one launch against the composed torch route,
written as one JSON object.  Default Burgers net (5 taps x 32 filters, 3 layers), N = 64,
512 windows, T = 8, 32 and 128 midpoint steps, every step saved, UNFORCED so that the two
routes compute the same thing.  Timed in one process, alternating:
  (a) one ddd_train_rollout_loss_grad call (csrc/train_rollout.hip): the forward sweep, the
      adjoint and the slab sum;
  (b) the same loss through model.differentiable_time_evolution (ddd_result_vjp per
      evaluation: 4 T kernel calls, 2 T slab sums) and torch autograd.
Device events around calls that end in a synchronise; two warm-up calls of each first; the
repetitions per window are chosen so that a window lasts about half a second; per row the
median over the rounds and their spread (min, max).  The two gradients are compared once
per row.

  python profiles/tools/train_rollout_throughput.py [--windows 512] [--steps 8,32,128]
      [--rounds 5] [--out profiles/train_rollout_throughput.json]
"""
import argparse
import ctypes
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


def measure(windows, steps, rounds, seed=0):
  hp = ddd1d_amd.create_hparams('burgers', conservative=False,
                                equation_kwargs=json.dumps({'num_points': 256}))
  _, eq = equations.from_hparams(hp)
  model = model_lib.LearnedStencilModel(eq, hp, init_seed=seed)
  n = eq.grid.solution_num_points
  rs = np.random.RandomState(seed)
  x = eq.grid.solution_x
  y = np.sum(rs.uniform(-0.5, 0.5, (windows, 4, 1)) * np.sin(
      2 * np.pi * rs.randint(1, 4, (windows, 4, 1)) * x / eq.grid.period
      + rs.uniform(0, 2 * np.pi, (windows, 4, 1))), axis=1).astype(np.float32)
  y = torch.as_tensor(y, device='cuda')
  targets = (y[:, None, :] + 0.1 * torch.as_tensor(
      rs.randn(windows, steps, n).astype(np.float32), device='cuda')).contiguous()
  step_weights = torch.full((steps,), 1.0 / steps, device='cuda')
  cfg = training._train_config(model)
  nullspace, bias = model_lib._vjp_tables(model)
  weights = torch.as_tensor(model_lib.model_weights(model), device='cuda')
  ws_bytes = _lib.load_library().ddd_train_rollout_workspace_bytes(
      ctypes.byref(cfg), windows, steps)
  workspace = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')

  def fused():
    return _lib.train_rollout_loss_grad(
        cfg, weights, y, targets, step_weights, steps, 1, eq.time_step, nullspace=nullspace,
        bias=bias, workspace=workspace)[1]

  def composed():
    w = weights.detach().requires_grad_(True)
    traj = model_lib.differentiable_time_evolution(y, model, steps, w)   # [window, x, T]
    means = ((traj.permute(0, 2, 1) - targets) ** 2).mean(dim=(0, 2))
    (step_weights * means).sum().backward()
    return w.grad

  for fn in (fused, composed, fused, composed):   # warm-up
    fn()
  g_fused, g_composed = fused(), composed()
  difference = ((g_fused - g_composed).norm() / g_composed.norm()).item()
  reps = {name: int(min(50, max(2, np.ceil(500.0 / timed(fn, 2)))))
          for name, fn in (('fused', fused), ('composed', composed))}
  fused_ms, composed_ms = [], []
  for _ in range(rounds):   # alternating
    fused_ms.append(timed(fused, reps['fused']))
    composed_ms.append(timed(composed, reps['composed']))
  return {
      'windows': windows, 'num_points': n, 'num_steps': steps, 'reps': reps,
      'workspace_mib': ws_bytes / 2.0 ** 20,
      'fused_ms': fused_ms, 'composed_ms': composed_ms,
      'fused_ms_median': float(np.median(fused_ms)),
      'fused_ms_spread': [float(min(fused_ms)), float(max(fused_ms))],
      'composed_ms_median': float(np.median(composed_ms)),
      'composed_ms_spread': [float(min(composed_ms)), float(max(composed_ms))],
      'composed_over_fused': float(np.median(composed_ms) / np.median(fused_ms)),
      'gradient_rel_difference': difference,
  }


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--windows', type=int, default=512)
  parser.add_argument('--steps', default='8,32,128')
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=os.path.join(ROOT, 'profiles',
                                                    'train_rollout_throughput.json'))
  args = parser.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('train_rollout_throughput.py needs a GPU')
  _lib.load_library()
  started = time.time()
  rows = [measure(args.windows, int(t), args.rounds) for t in args.steps.split(',')]
  result = {'tool': 'train_rollout_throughput', 'device': torch.cuda.get_device_name(0),
            'rows': rows, 'wall_s': time.time() - started}
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1)
    f.write('\n')
  print(json.dumps(result))


if __name__ == '__main__':
  main()
