"""Loss and gradient through time on one GPU, fused against composed, printed as one JSON
object.  Default Burgers net (5 taps x 32 filters, 3 layers), N = 64, num_time_steps
T = 1 and 4, batches of 512 and 8192 samples.  Timed in one process, alternating:
  (a) one ddd_train_unrolled_loss_grad call (csrc/train_unrolled.hip): every head's loss
      and the weight gradient in one launch plus the slab sum;
  (b) the same loss and gradient composed from model.differentiable_result +
      model.differentiable_time_evolution (ddd_result_vjp per evaluation) and torch
      autograd: 4 T + 2 kernel calls, 2 T + 1 slab sums and the torch glue between them.
Device events around calls that end in a synchronise, two warm-up calls of each first.
Inputs are random-phase sine waves; labels / baseline are synthetic perturbations (the
cost does not depend on their values).  The two gradients are compared once per row.

  python profiles/tools/train_unrolled_throughput.py [--batches 512,8192] [--steps 1,4]
      [--reps 20] [--rounds 3]
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


def measure(batch, steps, reps, rounds, seed=0):
  hp = ddd1d_amd.create_hparams('burgers', conservative=False, num_time_steps=steps,
                                equation_kwargs=json.dumps({'num_points': 256}))
  _, eq = equations.from_hparams(hp)
  model = model_lib.LearnedStencilModel(eq, hp, init_seed=seed)
  n = eq.grid.solution_num_points
  rs = np.random.RandomState(seed)
  x = eq.grid.solution_x
  y = np.sum(rs.uniform(-0.5, 0.5, (batch, 4, 1)) * np.sin(
      2 * np.pi * rs.randint(1, 4, (batch, 4, 1)) * x / eq.grid.period
      + rs.uniform(0, 2 * np.pi, (batch, 4, 1))), axis=1).astype(np.float32)
  y = torch.as_tensor(y, device='cuda')
  heads = len(eq.DERIVATIVE_ORDERS) + 1 + steps
  labels = torch.as_tensor(rs.randn(batch, n, heads).astype(np.float32), device='cuda')
  baseline = labels + 0.1 * torch.as_tensor(rs.randn(batch, n, heads).astype(np.float32),
                                            device='cuda')
  floor = np.full(heads, 1e-3)
  coef_abs = rs.uniform(0.5, 1.5, heads)
  coef_rel = rs.uniform(0.1, 0.3, heads)
  cfg = training._train_config(model)
  nullspace, bias = model_lib._vjp_tables(model)
  weights = torch.as_tensor(model_lib.model_weights(model), device='cuda')
  ws_bytes = _lib.load_library().ddd_train_unrolled_workspace_bytes(
      ctypes.byref(cfg), batch, steps)
  workspace = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')

  def fused():
    return _lib.train_unrolled_loss_grad(
        cfg, weights, y, labels, baseline, floor, coef_abs, coef_rel, steps, eq.time_step,
        nullspace=nullspace, bias=bias, workspace=workspace)[1]

  consts = [torch.as_tensor(v, dtype=torch.float32, device='cuda')
            for v in (floor, coef_abs, coef_rel)]

  def composed():
    w = weights.detach().requires_grad_(True)
    pred = torch.cat([model_lib.differentiable_result(y, model, w),
                      model_lib.differentiable_time_evolution(y, model, steps, w)], dim=-1)
    me = (labels - pred) ** 2
    rel = me / ((labels - baseline) ** 2 + consts[0])
    loss = (consts[1] * me.mean(dim=(0, 1))).sum() + (consts[2] * rel.mean(dim=(0, 1))).sum()
    loss.backward()
    return w.grad

  for fn in (fused, composed, fused, composed):   # warm-up
    fn()
  g_fused, g_composed = fused(), composed()
  difference = ((g_fused - g_composed).norm() / g_composed.norm()).item()
  fused_ms, composed_ms = [], []
  for _ in range(rounds):   # alternating
    fused_ms.append(timed(fused, reps))
    composed_ms.append(timed(composed, reps))
  return {
      'batch': batch, 'num_points': n, 'num_time_steps': steps,
      'fused_ms': fused_ms, 'composed_ms': composed_ms,
      'fused_ms_median': float(np.median(fused_ms)),
      'composed_ms_median': float(np.median(composed_ms)),
      'composed_over_fused': float(np.median(composed_ms) / np.median(fused_ms)),
      'gradient_rel_difference': difference,
  }


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--batches', default='512,8192')
  parser.add_argument('--steps', default='1,4')
  parser.add_argument('--reps', type=int, default=20)
  parser.add_argument('--rounds', type=int, default=3)
  args = parser.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('train_unrolled_throughput.py needs a GPU')
  _lib.load_library()
  started = time.time()
  rows = [measure(int(b), int(t), args.reps, args.rounds)
          for t in args.steps.split(',') for b in args.batches.split(',')]
  print(json.dumps({'tool': 'train_unrolled_throughput',
                    'device': torch.cuda.get_device_name(0), 'rows': rows,
                    'wall_s': time.time() - started}))


if __name__ == '__main__':
  main()
