"""Optimiser steps per second of the training loop on one GPU, printed as one JSON object:
`steps` x training.Trainer.step (one kernel call, a host read of the loss and
torch.optim.Adam per step) against one training.Trainer.run(steps) (ddd_train_run: every
step enqueued by one call, Adam fused into the slab sum, error_max decided on the
device), by wall clock around a final synchronise.

Default Burgers net (5 taps x 32 filters, 3 layers), the same seeded data and minibatch
order for both, at two sizes: the notebook's batch shape (N = 32, 2 048 rows per step)
and N = 64 with 512 rows; each with error_max = 0 and with an error_max that clips a
head.  Per case, in a child process of its own: one warm-up of each loop, then three
alternating rounds; the medians and the spread (max - min) / median of the `step` rounds
are reported.  Inputs are random-phase sine waves; labels / baseline are synthetic
perturbations (the step's cost does not depend on their values).

  python profiles/tools/train_loop_throughput.py [--steps 200] [--rounds 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CASES = [   # (coarse points N, rows per step)
    (32, 2048),
    (64, 512),
]


def measure(num_points, batch, clip, steps, rounds, seed=0):
  import torch
  import ddd1d_amd
  from ddd1d_amd import equations, model as model_lib, training
  ddd1d_amd._lib.load_library()
  hp = ddd1d_amd.create_hparams('burgers', conservative=False,
                                equation_kwargs=json.dumps({'num_points': 4 * num_points}),
                                resample_factor=4)
  _, eq = equations.from_hparams(hp)
  model = model_lib.LearnedStencilModel(eq, hp, init_seed=seed)
  n = eq.grid.solution_num_points
  rows = 4 * batch
  rs = np.random.RandomState(seed)
  x = eq.grid.solution_x
  y = np.sum(rs.uniform(-0.5, 0.5, (rows, 4, 1)) * np.sin(
      2 * np.pi * rs.randint(1, 4, (rows, 4, 1)) * x / eq.grid.period
      + rs.uniform(0, 2 * np.pi, (rows, 4, 1))), axis=1).astype(np.float32)
  y = torch.as_tensor(y, device='cuda')
  heads = len(eq.DERIVATIVE_ORDERS) + 1
  labels = torch.as_tensor(rs.randn(rows, n, heads).astype(np.float32), device='cuda')
  baseline = labels + 0.1 * torch.as_tensor(rs.randn(rows, n, heads).astype(np.float32),
                                            device='cuda')
  hp.error_scale = [1.0] * (2 * heads)
  hp.error_floor = [1e-3] * heads
  hp.learning_rates = [1e-4]
  hp.learning_stops = [10 ** 9]
  data = model_lib.DeviceDataset(y, labels, baseline, batch, repeat=True, seed=seed)
  index = torch.as_tensor(rs.randint(0, rows, (steps, batch)).astype(np.int32), device='cuda')
  each = [index[k].contiguous() for k in range(steps)]
  clipped = None
  if clip:   # between the entries of the first step's loss: some clipped, some not
    first, _, _ = training.Trainer(model, hp).loss_and_grad(data, each[0], want_grad=False)
    hp.error_max = float(np.median(first))
    clipped = int((first >= hp.error_max).sum())

  def step_loop():
    trainer = training.Trainer(model, hp)
    torch.cuda.synchronize()
    started = time.perf_counter()
    for k in range(steps):
      trainer.step(data, each[k])
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - started)

  def run_loop():
    trainer = training.Trainer(model, hp)
    torch.cuda.synchronize()
    started = time.perf_counter()
    trainer.run(data, steps, index)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - started)

  step_loop()
  run_loop()
  step_rates, run_rates = [], []
  for _ in range(rounds):
    step_rates.append(step_loop())
    run_rates.append(run_loop())
  step_median, run_median = float(np.median(step_rates)), float(np.median(run_rates))
  return {
      'num_points': n, 'batch': batch, 'error_max': float(hp.error_max or 0.0),
      'clipped_entries_at_step_0': clipped, 'steps': steps,
      'step_steps_per_s': step_rates, 'run_steps_per_s': run_rates,
      'step_median': step_median, 'run_median': run_median,
      'step_spread': (max(step_rates) - min(step_rates)) / step_median,
      'run_over_step': run_median / step_median,
  }


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--steps', type=int, default=200)
  parser.add_argument('--rounds', type=int, default=3)
  parser.add_argument('--case', default=None,
                      help='N,batch,clip: one case in this process (the children)')
  args = parser.parse_args()
  if args.case is not None:
    num_points, batch, clip = (int(v) for v in args.case.split(','))
    print(json.dumps(measure(num_points, batch, bool(clip), args.steps, args.rounds)))
    return
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('train_loop_throughput.py needs a GPU')
  device = torch.cuda.get_device_name(0)
  started = time.time()
  rows = []
  for num_points, batch in CASES:
    for clip in (0, 1):
      done = subprocess.run(
          [sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--rounds',
           str(args.rounds), '--case', '{},{},{}'.format(num_points, batch, clip)],
          capture_output=True, text=True, timeout=300)
      if done.returncode != 0:   # nothing more is started on the device after a failure
        raise SystemExit('case {} {} {} failed ({}):\n{}'.format(
            num_points, batch, clip, done.returncode, done.stderr[-2000:]))
      rows.append(json.loads(done.stdout.strip().splitlines()[-1]))
  print(json.dumps({'tool': 'train_loop_throughput', 'device': device, 'rows': rows,
                    'wall_s': time.time() - started}))


if __name__ == '__main__':
  main()
