"""Optimiser steps x replicas per second of rollout fine-tuning on one GPU, printed as one
JSON object: one training.RolloutPopulationTrainer.run(steps) on R replicas
(ddd_train_rollout_run: the replicas as a second grid dimension, four launches per step
whatever R is, no host read inside the call) against R sequential loops of
training.RolloutTrainer.step (ddd_train_rollout_loss_grad, the norm read on the host, the
clip in torch ops, torch.optim.Adam), by wall clock around a final synchronise.

Default Burgers net (5 taps x 32 filters, 3 layers) at N = 64, minibatches of 64 windows out
of 256, T = 32 model steps saved every 8, forced, clip_norm 1, R in {1, 4, 16}; the same
seeded windows and one minibatch order for every replica and both paths, replica r from init
seed r.  Per R, in a child process of its own: one warm-up of each path, then `rounds`
alternating rounds; the medians and the spread (max - min) / median of each path's rounds
are reported, and `ratio` = population over sequential.  Window starts are random-phase sine
waves and the targets synthetic perturbations of them (the step's cost does not depend on
their values).

  python profiles/tools/train_rollout_population_throughput.py [--steps 30] [--rounds 5]
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

REPLICAS = [1, 4, 16]
NUM_POINTS, BATCH, NUM_STEPS, SAVE_EVERY = 64, 64, 32, 8
LEARNING_RATE, CLIP_NORM = 1e-4, 1.0


def measure(replicas, steps, rounds, seed=0):
  import torch
  import ddd1d_amd
  from ddd1d_amd import equations, model as model_lib, training
  ddd1d_amd._lib.load_library()
  hp = ddd1d_amd.create_hparams('burgers', conservative=True,
                                equation_kwargs=json.dumps({'num_points': 4 * NUM_POINTS}),
                                resample_factor=4)
  _, eq = equations.from_hparams(hp)
  models = [model_lib.LearnedStencilModel(eq, hp, init_seed=seed + r) for r in range(replicas)]
  n = eq.grid.solution_num_points
  rows = 4 * BATCH
  saved = NUM_STEPS // SAVE_EVERY
  rs = np.random.RandomState(seed)
  x = eq.grid.solution_x
  y0 = np.sum(rs.uniform(-0.5, 0.5, (rows, 4, 1)) * np.sin(
      2 * np.pi * rs.randint(1, 4, (rows, 4, 1)) * x / eq.grid.period
      + rs.uniform(0, 2 * np.pi, (rows, 4, 1))), axis=1).astype(np.float32)
  targets = (y0[:, None, :] + 0.05 * rs.randn(rows, saved, n)).astype(np.float32)
  tables = model_lib.forcing_kernel_tables(
      model_lib.batched_forcing_parameters(range(rows), nparams=20), eq.grid)
  forcing = {key: torch.as_tensor(np.ascontiguousarray(value), device='cuda')
             for key, value in tables.items()}
  windows = training.RolloutWindows(
      torch.as_tensor(y0, device='cuda'), torch.as_tensor(targets, device='cuda'),
      torch.as_tensor(rs.uniform(0.0, 1.0, rows), device='cuda'), forcing, eq.time_step,
      NUM_STEPS, SAVE_EVERY, None, None)
  index = torch.as_tensor(rs.randint(0, rows, (steps, BATCH)).astype(np.int32), device='cuda')

  def sequential():
    trainers = [training.RolloutTrainer(model, hp, clip_norm=CLIP_NORM) for model in models]
    torch.cuda.synchronize()
    started = time.perf_counter()
    for trainer in trainers:
      for k in range(steps):
        trainer.step(windows, index[k], LEARNING_RATE)
    torch.cuda.synchronize()
    rate = steps * replicas / (time.perf_counter() - started)
    return rate, sum(trainer.skipped_steps for trainer in trainers)

  def population():
    trainer = training.RolloutPopulationTrainer(models, hp, clip_norm=CLIP_NORM)
    torch.cuda.synchronize()
    started = time.perf_counter()
    trainer.run(windows, steps, LEARNING_RATE, index)
    torch.cuda.synchronize()
    rate = steps * replicas / (time.perf_counter() - started)
    return rate, int(trainer.skipped_steps.sum())

  skipped = sequential()[1] + population()[1]
  seq_rates, pop_rates = [], []
  for _ in range(rounds):
    seq_rates.append(sequential()[0])
    pop_rates.append(population()[0])
  seq_median, pop_median = float(np.median(seq_rates)), float(np.median(pop_rates))
  return {
      'replicas': replicas, 'num_points': n, 'batch': BATCH, 'num_steps': NUM_STEPS,
      'save_every': SAVE_EVERY, 'opt_steps': steps, 'skipped_steps_in_warm_up': skipped,
      'step_loop_steps_replicas_per_s': seq_rates,
      'population_steps_replicas_per_s': pop_rates,
      'step_loop_median': seq_median, 'population_median': pop_median,
      'step_loop_spread': (max(seq_rates) - min(seq_rates)) / seq_median,
      'population_spread': (max(pop_rates) - min(pop_rates)) / pop_median,
      'ratio': pop_median / seq_median,
  }


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--steps', type=int, default=30)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--replicas', type=int, default=None,
                      help='one R in this process (the children)')
  args = parser.parse_args()
  if args.replicas is not None:
    print(json.dumps(measure(args.replicas, args.steps, args.rounds)))
    return
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('train_rollout_population_throughput.py needs a GPU')
  device = torch.cuda.get_device_name(0)
  started = time.time()
  rows = []
  for replicas in REPLICAS:
    done = subprocess.run(
        [sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--rounds',
         str(args.rounds), '--replicas', str(replicas)],
        capture_output=True, text=True, timeout=400)
    if done.returncode != 0:   # nothing more is started on the device after a failure
      raise SystemExit('R = {} failed ({}):\n{}'.format(replicas, done.returncode,
                                                       done.stderr[-2000:]))
    rows.append(json.loads(done.stdout.strip().splitlines()[-1]))
    sys.stderr.write('R = {}: {:.1f} / {:.1f} steps x replicas per s\n'.format(
        replicas, rows[-1]['population_median'], rows[-1]['step_loop_median']))
    sys.stderr.flush()
  print(json.dumps({'tool': 'train_rollout_population_throughput', 'device': device,
                    'rows': rows, 'wall_s': time.time() - started}))


if __name__ == '__main__':
  main()
