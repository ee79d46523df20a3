"""Optimiser steps x replicas per second of replica-population training on one GPU, printed
as one JSON object: one training.PopulationTrainer.run(steps) on R replicas
(ddd_train_population_run: the replicas as a second grid dimension, two launches per step
whatever R is) against R sequential training.Trainer.run(steps) calls on the same stream
(ddd_train_run, the path before populations existed), by wall clock around a final
synchronise.

Default Burgers net (5 taps x 32 filters, 3 layers) at N = 64, batch 128, 200 steps,
R in {1, 2, 4, 8, 16}; the same seeded data and one minibatch order for every replica and
both paths, replica r from init seed r.  Per R, in a child process of its own: one warm-up
of each path, then `rounds` alternating rounds; the medians and the spread
(max - min) / median of each path's rounds are reported, and `ratio` = population over
sequential.  The child also checks that replica 0 of the population run ends on the bits
of its sequential run.  Inputs are random-phase sine waves; labels / baseline are
synthetic perturbations (the step's cost does not depend on their values).

  python profiles/tools/train_population_throughput.py [--steps 200] [--rounds 5]
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

REPLICAS = [1, 2, 4, 8, 16]
NUM_POINTS, BATCH = 64, 128


def measure(replicas, steps, rounds, seed=0):
  import torch
  import ddd1d_amd
  from ddd1d_amd import equations, model as model_lib, training
  ddd1d_amd._lib.load_library()
  hp = ddd1d_amd.create_hparams('burgers', conservative=False,
                                equation_kwargs=json.dumps({'num_points': 4 * NUM_POINTS}),
                                resample_factor=4)
  _, eq = equations.from_hparams(hp)
  models = [model_lib.LearnedStencilModel(eq, hp, init_seed=seed + r) for r in range(replicas)]
  n = eq.grid.solution_num_points
  rows = 4 * BATCH
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
  data = model_lib.DeviceDataset(y, labels, baseline, BATCH, repeat=True, seed=seed)
  index = torch.as_tensor(rs.randint(0, rows, (steps, BATCH)).astype(np.int32), device='cuda')

  def sequential():
    trainers = [training.Trainer(model, hp) for model in models]
    torch.cuda.synchronize()
    started = time.perf_counter()
    for trainer in trainers:
      trainer.run(data, steps, index)
    torch.cuda.synchronize()
    return steps * replicas / (time.perf_counter() - started), trainers[0].weights.detach()

  def population():
    trainer = training.PopulationTrainer(models, hp)
    torch.cuda.synchronize()
    started = time.perf_counter()
    trainer.run(data, steps, index)
    torch.cuda.synchronize()
    return steps * replicas / (time.perf_counter() - started), trainer.weights[0]

  _, want = sequential()
  _, got = population()
  same_bits = bool(torch.equal(got, want))
  seq_rates, pop_rates = [], []
  for _ in range(rounds):
    seq_rates.append(sequential()[0])
    pop_rates.append(population()[0])
  seq_median, pop_median = float(np.median(seq_rates)), float(np.median(pop_rates))
  return {
      'replicas': replicas, 'num_points': n, 'batch': BATCH, 'steps': steps,
      'replica_0_same_bits': same_bits,
      'sequential_steps_replicas_per_s': seq_rates,
      'population_steps_replicas_per_s': pop_rates,
      'sequential_median': seq_median, 'population_median': pop_median,
      'sequential_spread': (max(seq_rates) - min(seq_rates)) / seq_median,
      'population_spread': (max(pop_rates) - min(pop_rates)) / pop_median,
      'ratio': pop_median / seq_median,
  }


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--steps', type=int, default=200)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--replicas', type=int, default=None,
                      help='one R in this process (the children)')
  args = parser.parse_args()
  if args.replicas is not None:
    print(json.dumps(measure(args.replicas, args.steps, args.rounds)))
    return
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('train_population_throughput.py needs a GPU')
  device = torch.cuda.get_device_name(0)
  started = time.time()
  rows = []
  for replicas in REPLICAS:
    done = subprocess.run(
        [sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--rounds',
         str(args.rounds), '--replicas', str(replicas)],
        capture_output=True, text=True, timeout=300)
    if done.returncode != 0:   # nothing more is started on the device after a failure
      raise SystemExit('R = {} failed ({}):\n{}'.format(replicas, done.returncode,
                                                       done.stderr[-2000:]))
    rows.append(json.loads(done.stdout.strip().splitlines()[-1]))
  print(json.dumps({'tool': 'train_population_throughput', 'device': device, 'rows': rows,
                    'wall_s': time.time() - started}))


if __name__ == '__main__':
  main()
