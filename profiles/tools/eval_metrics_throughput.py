"""Evaluations of a replica population per second on one GPU, printed as one JSON object: one
training.Inferer.run over R replicas (ddd_eval_metrics: two launches and one host read
whatever R is) against the route to the same numbers before it existed: per replica one
forward-only ddd_train_loss_grad call with want_predictions, a copy of the predictions to
the host and training.calculate_metrics in NumPy.

Default Burgers net (5 taps x 32 filters, 3 layers) at N = 64, 2 048 rows, R in {1, 4, 16},
replica r from init seed r.  Per R, in a child process of its own: one warm-up of each
route, then `rounds` (at least 5) alternating rounds by wall clock, each ending on the host
with the metrics dicts; the medians and the spread (max - min) / median of each route's
rounds are reported, and `ratio` = the per-replica route's time over Inferer.run's.  The
child also checks that the two routes' loss agrees bit for bit and their MAE to 1e-4.
Inputs are random-phase sine waves; labels / baseline are synthetic perturbations.

  python profiles/tools/eval_metrics_throughput.py [--rounds 5]
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
NUM_POINTS, ROWS = 64, 2048


def measure(replicas, rounds, seed=0):
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
  rs = np.random.RandomState(seed)
  x = eq.grid.solution_x
  y = np.sum(rs.uniform(-0.5, 0.5, (ROWS, 4, 1)) * np.sin(
      2 * np.pi * rs.randint(1, 4, (ROWS, 4, 1)) * x / eq.grid.period
      + rs.uniform(0, 2 * np.pi, (ROWS, 4, 1))), axis=1).astype(np.float32)
  y = torch.as_tensor(y, device='cuda')
  heads = len(eq.DERIVATIVE_ORDERS) + 1
  labels = torch.as_tensor(rs.randn(ROWS, n, heads).astype(np.float32), device='cuda')
  baseline = labels + 0.1 * torch.as_tensor(rs.randn(ROWS, n, heads).astype(np.float32),
                                            device='cuda')
  hp.error_scale = [1.0] * (2 * heads)
  hp.error_floor = [1e-3] * heads
  data = model_lib.DeviceDataset(y, labels, baseline, 128, repeat=False, seed=seed)
  population = training.PopulationTrainer(models, hp)
  inferer = training.Inferer(data, population)
  equation_type = equations.equation_type_from_hparams(hp)
  host_labels, host_baseline = labels.cpu().numpy(), baseline.cpu().numpy()

  def one_call():
    torch.cuda.synchronize()
    started = time.perf_counter()
    metrics = inferer.run()
    return time.perf_counter() - started, metrics

  def per_replica():
    torch.cuda.synchronize()
    started = time.perf_counter()
    metrics = []
    for trainer in population.trainers:
      per_head, _, preds = trainer.loss_and_grad(data, want_grad=False, want_predictions=True)
      found = training.calculate_metrics(
          dict(labels=host_labels, baseline=host_baseline, predictions=preds.cpu().numpy(),
               **training.loss_metrics(per_head, hp, equation_type)), equation_type)
      metrics.append(found)
    return time.perf_counter() - started, metrics

  _, want = per_replica()
  _, got = one_call()
  same_loss = all(g['loss'] == w['loss'] for g, w in zip(got, want))
  mae_close = all(abs(g[k] - w[k]) <= 1e-4 * abs(w[k]) for g, w in zip(got, want)
                  for k in w if k.startswith('mae/'))
  old_times, new_times = [], []
  for _ in range(max(rounds, 5)):
    old_times.append(per_replica()[0])
    new_times.append(one_call()[0])
  old_median, new_median = float(np.median(old_times)), float(np.median(new_times))
  return {
      'replicas': replicas, 'num_points': n, 'rows': ROWS,
      'same_loss_bits': same_loss, 'mae_within_1e-4': mae_close,
      'per_replica_route_s': old_times, 'inferer_run_s': new_times,
      'per_replica_route_median_s': old_median, 'inferer_run_median_s': new_median,
      'per_replica_route_spread': (max(old_times) - min(old_times)) / old_median,
      'inferer_run_spread': (max(new_times) - min(new_times)) / new_median,
      'ratio': old_median / new_median,
  }


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--replicas', type=int, default=None,
                      help='one R in this process (the children)')
  args = parser.parse_args()
  if args.replicas is not None:
    print(json.dumps(measure(args.replicas, args.rounds)))
    return
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('eval_metrics_throughput.py needs a GPU')
  device = torch.cuda.get_device_name(0)
  started = time.time()
  rows = []
  for replicas in REPLICAS:
    done = subprocess.run(
        [sys.executable, os.path.abspath(__file__), '--rounds', str(args.rounds), '--replicas',
         str(replicas)], capture_output=True, text=True, timeout=300)
    if done.returncode != 0:   # nothing more is started on the device after a failure
      raise SystemExit('R = {} failed ({}):\n{}'.format(replicas, done.returncode,
                                                       done.stderr[-2000:]))
    rows.append(json.loads(done.stdout.strip().splitlines()[-1]))
  print(json.dumps({'tool': 'eval_metrics_throughput', 'device': device, 'rows': rows,
                    'wall_s': time.time() - started}))


if __name__ == '__main__':
  main()
