"""ddd_eval_metrics on the GPU: the loss rows against the forward-only loss kernels bit for
bit, replica independence and determinism, the exact indicator count, the five sums against
float64 NumPy, Inferer end to end against calculate_metrics on a float64 restatement, the
out-of-range index, and training_loop(metrics=True).

Every case runs once (_context, cached) and the tests read its results."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ddd1d_amd
from helpers import ROOT, make_model
from test_gpu_training import restated_result
from test_gpu_training import _setup as _setup_single
from test_gpu_train_unrolled import _restated, _setup as _setup_unrolled
from ddd1d_amd import _lib, equations, model as model_lib, training

pytestmark = pytest.mark.gpu

REPLICAS = 3
ROWS = 37   # rows of every case's dataset; 515 evaluated rows are drawn from them
CASES = {
    # name: (equation, conservative, N, overrides, T, rows evaluated, index).  The seeds of
    # labels / baseline are _setup's (0).  Share of points left out of the
    # frac_below_baseline comparison (two squared errors within 1e-4 relative, float64
    # restatement): the errors are continuous random variables of spread 0.3 and 0.1 of the
    # head's scale, so the expected share is of the order of 1e-4; each case asserts <= 1 %
    # and prints its share (test_end_to_end).  Measured on an MI355X: at most 0.028 % in
    # every case and replica (one or no point of a case).
    'burgers-cons-N32-T0': ('burgers', True, 32, dict(filter_size=32), 0, ROWS, None),
    'burgers-cons-N32-T2-515': ('burgers', True, 32, dict(filter_size=32), 2, 515, 'shared'),
    'burgers-cons-N128-T2': ('burgers', True, 128, dict(filter_size=32), 2, ROWS, 'shared'),
    'ks-N24-f16-T0-515': ('ks', False, 24, dict(filter_size=16), 0, 515, 'replica'),
    'ks-N24-f16-T2': ('ks', False, 24, dict(filter_size=16), 2, ROWS, 'replica'),
    'kdv-N40-T0': ('kdv', False, 40, dict(), 0, ROWS, 'shared'),
    'kdv-N40-space-T2': ('kdv', False, 40, dict(model_target='space_derivatives',
                                                kernel_size=3), 2, ROWS, None),
    'kdv-cons-N32-time-T0': ('kdv', True, 32, dict(model_target='time_derivative',
                                                   space_derivatives_weight=0.0), 0, ROWS,
                             'shared'),
}
NAMES = sorted(CASES)


def _flat(model):
  return torch.as_tensor(np.concatenate([np.concatenate([w.ravel(), b.ravel()])
                                         for w, b in zip(model.conv_kernels, model.conv_biases)]),
                         device='cuda')


def _eval(c, weights, index, **kwargs):
  s = c['s']
  out = _lib.eval_metrics(s['cfg'], weights, s['y'], s['labels'], s['baseline'], s['floor'],
                          s['coef_abs'], s['coef_rel'], num_time_steps=c['steps'],
                          time_step=s.get('dt', 0.0), nullspace=s['nullspace'], bias=s['bias'],
                          sample_index=index, want_predictions=True, **kwargs)
  return tuple(t.cpu().numpy() for t in out)


def _parent_means(c, weights, index):
  """head_means of the forward-only loss call on one replica's weights and index."""
  s = c['s']
  common = dict(nullspace=s['nullspace'], bias=s['bias'], sample_index=index,
                batch=c['evaluated'], want_grad=False)
  if c['steps']:
    means, _, _ = _lib.train_unrolled_loss_grad(
        s['cfg'], weights, s['y'], s['labels'], s['baseline'], s['floor'], s['coef_abs'],
        s['coef_rel'], c['steps'], s['dt'], **common)
  else:
    means, _, _ = _lib.train_loss_grad(
        s['cfg'], weights, s['y'], s['labels'], s['baseline'], s['floor'], s['coef_abs'],
        s['coef_rel'], **common)
  return means.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _context(name):
  equation, conservative, n, overrides, steps, evaluated, index_kind = CASES[name]
  models = [make_model(equation, conservative=conservative, num_points=n, init_seed=r,
                       **overrides) for r in range(REPLICAS)]
  s = _setup_unrolled(models[0], ROWS, steps) if steps else _setup_single(models[0], ROWS)
  weights = torch.stack([_flat(model) for model in models]).contiguous()
  rs = np.random.RandomState(len(name))
  index = None
  if index_kind == 'shared':
    index = rs.randint(0, ROWS, size=evaluated).astype(np.int32)
  elif index_kind == 'replica':
    index = rs.randint(0, ROWS, size=(REPLICAS, evaluated)).astype(np.int32)
  assert index is not None or evaluated == ROWS
  c = dict(name=name, models=models, s=s, steps=steps, evaluated=evaluated, weights=weights,
           index=index, index_dev=None if index is None else torch.as_tensor(index).cuda())
  c['all'] = _eval(c, weights, c['index_dev'])
  c['again'] = _eval(c, weights, c['index_dev'])
  c['solo'] = [_eval(c, weights[r:r + 1].contiguous(), _row(c, r, keep_dim=True))
               for r in range(REPLICAS)]
  c['parent'] = [_parent_means(c, weights[r].contiguous(), _row(c, r))
                 for r in range(REPLICAS)]
  return c


def _row(c, r, keep_dim=False):
  """Replica r's sample_index as a device tensor ([B], or [1, B] for a per-replica call)."""
  index = c['index_dev']
  if index is None or index.dim() == 1:
    return index
  return index[r:r + 1].contiguous() if keep_dim else index[r].contiguous()


def _rows_of(c, r):
  """Replica r's evaluated rows as a host array."""
  if c['index'] is None:
    return np.arange(c['evaluated'])
  return c['index'] if c['index'].ndim == 1 else c['index'][r]


@pytest.mark.parametrize('name', NAMES)
def test_loss_rows_are_the_forward_only_head_means(name):
  c = _context(name)
  sums = c['all'][0]
  assert sums.shape == (REPLICAS, 7, c['s']['labels'].shape[-1])
  for r in range(REPLICAS):
    np.testing.assert_array_equal(sums[r, :2], c['parent'][r])
    assert np.isfinite(sums[r]).all()


@pytest.mark.parametrize('name', NAMES)
def test_replicas_are_independent_and_calls_repeat(name):
  c = _context(name)
  for got, again in zip(c['all'], c['again']):
    np.testing.assert_array_equal(got, again)
  for r in range(REPLICAS):
    for got, solo in zip(c['all'], c['solo'][r]):
      np.testing.assert_array_equal(got[r], solo[0])


def _terms(labels, baseline, predictions, dtype):
  """The five sums' terms and the indicator, every operation in `dtype`."""
  l, b, p = (np.asarray(a, dtype) for a in (labels, baseline, predictions))
  d, e = l - p, l - b
  tiny = dtype(1e-8)
  terms = [np.abs(d), np.abs(e), d * d, e * e,
           np.log(np.maximum(np.abs(d), tiny)) - np.log(np.maximum(np.abs(e), tiny))]
  return terms, d * d < e * e


@pytest.mark.parametrize('name', NAMES)
def test_indicator_count_is_exact(name):
  c = _context(name)
  _, below, preds = c['all']
  labels, baseline = c['s']['labels'].cpu().numpy(), c['s']['baseline'].cpu().numpy()
  for r in range(REPLICAS):
    rows = _rows_of(c, r)
    _, under = _terms(labels[rows], baseline[rows], preds[r], np.float32)
    np.testing.assert_array_equal(below[r], under.sum(axis=(0, 1)))
    assert below.dtype == np.int32


@pytest.mark.parametrize('name', NAMES)
def test_five_sums_against_float64(name):
  """Error of each sum over the float64 sum of its terms' magnitudes (the sum itself for the
  four non-negative ones; the log differences cancel, so their sum is no scale of its
  rounding).  Bound: max(1e-5, 4 x floor), the floor being the same error of float32 NumPy
  sums under two orders (pairwise and sequential) of float32 terms; above 1e-3 it fails."""
  c = _context(name)
  sums, _, preds = c['all']
  labels, baseline = c['s']['labels'].cpu().numpy(), c['s']['baseline'].cpu().numpy()
  worst = 0.0
  for r in range(REPLICAS):
    rows = _rows_of(c, r)
    terms64, _ = _terms(labels[rows], baseline[rows], preds[r], np.float64)
    terms32, _ = _terms(labels[rows], baseline[rows], preds[r], np.float32)
    for k, (t64, t32) in enumerate(zip(terms64, terms32)):
      heads = t64.shape[-1]
      want = t64.reshape(-1, heads).sum(axis=0)
      scale = np.abs(t64).reshape(-1, heads).sum(axis=0)
      flat32 = t32.reshape(-1, heads)
      pairwise = np.ascontiguousarray(flat32.T).sum(axis=1, dtype=np.float32)
      sequential = np.cumsum(flat32, axis=0, dtype=np.float32)[-1]
      floor = max(np.max(np.abs(pairwise - want) / scale),
                  np.max(np.abs(sequential - want) / scale))
      err = np.max(np.abs(sums[r, 2 + k].astype(np.float64) - want) / scale)
      print('{} replica {} sum {}: err {:.2e} floor {:.2e}'.format(name, r, 2 + k, err, floor))
      worst = max(worst, floor)
      assert floor < 1e-3, (name, r, k, floor)
      assert err < max(1e-5, 4 * floor), (name, r, k, err, floor)
  print('{}: largest float32 floor {:.2e}'.format(name, worst))


def _population(c):
  """A PopulationTrainer over the case's models and its dataset, loss constants from the
  case (error_scale 1: the coefficients are folded into nothing the metrics read)."""
  import copy
  s = c['s']
  hp = copy.copy(c['models'][0].hparams)
  hp.num_time_steps = c['steps']
  heads = int(s['labels'].shape[-1])
  hp.error_floor = [float(v) for v in s['floor']]
  hp.error_scale = [1.0] * (2 * heads)
  population = training.PopulationTrainer(c['models'], hp)
  dataset = model_lib.DeviceDataset(s['y'], s['labels'], s['baseline'], 8, False, 0)
  return population, dataset, hp


def _rel(got, want):
  return abs(got - want) / abs(want)


@pytest.mark.parametrize('name', NAMES)
def test_end_to_end_against_float64_restatement(name):
  """Inferer.run against calculate_metrics on float64 predictions of the restated forward
  pass.  Ratios and geometric means: max(1e-5, 4 x floor), the floor being the same
  metric of the float32 restatement against the float64 one (ceiling 1e-3).
  frac_below_baseline: the points whose two squared errors differ by less than 1e-4
  relative (float64) are left out, at most 1 % of a case's points; on the others the
  indicator of the kernel's predictions is the float64 one."""
  c = _context(name)
  population, dataset, hp = _population(c)
  assert np.array_equal(population.weights.cpu().numpy(), c['weights'].cpu().numpy())
  inferer = training.Inferer(dataset, population)
  got = inferer.run()
  _, _, preds = inferer.run_async(want_predictions=True)
  preds = preds.cpu().numpy()
  equation_type = equations.equation_type_from_hparams(hp)
  s = c['s']
  labels, baseline = s['labels'].double().cpu().numpy(), s['baseline'].double().cpu().numpy()
  assert len(got) == REPLICAS
  for r in range(REPLICAS):
    with torch.no_grad():
      if c['steps']:
        p64 = _restated(c['models'][r], s['y'], c['weights'][r], c['steps'], torch.float64)
        p32 = _restated(c['models'][r], s['y'], c['weights'][r], c['steps'], torch.float32)
      else:
        p64 = restated_result(c['models'][r], s['y'], c['weights'][r], torch.float64)
        p32 = restated_result(c['models'][r], s['y'], c['weights'][r], torch.float32)
    p64, p32 = p64.cpu().numpy(), p32.double().cpu().numpy()
    data = dict(labels=labels, baseline=baseline)
    want = training.calculate_metrics(dict(data, predictions=p64), equation_type)
    want32 = training.calculate_metrics(dict(data, predictions=p32), equation_type)
    assert got[r]['count'] == ROWS
    assert set(want) | {'loss', 'loss/space_derivatives', 'loss/time_derivative'} <= set(got[r])
    for key in want:
      if key == 'count' or key.startswith('frac_below_baseline'):
        continue
      if hp.model_target == 'time_derivative' and not key.endswith(('u_t', 'u(t)')):
        # (zero predictions: the space-derivative metrics do not depend on the net)
        assert _rel(got[r][key], want[key]) < 1e-5, (key, got[r][key], want[key])
        continue
      floor = _rel(want32[key], want[key])
      err = _rel(got[r][key], want[key])
      print('{} replica {} {}: err {:.2e} floor {:.2e}'.format(name, r, key, err, floor))
      assert floor < 1e-3, (key, floor)
      assert err < max(1e-5, 4 * floor), (key, err, floor)
    d2, b2 = (labels - p64) ** 2, (labels - baseline) ** 2
    keep = np.abs(d2 - b2) >= 1e-4 * np.maximum(d2, b2)
    share = 1.0 - keep.mean()
    print('{} replica {}: {:.3%} of the points left out'.format(name, r, share))
    assert share <= 0.01
    lab32, base32 = s['labels'].cpu().numpy(), s['baseline'].cpu().numpy()
    under = (lab32 - preds[r]) * (lab32 - preds[r]) < (lab32 - base32) * (lab32 - base32)
    np.testing.assert_array_equal(under[keep], (d2 < b2)[keep])
    for key in want:
      if key.startswith('frac_below_baseline'):
        assert abs(got[r][key] - want[key]) <= share + 1e-12, (key, got[r][key], want[key])
    # the loss entries: the forward-only loss of the whole dataset
    per_head = population.trainers[r].loss_and_grad(dataset, want_grad=False)[0]
    assert got[r]['loss'] == float(model_lib.weighted_loss(per_head, hp))


@pytest.mark.parametrize('name', ['burgers-cons-N32-T2-515', 'ks-N24-f16-T0-515', 'kdv-N40-T0'])
def test_population_loss_is_the_per_replica_loop(name):
  c = _context(name)
  population, dataset, _ = _population(c)
  want = np.stack([trainer.loss_and_grad(dataset, want_grad=False)[0]
                   for trainer in population.trainers])
  np.testing.assert_array_equal(population.loss(dataset), want)


@pytest.mark.parametrize('name', ['burgers-cons-N32-T2-515', 'ks-N24-f16-T0-515'])
def test_out_of_range_index_poisons_its_replica_only(name):
  c = _context(name)
  index = c['index'] if c['index'].ndim == 2 else np.stack([c['index']] * REPLICAS)
  index = index.copy()
  index[1, c['evaluated'] // 2] = ROWS   # one past the last row, in replica 1 only
  sums, below, preds = _eval(c, c['weights'], torch.as_tensor(index).cuda())
  assert np.isnan(sums[1]).all() and (below[1] == -1).all()
  assert np.isnan(preds[1, c['evaluated'] // 2]).all()
  for r in (0, 2):
    for got, base in zip((sums, below, preds), c['all']):
      np.testing.assert_array_equal(got[r], base[r])


def test_training_loop_with_metrics(tmp_path):
  """The reference's sanity case (training_test.py): 100 random snapshots of 256 points,
  20 steps, an evaluation every 10."""
  snapshots = np.random.RandomState(0).randn(100, 256)
  hp = ddd1d_amd.create_hparams('burgers', learning_rates=[1e-3], learning_stops=[20],
                                eval_interval=10,
                                equation_kwargs=json.dumps({'num_points': 256}))
  plain = training.training_loop(snapshots, str(tmp_path / 'plain'), hp, num_steps=20)
  rows = training.training_loop(snapshots, str(tmp_path / 'metrics'), hp, num_steps=20,
                                metrics=True)
  assert [row['step'] for row in rows] == [0, 10, 20] and len(plain) == 3
  with np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_metrics.npz')) as z:
    keys = [str(k) for k in z['case0_keys']]   # conservative Burgers (the default), no integrated heads
  for row, base in zip(rows, plain):
    assert sorted(base) == ['loss', 'loss_per_head', 'step']
    assert {k: row[k] for k in base} == base   # the metrics change nothing else
    for key in keys:
      for split in ('test_', 'train_'):
        assert np.isfinite(row[split + key]), (split + key, row[split + key])
    assert row['test_count'] == 20 and row['train_count'] == 80
    assert row['test_loss'] == row['loss']
  with np.load(str(tmp_path / 'plain' / 'model.npz')) as a, \
       np.load(str(tmp_path / 'metrics' / 'model.npz')) as b:
    for key in a.files:
      np.testing.assert_array_equal(a[key], b[key])
  frame = training.metrics_to_dataframe(
      [(row['step'], {k[5:]: v for k, v in row.items() if k.startswith('test_')},
        {k[6:]: v for k, v in row.items() if k.startswith('train_')}) for row in rows])
  assert len(frame) == 3 and 'test_mae/u_x' in frame.columns
