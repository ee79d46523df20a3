"""Replica populations on the GPU (ddd_train_population_run, PopulationTrainer,
training_population).  The criterion needs no tolerance: replica r of a population call
is bit for bit (torch.equal) the solo ddd_train_run call given replica r's weights, Adam
state, learning rates and index -- the weights, adam_m, adam_v, every log row and
last_grad.  Unless a case says otherwise the replicas start from distinct weights
(distinct init seeds) and non-zero Adam states, with distinct learning-rate rows and
distinct index rows."""
import copy

import numpy as np
import pytest
import torch

from helpers import make_hparams
from test_gpu_training import _model, _setup, _run
from test_gpu_train_unrolled import _setup as _setup_unrolled
from ddd1d_amd import _lib, model as model_lib, training

pytestmark = pytest.mark.gpu

BETAS = (0.9, 0.99)
EPS = 1e-8


def _flat(model):
  return torch.as_tensor(np.concatenate([np.concatenate([w.ravel(), b.ravel()])
                                         for w, b in zip(model.conv_kernels,
                                                         model.conv_biases)]), device='cuda')


def _replica_weights(equation, conservative, n, overrides, replicas):
  """[R, n_weights]: row r is the model of init seed r."""
  return torch.stack([_flat(_model(equation, conservative, n, dict(overrides, init_seed=r)))
                      for r in range(replicas)]).contiguous()


def _state(weights, seed):
  """Non-zero Adam moments of the size a few steps leave behind."""
  rs = np.random.RandomState(seed)
  m = torch.as_tensor((1e-2 * rs.randn(*weights.shape)).astype(np.float32), device='cuda')
  v = torch.as_tensor((1e-4 * rs.uniform(0.1, 2.0, weights.shape)).astype(np.float32),
                      device='cuda')
  return m, v


def _index(steps, replicas, batch, rows, seed=0):
  """[steps, R, batch] (replicas = None: [steps, batch])."""
  shape = (steps, batch) if replicas is None else (steps, replicas, batch)
  rs = np.random.RandomState(seed)
  return torch.as_tensor(rs.randint(0, rows, size=shape).astype(np.int32), device='cuda')


def _rates(replicas, steps):
  return [[1e-3 * (r + 1) / (k + 1) for k in range(steps)] for r in range(replicas)]


def _common(s, **kwargs):
  return dict(dict(betas=BETAS, epsilon=EPS, nullspace=s['nullspace'], bias=s['bias'],
                   want_last_grad=True), **kwargs)


def _population(s, weights, m, v, index, rates, **kwargs):
  """_lib.train_population_run on copies: (weights, m, v, log, last_grad)."""
  w, m, v = weights.clone(), m.clone(), v.clone()
  log, last = _lib.train_population_run(
      s['cfg'], w, m, v, s['y'], s['labels'], s['baseline'], index, rates, s['floor'],
      s['coef_abs'], s['coef_rel'], **_common(s, **kwargs))
  return w, m, v, log, last


def _solo(s, weights, m, v, index, rates, **kwargs):
  """_lib.train_run on copies of one replica's rows: (weights, m, v, log, last_grad)."""
  w, m, v = weights.clone(), m.clone(), v.clone()
  log, last = _lib.train_run(
      s['cfg'], w, m, v, s['y'], s['labels'], s['baseline'], index.contiguous(), rates,
      s['floor'], s['coef_abs'], s['coef_rel'], **_common(s, **kwargs))
  return w, m, v, log, last


def _assert_replicas_are_solo_runs(s, weights, m, v, index, rates, replicas=None, **kwargs):
  """Every replica (or those listed) of the population call against its solo run; returns
  the population call's outputs and the solo runs'."""
  got = _population(s, weights, m, v, index, rates, **kwargs)
  solos = {}
  for r in (range(len(rates)) if replicas is None else replicas):
    rows = index[:, r] if index.dim() == 3 else index
    want = _solo(s, weights[r], m[r], v[r], rows, rates[r], **kwargs)
    solos[r] = want
    names = ('weights', 'adam_m', 'adam_v', 'log', 'last_grad')
    for name, a, b in zip(names, got, want):
      a = a[:, r] if name == 'log' else a[r]
      assert torch.equal(a, b), (name, r)
    assert torch.isfinite(want[0]).all() and not torch.equal(want[0], weights[r])
  return got, solos


# ---- 1. - 4. one evaluation per step ----

@pytest.mark.parametrize('equation,n,overrides,rows,batch,replicas,steps,per_replica', [
    # 1. the baseline
    ('burgers', 32, dict(), 12, 6, 3, 4, True),
    # 2. R = 1 with a shared index: ddd_train_run itself
    ('burgers', 32, dict(), 12, 6, 1, 4, False),
    # 3. more samples than slabs: 2 x 512 workgroups
    ('burgers', 32, dict(), 700, 600, 2, 1, True),
    # 4. the VALU-only route at the LDS limit
    ('ks', 256, dict(kernel_size=7, filter_size=64, num_layers=1), 12, 6, 2, 1, True),
    # 5. the MFMA route on all four wavefronts: the replicas' staged kernels and biases
    ('burgers', 128, dict(), 12, 6, 2, 2, True),
])
def test_replicas_are_solo_runs(equation, n, overrides, rows, batch, replicas, steps,
                                per_replica):
  s = _setup(_model(equation, False, n, overrides), rows, seed=4)
  weights = _replica_weights(equation, False, n, overrides, replicas)
  assert replicas == 1 or not torch.equal(weights[0], weights[1])
  m, v = _state(weights, seed=1)
  index = _index(steps, replicas if per_replica else None, batch, rows, seed=2)
  got, _ = _assert_replicas_are_solo_runs(s, weights, m, v, index, _rates(replicas, steps),
                                          first_step=3)
  assert tuple(got[3].shape) == (steps, replicas, 2, s['labels'].shape[-1])


def test_a_shared_index_serves_every_replica():
  s = _setup(_model('burgers', False, 32, dict()), 12, seed=4)
  weights = _replica_weights('burgers', False, 32, dict(), 2)
  m, v = _state(weights, seed=1)
  _assert_replicas_are_solo_runs(s, weights, m, v, _index(2, None, 6, 12, seed=3),
                                 _rates(2, 2))


# ---- 5. through time ----

def test_replicas_through_time_are_solo_runs():
  s = _setup_unrolled(_model('burgers', True, 32, dict()), 12, 2, seed=1)
  weights = _replica_weights('burgers', True, 32, dict(), 2)
  m, v = _state(weights, seed=5)
  index = _index(2, 2, 6, 12, seed=6)
  got, _ = _assert_replicas_are_solo_runs(s, weights, m, v, index, _rates(2, 2),
                                          num_time_steps=2, time_step=s['dt'])
  assert tuple(got[3].shape) == (2, 2, 2, 3 + 2)


# ---- 6. error_max: the replicas clip independently ----

def test_replicas_clip_independently():
  """Replica 1's weights are replica 0's scaled up, so its errors are larger.  error_max
  lies between the two replicas' largest scaled means: replica 1 then clips a term that
  replica 0 keeps, which is asserted from the solo runs' logs before anything else."""
  s = _setup(_model('burgers', False, 32, dict()), 12, seed=4)
  scale = np.stack([s['coef_abs'], s['coef_rel']])   # error_scale: a weighted loss of sums
  base = _flat(_model('burgers', False, 32, dict()))
  weights = torch.stack([base, 3.0 * base]).contiguous()
  m, v = torch.zeros_like(weights), torch.zeros_like(weights)
  index = _index(1, None, 6, 12, seed=7)
  scaled = []
  for r in range(2):
    means, _, _ = _run(dict(s, flat=weights[r].contiguous()), sample_index=index[0].contiguous(),
                       want_grad=False)
    scaled.append(means.double().cpu().numpy() * scale)
  # the inputs of the case: some term of replica 1 lies above the same term of replica 0;
  # error_max goes between the two
  gap = scaled[1] - scaled[0]
  term = np.unravel_index(np.argmax(gap), gap.shape)
  assert gap[term] > 0, 'test inputs: replica 1 has no term above replica 0'
  error_max = float(0.5 * (scaled[0][term] + scaled[1][term]))
  kwargs = dict(error_max=error_max, error_scale=scale)
  got, solos = _assert_replicas_are_solo_runs(s, weights, m, v, index, _rates(2, 1), **kwargs)
  clipped = [solos[r][3][0].double().cpu().numpy() * scale >= error_max for r in range(2)]
  assert clipped[1][term] and not clipped[0][term]
  assert (clipped[1] & ~clipped[0]).any()
  # and the clipping acted: replica 1's gradient is not the unclipped one
  plain = _solo(s, weights[1], m[1], v[1], index, _rates(2, 1)[1])
  assert not torch.equal(plain[4], got[4][1])
  assert torch.equal(plain[3], got[3][:, 1])   # (the logged means are the unclipped ones)


# ---- 7. isolation ----

def _isolation_case():
  s = _setup(_model('burgers', False, 32, dict()), 12, seed=4)
  replicas, rows, sentinel = 2, 12, -123.25
  weights = _replica_weights('burgers', False, 32, dict(), replicas)
  m, v = _state(weights, seed=1)
  index = _index(2, replicas, 6, rows, seed=8)
  index[0, 1, 2] = rows   # out of range: replica 1 reads nothing for that sample
  rates = _rates(replicas, 2)

  def padded(t):
    return torch.cat([t, torch.full_like(t[:1], sentinel)]).contiguous()
  w, pm, pv = padded(weights), padded(m), padded(v)
  log, last = _lib.train_population_run(
      s['cfg'], w, pm, pv, s['y'], s['labels'], s['baseline'], index, rates, s['floor'],
      s['coef_abs'], s['coef_rel'], **_common(s))
  solos = [_solo(s, weights[0], m[0], v[0], index[:, 0], rates[0])]
  return sentinel, (w, pm, pv, log, last), solos


def test_replicas_are_isolated():
  """An index outside [0, S) in replica 1's rows: the kernel reads nothing for that sample,
  replica 1's means of that step and, through the update, its weights and Adam state
  become NaN (the contract include/ddd1d.h states), and nothing else is touched."""
  sentinel, (w, pm, pv, log, last), solos = _isolation_case()
  for t in (w, pm, pv):   # a row behind the last replica is not touched
    assert (t[2] == sentinel).all()
  assert tuple(last.shape) == (2, w.shape[1])
  print('replica 1: NaN in the log row {} of {}, in the weights {} of {}'.format(
      int(torch.isnan(log[0, 1]).sum()), log[0, 1].numel(), int(torch.isnan(w[1]).sum()),
      w.shape[1]))
  assert torch.isnan(log[0, 1]).all()
  for t in (w, pm, pv, last):
    assert torch.isnan(t[1]).all()
  # replica 0 next to it is its solo run
  for a, b in zip((w[0], pm[0], pv[0], log[:, 0], last[0]), solos[0]):
    assert torch.equal(a, b)
  assert torch.isfinite(w[0]).all() and torch.isfinite(log[:, 0]).all()


# ---- 8. determinism and continuity ----

def test_determinism_and_continuity():
  s = _setup(_model('burgers', False, 32, dict()), 12, seed=4)
  weights = _replica_weights('burgers', False, 32, dict(), 3)
  m, v = _state(weights, seed=1)
  index = _index(6, 3, 6, 12, seed=9)
  rates = _rates(3, 6)
  whole = _population(s, weights, m, v, index, rates, first_step=2)
  again = _population(s, weights, m, v, index, rates, first_step=2)
  for a, b in zip(whole, again):
    assert torch.equal(a, b)
  first = _population(s, weights, m, v, index[:3].contiguous(), [row[:3] for row in rates],
                      first_step=2)
  second = _population(s, first[0], first[1], first[2], index[3:].contiguous(),
                       [row[3:] for row in rates], first_step=5)
  for a, b in zip(whole[:3], second[:3]):
    assert torch.equal(a, b)
  assert torch.equal(whole[3], torch.cat([first[3], second[3]]))
  assert torch.equal(whole[4], second[4])


# ---- 9. Python ----

def _trainer_setup():
  hp = None
  models = []
  for r in range(3):
    model = _model('burgers', False, 32, dict(init_seed=r))
    models.append(model)
  s = _setup(models[0], 12, seed=6)
  hp = models[0].hparams
  hp.absolute_error_weight, hp.relative_error_weight = 1.0, 1.0
  hp.space_derivatives_weight, hp.time_derivative_weight = 1.0, 1.0
  hp.error_floor = list(s['floor'])
  hp.error_scale = list(np.concatenate([s['coef_abs'], s['coef_rel']]))
  hp.learning_rates = [1e-3, 1e-4]
  hp.learning_stops = [3, 6]
  data = model_lib.DeviceDataset(s['y'], s['labels'], s['baseline'], 6, True, 0)
  return models, hp, data


def test_population_trainer_against_trainers():
  models, hp, data = _trainer_setup()
  rows = [[1e-3, 1e-4], [5e-3, 5e-5], [2e-3, 2e-3]]
  index = _index(6, 3, 6, 12, seed=10)
  population = training.PopulationTrainer(models, hp, learning_rates=rows)
  losses = population.run(data, 4, index[:4])
  losses = np.concatenate([losses, population.run(data, 2, index[4:])])   # over the stop
  assert losses.shape == (6, 3, 2, 3) and population.step_count == 6
  exported = population.export()
  validation = population.loss(data)
  assert len(exported) == 3 and validation.shape == (3, 2, 3)
  for r, model in enumerate(models):
    replica_hp = copy.copy(hp)
    replica_hp.learning_rates = rows[r]
    solo = training.Trainer(model, replica_hp)
    want = solo.run(data, 6, index[:, r].contiguous())
    np.testing.assert_array_equal(losses[:, r], want)
    for a, b in zip(exported[r].conv_kernels + exported[r].conv_biases,
                    solo.export().conv_kernels + solo.export().conv_biases):
      np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(validation[r], solo.loss_and_grad(data, want_grad=False)[0])
  assert not np.array_equal(exported[0].conv_kernels[0], exported[1].conv_kernels[0])


def test_training_population_against_the_fused_loop(tmp_path):
  snapshots = np.random.RandomState(0).randn(60, 128).astype(np.float32)
  hp = make_hparams('burgers', conservative=True, num_points=32, resample_factor=4,
                    learning_stops=[5], eval_interval=2)
  seed = 3
  dirs = [str(tmp_path / 'replica0'), str(tmp_path / 'replica1')]
  rows = training.training_population(snapshots, dirs, hp, init_seeds=[seed, seed + 1],
                                      seed=seed)
  solo = training.training_loop(snapshots, str(tmp_path / 'solo'), hp, seed=seed, fused=True)
  assert len(rows) == 2 and [r['step'] for r in rows[0]] == [0, 2, 4]
  assert rows[0] == solo
  assert rows[1] != solo and all(np.isfinite(r['loss']) for r in rows[1])
  with np.load(str(tmp_path / 'solo' / 'model.npz')) as want:
    with np.load(str(tmp_path / 'replica0' / 'model.npz')) as same:
      assert sorted(same.files) == sorted(want.files)
      for name in want.files:
        np.testing.assert_array_equal(same[name], want[name])
    with np.load(str(tmp_path / 'replica1' / 'model.npz')) as other:
      assert any(not np.array_equal(other[name], want[name]) for name in want.files)
  with open(str(tmp_path / 'solo' / 'hparams.json')) as a:
    with open(str(tmp_path / 'replica0' / 'hparams.json')) as b:
      assert a.read() == b.read()
