"""Rollout fine-tuning on the device (ddd_train_rollout_run, RolloutTrainer.run,
RolloutPopulationTrainer, fine_tune_on_rollouts(fused=True),
fine_tune_population_on_rollouts) on the GPU: the gradient, the step means and the norm of a
step against ddd_train_rollout_loss_grad, the clipped Adam update against a float64
evaluation of its formulas, every replica of a population against the call on that replica
alone, continuity, determinism, skipped steps, the host loop of RolloutTrainer.step, the
forward-only form, the weights shared with a PopulationTrainer and the curricula end to end.

Windows: 6 rows, minibatches of 4, T = 4 model steps saved every 2, unless said otherwise."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from helpers import make_hparams
from test_gpu_training import _model
from test_gpu_train_rollout import _case, _run, _exact_data
from test_gpu_population_weights import _burgers_reference, _assert_results_equal, _models
from ddd1d_amd import _lib, equations, evaluation, model as model_lib, training

pytestmark = pytest.mark.gpu

BETAS = (0.9, 0.99)
EPS = 1e-8
# (equation, conservative, N, overrides, forced): VALU layers, unforced; the MFMA-staged
# layers, the flux difference and the forcing with per-row start times; the minimum N
A = ('burgers', False, 32, dict(), False)
B = ('burgers', True, 64, dict(), True)
C = ('kdv', False, 8, dict(model_target='space_derivatives', kernel_size=3, filter_size=16),
     False)
ROWS, BATCH, T, EVERY = 6, 4, 4, 2


def _make(config, rows=ROWS, steps=T, every=EVERY, seed=10):
  equation, conservative, n, overrides, forced = config
  return _case(_model(equation, conservative, n, overrides), rows, steps, every, forced,
               seed=seed)


def _index(steps, batch, rows, seed=0, replicas=None):
  shape = (steps, batch) if replicas is None else (steps, replicas, batch)
  rs = np.random.RandomState(seed)
  return torch.as_tensor(rs.randint(0, rows, size=shape).astype(np.int32), device='cuda')


def _replica_state(c, replicas, seed=0):
  """Distinct weights, Adam moments and step counts for `replicas` replicas of c's model."""
  rs = np.random.RandomState(seed)
  n = c['flat'].numel()
  spread = float(c['flat'].abs().mean())
  w = torch.stack([c['flat'] + torch.as_tensor(
      (0.05 * r * spread * rs.randn(n)).astype(np.float32), device='cuda')
                   for r in range(replicas)]).contiguous()
  m = torch.as_tensor((1e-3 * rs.randn(replicas, n)).astype(np.float32), device='cuda')
  v = torch.as_tensor(rs.uniform(1e-6, 1e-5, (replicas, n)).astype(np.float32), device='cuda')
  t = torch.as_tensor((3 * np.arange(replicas)).astype(np.int32), device='cuda')
  return w, m, v, t


def _rollout_run(c, index, rates, state=None, clip=0.0, **kwargs):
  """_lib.train_rollout_run on copies of the state (weights, m, v, adam_step; default:
  c's weights as the population of one, zero moments, step 0): a dict of the state after
  the call, the two logs and last_grad."""
  if state is None:
    w = c['flat'][None]
    state = (w, torch.zeros_like(w), torch.zeros_like(w),
             torch.zeros(1, dtype=torch.int32, device='cuda'))
  w, m, v, t = (x.clone() for x in state)
  log, norms, last = _lib.train_rollout_run(
      c['cfg'], w, m, v, t, c['y0'], c['targets'], c['step_weights'], c['steps'], c['every'],
      c['dt'], index, rates, betas=BETAS, epsilon=EPS, clip_norm=clip, t0=c['t0'],
      forcing=c['forcing'], nullspace=c['nullspace'], bias=c['bias'], want_last_grad=True,
      **kwargs)
  return dict(w=w, m=m, v=v, t=t, log=log, norms=norms, last=last)


def _bits(x):
  return x.view(torch.int32) if x.dtype == torch.float32 else x


def _assert_same(got, want, where=''):
  """State, logs and last_grad bit for bit."""
  for key in ('w', 'm', 'v', 't', 'log', 'norms', 'last'):
    assert torch.equal(_bits(got[key]), _bits(want[key])), (where, key)


def _replica_of(result, r):
  """Replica r of a population result in the shape of a solo result."""
  out = {key: result[key][r:r + 1] for key in ('w', 'm', 'v', 't', 'last')}
  out['log'] = result['log'][:, r:r + 1]
  out['norms'] = result['norms'][:, r:r + 1]
  return out


def _solo(c, state, r, index, rates, **kwargs):
  """The call on replica r alone: its state, its learning-rate row, its minibatches."""
  solo_index = index[:, r].contiguous() if index.dim() == 3 else index
  return _rollout_run(c, solo_index, [rates[r]], tuple(x[r:r + 1] for x in state), **kwargs)


def _windows(c):
  return training.RolloutWindows(c['y0'], c['targets'], c['t0'], c['forcing'], c['dt'],
                                 c['steps'], c['every'], None, None)


def _rel(got, want):
  return ((got.double() - want.double()).norm() / want.double().norm()).item()


# ---- 1. one step, R = 1 -------------------------------------------------------------------
def _check_one_step(c, index):
  means, grad, _ = _run(c, sample_index=index[0].contiguous())
  out = _rollout_run(c, index, [[1e-3]])
  assert torch.equal(out['last'][0], grad)
  assert torch.equal(out['log'][0, 0], means)
  want = float(np.sqrt((grad.double() ** 2).sum().item()))
  ulp = float(np.spacing(np.float32(want)))
  got = float(out['norms'][0, 0])
  print('norm {:.9g}, float64 {:.9g}, {:.2f} float32 ulps apart'.format(
      got, want, abs(got - want) / ulp))
  # one rounding of the cast and one of the root
  assert abs(got - want) <= 2 * ulp
  assert out['t'].tolist() == [1]
  assert torch.isfinite(out['w']).all() and not torch.equal(out['w'][0], c['flat'])
  assert tuple(out['log'].shape) == (1, 1, c['steps'] // c['every'])


@pytest.mark.parametrize('config', [A, B, C], ids=['A', 'B', 'C'])
def test_one_step_gradient_means_and_norm(config):
  c = _make(config)
  _check_one_step(c, _index(1, BATCH, ROWS, seed=1))


def test_one_step_with_more_windows_than_slabs():
  c = _make(A, rows=700, steps=2, every=1, seed=11)
  _check_one_step(c, _index(1, 600, 700, seed=2))


# ---- 2. the update ------------------------------------------------------------------------
def test_one_step_update_matches_float64_formulas():
  """The bounds of test_gpu_train_run.test_one_step_update_matches_float64_formulas: per
  vector max(1e-6, 4 x floor) relative in norm, floor = float32 torch.optim.Adam's distance
  (single-tensor path, same gradient and state) from the float64 evaluation of the formulas
  on the float32 inputs, a floor above 1e-5 fails; the update itself within 1e-5 + 4 x the
  rounding of the weights, relative to its norm.  Unclipped, then with clip_norm = half the
  measured norm, the float64 yardstick scaling g by min(1, clip / (norm + 1e-12)) too."""
  c = _make(A, seed=12)
  index = _index(1, BATCH, ROWS, seed=3)
  _, g, _ = _run(c, sample_index=index[0].contiguous())
  rs = np.random.RandomState(3)
  scale = g.abs().mean().item()
  m0 = torch.as_tensor((scale * rs.randn(g.numel())).astype(np.float32), device='cuda')
  v0 = torch.as_tensor((scale ** 2 * rs.uniform(0.1, 2.0, g.numel())).astype(np.float32),
                       device='cuda')
  lr, first = 1e-2, 4
  state = (c['flat'][None], m0[None], v0[None],
           torch.full((1,), first, dtype=torch.int32, device='cuda'))
  plain = _rollout_run(c, index, [[lr]], state)
  norm = float(plain['norms'][0, 0])
  assert torch.equal(plain['last'][0], g) and plain['t'].tolist() == [first + 1]

  for clip in (0.0, 0.5 * norm):
    out = plain if clip == 0.0 else _rollout_run(c, index, [[lr]], state, clip=clip)
    assert torch.equal(out['last'][0], g) and float(out['norms'][0, 0]) == norm
    t = first + 1
    factor = 1.0
    if clip:
      factor = min(1.0, clip / (np.sqrt((g.double() ** 2).sum().item()) + 1e-12))
      assert factor < 0.51
    g64, w0 = g.double() * factor, c['flat'].double()
    m64 = m0.double() + (g64 - m0.double()) * (1 - BETAS[0])
    v64 = BETAS[1] * v0.double() + (1 - BETAS[1]) * g64 * g64
    denom = v64.sqrt() / np.sqrt(1 - BETAS[1] ** t) + EPS
    w64 = w0 - (lr / (1 - BETAS[0] ** t)) * m64 / denom

    param = torch.nn.Parameter(c['flat'].clone())
    adam = torch.optim.Adam([param], lr=lr, betas=BETAS, eps=EPS, foreach=False)
    adam.state[param] = dict(step=torch.tensor(float(first)), exp_avg=m0.clone(),
                             exp_avg_sq=v0.clone())
    param.grad = g64.float()
    adam.step()
    torch_state = adam.state[param]
    for name, got, want, torch_got in (('weights', out['w'][0], w64, param.detach()),
                                       ('m', out['m'][0], m64, torch_state['exp_avg']),
                                       ('v', out['v'][0], v64, torch_state['exp_avg_sq'])):
      floor = _rel(torch_got, want)
      err = _rel(got, want)
      print('clip {:.3g}: {}: err {:.2e}, torch.optim.Adam float32 floor {:.2e}'.format(
          clip, name, err, floor))
      assert floor < 1e-5, (name, floor)
      assert err < max(1e-6, 4 * floor), (name, err, floor)
    update = w64 - w0
    rounding = 2.0 ** -24 * w0.norm().item() / update.norm().item()
    err = _rel(out['w'][0].double() - w0, update)
    print('clip {:.3g}: update: err {:.2e}, rounding of the weights {:.2e}'.format(
        clip, err, rounding))
    assert err < 1e-5 + 4 * rounding, (err, rounding)

  # a clip above the norm: the bits of no clip
  _assert_same(_rollout_run(c, index, [[lr]], state, clip=2.0 * norm), plain, 'clip above')
  clipped = _rollout_run(c, index, [[lr]], state, clip=0.5 * norm)
  assert not torch.equal(clipped['w'], plain['w'])


# ---- 3. replica identity ------------------------------------------------------------------
@pytest.mark.parametrize('per_replica', [False, True], ids=['shared-index', 'index-per-replica'])
@pytest.mark.parametrize('config', [A, B], ids=['A', 'B'])
def test_every_replica_is_its_solo_run(config, per_replica):
  replicas, opt_steps = 3, 3
  c = _make(config, seed=13)
  state = _replica_state(c, replicas, seed=4)
  assert not torch.equal(state[0][0], state[0][1]) and not torch.equal(state[1][0], state[1][2])
  rates = [[1e-3, 1e-3, 1e-4], [5e-3, 5e-4, 5e-5], [2e-3, 2e-3, 1e-3]]
  index = _index(opt_steps, BATCH, ROWS, seed=5, replicas=replicas if per_replica else None)
  clip = 0.0
  for attempt in range(2):   # unclipped, then with a clip that some steps reach
    got = _rollout_run(c, index, rates, state, clip=clip)
    assert torch.isfinite(got['norms']).all()
    assert got['t'].tolist() == [opt_steps + 3 * r for r in range(replicas)]
    for r in range(replicas):
      assert not torch.equal(got['w'][r], state[0][r])
      _assert_same(_replica_of(got, r), _solo(c, state, r, index, rates, clip=clip),
                   (clip, r))
    assert not torch.equal(got['w'][0], got['w'][1])
    clip = float(got['norms'].median())


# ---- 4. continuity and determinism --------------------------------------------------------
def test_continuity_and_determinism():
  c = _make(A, seed=14)
  index = _index(6, BATCH, ROWS, seed=6)
  rates = [[1e-3] * 3 + [1e-4] * 3]
  whole = _rollout_run(c, index, rates)
  _assert_same(_rollout_run(c, index, rates), whole, 'repeat')
  first = _rollout_run(c, index[:3].contiguous(), [rates[0][:3]])
  second = _rollout_run(c, index[3:].contiguous(), [rates[0][3:]],
                        (first['w'], first['m'], first['v'], first['t']))
  assert first['t'].tolist() == [3] and second['t'].tolist() == [6]
  halves = dict(second, log=torch.cat([first['log'], second['log']]),
                norms=torch.cat([first['norms'], second['norms']]))
  _assert_same(halves, whole, 'two halves')


# ---- 5. skips -----------------------------------------------------------------------------
SKIP_INDEX = [[[0, 1, 2, 3], [4, 3, 2, 1]],
              [[1, 2, 3, 4], [0, 5, 2, 4]],    # replica 1, step 1: row 5
              [[2, 3, 4, 0], [3, 1, 0, 2]]]


@pytest.mark.parametrize('poison', ['bad-index', 'nan-window'])
def test_a_skipped_step_leaves_that_replica_alone(poison):
  """Replica 1's minibatch of step 1 holds an index outside the rows (it reads nothing and
  yields NaN: the documented behaviour) or the only use of a window whose start holds a
  NaN: its step 1 is skipped, the others are the steps of a run without it."""
  c = _make(B, seed=15)
  index = torch.as_tensor(np.array(SKIP_INDEX, np.int32), device='cuda')
  if poison == 'bad-index':
    index[1, 1, 1] = ROWS
  else:
    y0 = c['y0'].clone()
    y0[5, 3] = float('nan')
    c = dict(c, y0=y0)
  state = _replica_state(c, 2, seed=7)
  rates = [[1e-3, 2e-3, 3e-3], [4e-3, 5e-3, 6e-3]]
  got = _rollout_run(c, index, rates, state, clip=1.0)
  assert not torch.isfinite(got['norms'][1, 1])
  assert torch.isnan(got['log'][1, 1]).all()
  assert torch.isfinite(got['log'][[0, 2], 1]).all() and torch.isfinite(got['log'][:, 0]).all()
  assert got['t'].tolist() == [3, 3 + 2]
  _assert_same(_replica_of(got, 0), _solo(c, state, 0, index, rates, clip=1.0), 'replica 0')
  kept = index[[0, 2], 1].contiguous()
  want = _rollout_run(c, kept, [[rates[1][0], rates[1][2]]],
                      tuple(x[1:2] for x in state), clip=1.0)
  for key in ('w', 'm', 'v', 't'):
    assert torch.equal(got[key][1:2], want[key]), key
  assert torch.equal(got['log'][[0, 2], 1], want['log'][:, 0])
  assert torch.equal(got['norms'][[0, 2], 1], want['norms'][:, 0])
  assert torch.isfinite(got['w']).all() and torch.isfinite(got['m']).all()


def test_population_trainer_counts_skipped_steps():
  equation, conservative, n, overrides, _ = B
  c = _make(B, seed=15)
  models = [_model(equation, conservative, n, overrides) for _ in range(2)]
  trainer = training.RolloutPopulationTrainer(models, models[0].hparams, clip_norm=1.0)
  index = torch.as_tensor(np.array(SKIP_INDEX, np.int32), device='cuda')
  index[1, 1, 1] = ROWS
  before = trainer.weights.clone()
  means, norms = trainer.run(_windows(c), 3, [1e-3, 2e-3], index, c['step_weights'])
  assert means.shape == (3, 2, T // EVERY) and norms.shape == (3, 2)
  assert trainer.skipped_steps.tolist() == [0, 1]
  assert trainer.adam_steps.tolist() == [3, 2]
  assert not np.isfinite(norms[1, 1]) and np.isnan(means[1, 1]).all()
  assert np.isfinite(np.delete(norms.ravel(), 3)).all()
  assert torch.isfinite(trainer.weights).all() and not torch.equal(trainer.weights, before)


# ---- 6. against the host loop -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_loop_and_float64():
  """The yardsticks of the multi-step bound, computed once: six RolloutTrainer.step calls
  (step means, final weights) and the same steps with gradients from
  ddd_train_rollout_loss_grad, the norm, the clip, the Adam state and the update in float64
  and the weights rounded to float32 for each kernel call.  clip_norm is the median of the
  six norms of an unclipped run.  Returns them and `floor`, the larger of their relative
  distances in the step means and in the final weights."""
  equation, conservative, n, overrides, _ = A
  model = _model(equation, conservative, n, overrides)
  c = _case(model, ROWS, T, EVERY, False, seed=16)
  windows = _windows(c)
  index = _index(6, BATCH, ROWS, seed=8)
  lr = 1e-3
  clip = float(_rollout_run(c, index, [[lr] * 6])['norms'].median())

  looped = training.RolloutTrainer(model, clip_norm=clip)
  assert torch.equal(looped.weights.detach(), c['flat'])
  loop_means = torch.stack([looped.step(windows, index[k].contiguous(), lr, c['step_weights'])
                            for k in range(6)]).double().cpu().numpy()
  loop_weights = looped.weights.detach().clone()
  assert looped.skipped_steps == 0

  w = c['flat'].double()
  m, v = torch.zeros_like(w), torch.zeros_like(w)
  means64 = []
  for k in range(6):
    means, g, _ = _run(dict(c, flat=w.float()), sample_index=index[k].contiguous())
    means64.append(means.double().cpu().numpy())
    g, t = g.double(), k + 1
    g = g * min(1.0, clip / (float(g.norm()) + 1e-12))
    m = m + (g - m) * (1 - BETAS[0])
    v = BETAS[1] * v + (1 - BETAS[1]) * g * g
    denom = v.sqrt() / np.sqrt(1 - BETAS[1] ** t) + EPS
    w = w - (lr / (1 - BETAS[0] ** t)) * m / denom
  means64 = np.stack(means64)
  floor = max(_rel(loop_weights, w),
              np.linalg.norm(loop_means - means64) / np.linalg.norm(means64))
  print('6 steps: RolloutTrainer.step loop against float64 Adam: floor {:.2e}'.format(floor))
  assert floor < 1e-3, floor
  return model, c, index, lr, clip, loop_means, loop_weights, means64, w, floor


def test_six_steps_match_the_step_loop():
  model, c, index, lr, clip, loop_means, loop_weights, means64, w64, floor = (
      _step_loop_and_float64())
  norms = _rollout_run(c, index, [[lr] * 6], clip=clip)['norms']
  print('norms {}, clip_norm {:.4g}'.format(norms[:, 0].tolist(), clip))
  assert (norms > clip).any()   # the clip acts
  fused = training.RolloutTrainer(model, clip_norm=clip)
  means = fused.run(_windows(c), 6, lr, index, c['step_weights'])
  assert tuple(means.shape) == (6, T // EVERY)
  assert fused.step_count == 6 and fused.skipped_steps == 0
  assert float(fused.optimizer.state[fused.weights]['step']) == 6.0
  assert fused.optimizer.param_groups[0]['lr'] == lr
  means = means.double().cpu().numpy()
  bound = max(1e-5, 4 * floor)
  for want_m, want_w, name in ((loop_means, loop_weights, 'RolloutTrainer.step loop'),
                               (means64, w64, 'float64 Adam')):
    err_m = np.linalg.norm(means - want_m) / np.linalg.norm(want_m)
    err_w = _rel(fused.weights.detach(), want_w)
    print('against {}: step means {:.2e}, weights {:.2e}, bound {:.2e}'.format(
        name, err_m, err_w, bound))
    assert err_m < bound and err_w < bound, (name, err_m, err_w, floor)
  # `step` goes on from the state `run` left
  fused.step(_windows(c), index[0].contiguous(), lr, c['step_weights'])
  assert fused.step_count == 7
  assert float(fused.optimizer.state[fused.weights]['step']) == 7.0


# ---- 7. forward only ----------------------------------------------------------------------
def test_forward_only_fills_the_means_and_nothing_else():
  c = _make(B, seed=17)
  state = _replica_state(c, 3, seed=9)
  w, m, v, t = (x.clone() for x in state)
  log, norms, last = _lib.train_rollout_run(
      c['cfg'], w, m, v, t, c['y0'], c['targets'], c['step_weights'], c['steps'], c['every'],
      c['dt'], None, None, t0=c['t0'], forcing=c['forcing'], nullspace=c['nullspace'],
      bias=c['bias'], forward_only=True, want_last_grad=True)
  assert norms is None and last is None and tuple(log.shape) == (1, 3, T // EVERY)
  for r in range(3):
    means, grad, _ = _run(dict(c, flat=state[0][r].contiguous()), want_grad=False)
    assert grad is None and torch.equal(log[0, r], means)
  assert not torch.equal(log[0, 0], log[0, 1])
  for after, before in zip((w, m, v, t), state):
    assert torch.equal(after, before)
  # the state may be left out altogether
  log_none, _, _ = _lib.train_rollout_run(
      c['cfg'], w, None, None, None, c['y0'], c['targets'], c['step_weights'], c['steps'],
      c['every'], c['dt'], None, None, t0=c['t0'], forcing=c['forcing'],
      nullspace=c['nullspace'], bias=c['bias'], forward_only=True)
  assert torch.equal(log_none, log)


# ---- 8. shared weights --------------------------------------------------------------------
def test_population_trainer_fine_tunes_its_own_weights():
  hp = make_hparams('burgers', conservative=False, num_points=32, resample_factor=4)
  models = _models('burgers', False, 32, replicas=2)
  c = _case(models[0], ROWS, T, EVERY, False, seed=18)
  population = training.PopulationTrainer(models, hp)
  rollout = population.rollout_trainer(clip_norm=1.0)
  assert rollout.weights.data_ptr() == population.weights.data_ptr()
  assert rollout.weights is population.weights
  assert rollout.adam_steps.tolist() == [0, 0] and not rollout.adam_m.any()
  before = population.weights.clone()
  losses = rollout.loss(_windows(c))
  means, norms = rollout.run(_windows(c), 3, [1e-3, 2e-3], _index(3, BATCH, ROWS, seed=10))
  assert np.isfinite(means).all() and np.isfinite(norms).all()
  assert rollout.adam_steps.tolist() == [3, 3] and rollout.skipped_steps.tolist() == [0, 0]
  assert not torch.equal(population.weights[0], before[0])
  assert not torch.equal(population.weights[1], before[1])
  assert rollout.loss(_windows(c)).shape == (2, T // EVERY)
  assert not np.array_equal(rollout.loss(_windows(c)), losses)
  reference = _burgers_reference()
  got = evaluation.evaluate_population(population.rollout_population(), hp, reference,
                                       keep_trajectories=True)
  exported = rollout.export()
  for r, model in enumerate(exported):
    np.testing.assert_array_equal(model_lib.model_weights(model),
                                  population.weights[r].cpu().numpy())
  _assert_results_equal(got, evaluation.evaluate_population(
      exported, hp, reference, keep_trajectories=True, launch='population'))


# ---- 9. end to end ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fine_tuning_fixture():
  """The fixture of test_gpu_train_rollout.test_fine_tune_on_rollouts_end_to_end."""
  hp = make_hparams('burgers', conservative=True, num_points=32, resample_factor=4,
                    eval_interval=3)
  _, coarse = equations.from_hparams(hp)
  y_exact, times = _exact_data(hp, 3, 10, 2)
  return hp, coarse, y_exact, times


HORIZONS = ((6, 4), (6, 12))
SCHEDULE = [(0, 4), (3, 4), (6, 4), (6, 12), (9, 12), (12, 12)]


def test_fine_tune_on_rollouts_fused(tmp_path):
  hp, coarse, y_exact, times = _fine_tuning_fixture()

  def run(name, **kwargs):
    model = model_lib.LearnedStencilModel(coarse, hp, init_seed=0)
    return training.fine_tune_on_rollouts(
        model, y_exact, times, hp, str(tmp_path / name), horizons=HORIZONS, save_every=2,
        batch=8, learning_rate=1e-3, seed=0, **kwargs)

  plain, fused = run('plain'), run('fused', fused=True)
  assert [(r['step'], r['num_steps']) for r in plain] == SCHEDULE
  assert [(r['step'], r['num_steps']) for r in fused] == SCHEDULE
  assert [len(r['step_means']) for r in fused] == [2, 2, 2, 6, 6, 6]
  assert fused[0] == plain[0] and fused[-1]['skipped_steps'] == 0
  want = np.array([r['loss'] for r in plain])
  got = np.array([r['loss'] for r in fused])
  floor = _step_loop_and_float64()[-1]
  bound = max(1e-5, 4 * floor)
  err = np.linalg.norm(got - want) / np.linalg.norm(want)
  print('fused against unfused losses: {:.2e}, bound {:.2e}\n{}\n{}'.format(
      err, bound, got.tolist(), want.tolist()))
  assert np.isfinite(got).all() and err < bound, (err, floor)
  assert fused[2]['loss'] < fused[0]['loss']
  for name in ('hparams.json', 'model.npz'):
    assert os.path.exists(str(tmp_path / 'fused' / name))


def test_fine_tune_population_on_rollouts(tmp_path):
  hp, coarse, y_exact, times = _fine_tuning_fixture()

  def run(name, seeds, rates):
    models = [model_lib.LearnedStencilModel(coarse, hp, init_seed=s) for s in seeds]
    dirs = [str(tmp_path / name / 'replica{}'.format(r)) for r in range(len(seeds))]
    rows = training.fine_tune_population_on_rollouts(
        models, y_exact, times, hp, dirs, HORIZONS, 2, 8, rates, seed=0, clip_norm=1.0)
    return rows, dirs

  rows, dirs = run('two', [0, 1], [1e-3, 3e-3])
  solo, solo_dirs = run('one', [0], [1e-3])
  assert len(rows) == 2 and len(solo) == 1
  for replica_rows in rows:
    assert [(r['step'], r['num_steps']) for r in replica_rows] == SCHEDULE
    assert np.isfinite([r['loss'] for r in replica_rows]).all()
    assert replica_rows[-1]['skipped_steps'] == 0
  assert rows[0] != rows[1]
  for directory in dirs:
    for name in ('hparams.json', 'model.npz'):
      assert os.path.exists(os.path.join(directory, name))
  # replica 0 of two is the population of one, bit for bit
  assert json.dumps(rows[0]) == json.dumps(solo[0])
  with np.load(os.path.join(dirs[0], 'model.npz')) as a, \
       np.load(os.path.join(solo_dirs[0], 'model.npz')) as b, \
       np.load(os.path.join(dirs[1], 'model.npz')) as other:
    for key in a.files:
      np.testing.assert_array_equal(a[key], b[key])
    assert any(not np.array_equal(a[key], other[key]) for key in a.files)
  with pytest.raises(ValueError, match='one checkpoint directory'):
    training.fine_tune_population_on_rollouts(
        [model_lib.LearnedStencilModel(coarse, hp, init_seed=0)], y_exact, times, hp, dirs,
        HORIZONS, 2, 8, [1e-3])
