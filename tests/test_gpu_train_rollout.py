"""Training on rollout error (ddd_train_rollout_loss_grad) on the GPU: the unforced forward
sweep bit for bit against the kernel through time, the forced one against the inference
integrator and a float64 restatement, the gradient and the step means against float64
torch.autograd through the restated midpoint unroll (plus RandomForcing), the adjoint
step by step against the composed torch route, determinism and the gather / NULL paths,
and fine_tune_on_rollouts end to end."""

import json
import os

import numpy as np
import pytest
import torch

from helpers import batch_forcing, make_hparams, measured_bound, random_phase_ic, rel_err
from test_gpu_training import restated_result, _model
from test_gpu_result_vjp import _restated_unroll, _floor_bound
from test_gpu_train_unrolled import _setup as _setup_unrolled, _run as _run_unrolled
from ddd1d_amd import _lib, equations, integrate, model as model_lib, training

pytestmark = pytest.mark.gpu

CONFIGS = [
    # (equation, conservative, N, overrides, forced): the smallest shapes where each branch
    # can go wrong -- VALU layers and the non-conservative state partials; the MFMA-staged
    # 32 -> 32 layers, the flux difference and the forcing; the minimum N; a direct time
    # derivative; tanh; coefficients without a projection
    ('burgers', False, 32, dict(), False),
    ('burgers', True, 64, dict(), True),
    ('kdv', False, 8, dict(model_target='space_derivatives', kernel_size=3, filter_size=16),
     False),
    ('kdv', True, 32, dict(model_target='time_derivative', num_layers=4), False),
    ('ks', True, 32, dict(nonlinearity='tanh'), False),
    ('burgers', True, 64, dict(polynomial_accuracy_order=0), False),
]
IDS = ['{}-{}-N{}-{}{}'.format(e, 'cons' if c else 'plain', n,
                               '-'.join('{}={}'.format(k, v) for k, v in o.items()) or 'default',
                               '-forced' if f else '')
       for e, c, n, o, f in CONFIGS]
FORCED = CONFIGS[1]

# The longest horizon of the gradient tests: the largest of 12, 24, 48 at which the float32
# restatement stays within 1e-3 of the float64 one for every configuration (a tenth of
# _floor_bound's cap), measured on the CPU before the kernel ran; the figures are in
# test_gradient_and_step_means_match_float64_autograd's docstring.
T_LONG = 48


def _forcing_value(model, params, t, dtype):
  """RandomForcing.__call__ (equations.py:214-219) per row at the times t [batch] in
  `dtype`: the waves on the reference grid, resampled the grid's way -- not the folded
  tables the kernel reads."""
  grid = model.equation.grid
  device = t.device
  a, omega, k, phi = (torch.as_tensor(np.asarray(params[key], np.float64), device=device)
                      for key in ('a', 'omega', 'k', 'phi'))
  ref_x = torch.as_tensor(grid.reference_x, dtype=torch.float64, device=device)
  spatial = (2 * np.pi * k[..., None] * ref_x / grid.period).to(dtype)
  phase = (omega.to(dtype) * t.to(dtype)[:, None])[..., None] + spatial + phi.to(dtype)[..., None]
  total = (a.to(dtype)[..., None] * torch.sin(phase)).sum(dim=-2)
  factor = grid.resample_factor
  if grid.resample_method == 'mean':
    return total.reshape(total.shape[0], -1, factor).mean(dim=-1)
  return total[:, ::factor]


def _unroll(model, y, w, steps, dtype, params=None, t0=None):
  """The model's midpoint trajectory [batch, x, steps] in torch: _restated_unroll, with
  the forcing added to both evaluations of a step where `params` are given."""
  if params is None:
    return _restated_unroll(model, y.to(dtype), w, steps, dtype)
  dt = model.equation.time_step
  y, out = y.to(dtype), []
  for s in range(steps):
    t = t0 + s * dt
    k1 = restated_result(model, y, w, dtype)[..., -1] + _forcing_value(model, params, t, dtype)
    k2 = (restated_result(model, y + (0.5 * dt) * k1, w, dtype)[..., -1] +
          _forcing_value(model, params, t + 0.5 * dt, dtype))
    y = y + dt * k2
    out.append(y)
  return torch.stack(out, dim=-1)


def _case(model, batch, steps, every, forced, seed=0, device='cuda'):
  """Window starts, targets near the float64 trajectory, random positive step weights and,
  where forced, forcing rows and per-row different non-zero start times."""
  y0 = torch.as_tensor(random_phase_ic(model.equation, batch, seed0=900 + seed),
                       device=device).contiguous()
  flat = torch.as_tensor(model_lib.model_weights(model), device=device)
  params = batch_forcing(batch, seed0=40 + seed) if forced else None
  t0 = (torch.as_tensor(0.3 + 0.7 * np.arange(batch), dtype=torch.float64, device=device)
        if forced else None)
  with torch.no_grad():
    traj = _unroll(model, y0, flat, steps, torch.float64, params, t0)
  rs = np.random.RandomState(200 + seed)
  saved = traj[..., every - 1::every].permute(0, 2, 1)   # [batch, saved, x]
  scale = float(saved.abs().amax().clamp_min(1e-3))
  targets = (saved + 0.3 * scale * torch.as_tensor(rs.randn(*saved.shape), device=device)
             ).float().contiguous()
  weights = torch.as_tensor(rs.uniform(0.5, 1.5, steps // every).astype(np.float32),
                            device=device)
  case = dict(model=model, y0=y0, flat=flat, params=params, t0=t0, steps=steps, every=every,
              targets=targets, step_weights=weights, dt=model.equation.time_step,
              truth=traj, forcing=None, cfg=None, nullspace=None, bias=None)
  if device == 'cuda':
    case['cfg'] = training._train_config(model)
    case['nullspace'], case['bias'] = model_lib._vjp_tables(model)
    if forced:
      tables = model_lib.forcing_kernel_tables(params, model.equation.grid)
      case['forcing'] = {key: torch.as_tensor(np.ascontiguousarray(value), device='cuda')
                         for key, value in tables.items()}
  return case


def _run(c, **kwargs):
  call = dict(t0=c['t0'], forcing=c['forcing'], nullspace=c['nullspace'], bias=c['bias'])
  call.update(kwargs)
  return _lib.train_rollout_loss_grad(c['cfg'], c['flat'], c['y0'], c['targets'],
                                      c['step_weights'], c['steps'], c['every'], c['dt'], **call)


def _autograd(c, dtype, device='cuda'):
  """(grad, step_means) of the weighted loss through the restatement, float64 on `device`."""
  model = c['model']
  w = c['flat'].detach().to(device, dtype).requires_grad_(True)
  t0 = None if c['t0'] is None else c['t0'].to(device)
  traj = _unroll(model, c['y0'].to(device), w, c['steps'], dtype, c['params'], t0)
  saved = traj[..., c['every'] - 1::c['every']].permute(0, 2, 1)
  means = ((saved - c['targets'].to(device, dtype)) ** 2).mean(dim=(0, 2))
  (c['step_weights'].to(device, dtype) * means).sum().backward()
  return w.grad.double(), means.detach().double()


def _check_gradient(c, grad, means=None):
  want64 = _autograd(c, torch.float64)
  runs32 = [_autograd(c, torch.float32), [t.cuda() for t in _autograd(c, torch.float32, 'cpu')]]
  model, offset = c['model'], 0
  for l, (w, b) in enumerate(zip(model.conv_kernels, model.conv_biases)):
    for part, size in (('kernel', w.size), ('bias', b.size)):
      sl = slice(offset, offset + size)
      offset += size
      _floor_bound(grad[sl], want64[0][sl], [r[0][sl] for r in runs32], (l, part))
  if means is not None:
    _floor_bound(means, want64[1], [r[1] for r in runs32], 'step_means')
  return want64, runs32


# ---- 1. forward, unforced -----------------------------------------------------------------
@pytest.mark.parametrize('steps', [1, 4, 8])
@pytest.mark.parametrize('equation,conservative,n,overrides,forced', CONFIGS, ids=IDS)
def test_unforced_trajectory_is_the_unrolled_kernels_bit_for_bit(equation, conservative, n,
                                                                 overrides, forced, steps):
  model = _model(equation, conservative, n, overrides)
  s = _setup_unrolled(model, 6, steps)
  _, _, pred = _run_unrolled(s, want_grad=False, want_predictions=True)
  want = pred[..., pred.shape[-1] - steps:].permute(0, 2, 1).contiguous()   # [batch, T, x]
  saved = steps
  means, grad, traj = _lib.train_rollout_loss_grad(
      s['cfg'], s['flat'], s['y'], torch.zeros((6, saved, n), device='cuda'),
      torch.ones(saved, device='cuda'), steps, 1, s['dt'], nullspace=s['nullspace'],
      bias=s['bias'], want_grad=False, want_trajectory=True)
  assert grad is None and traj.shape == (6, steps, n) and means.shape == (steps,)
  assert torch.isfinite(traj).all()
  assert torch.equal(traj, want)


@pytest.mark.parametrize('equation,conservative,n,overrides,forced', CONFIGS, ids=IDS)
def test_saved_rows_are_rows_of_the_run_that_saves_every_step(equation, conservative, n,
                                                              overrides, forced):
  model = _model(equation, conservative, n, overrides)
  every1 = _case(model, 5, 12, 1, False, seed=1)
  every3 = dict(every1, every=3, targets=every1['targets'][:, 2::3].contiguous(),
                step_weights=every1['step_weights'][2::3].contiguous())
  m1, _, t1 = _run(every1, want_grad=False, want_trajectory=True)
  m3, _, t3 = _run(every3, want_grad=False, want_trajectory=True)
  assert t3.shape == (5, 4, n)
  assert torch.equal(t3, t1[:, [2, 5, 8, 11]])
  assert torch.equal(m3, m1[[2, 5, 8, 11]])


# ---- 2. forward, forced -------------------------------------------------------------------
def test_forced_trajectory_matches_the_integrator_and_float64():
  equation, conservative, n, overrides, _ = FORCED
  model = _model(equation, conservative, n, overrides)
  steps, batch = 24, 4
  c = _case(model, batch, steps, 1, True, seed=2)
  _, _, traj = _run(c, want_grad=False, want_trajectory=True)
  with torch.no_grad():
    f32 = _unroll(model, c['y0'], c['flat'], steps, torch.float32, c['params'], c['t0'])
  truth = c['truth'].permute(0, 2, 1).cpu().numpy()   # [batch, T, x]
  bound = measured_bound(f32.permute(0, 2, 1).cpu().numpy(), truth, label='forced rollout:')
  err64 = rel_err(traj.cpu().numpy(), truth)
  # the inference integrator, one row at a time: each row has its own clock
  rows = []
  for i in range(batch):
    model.set_forcing({key: value[i:i + 1] for key, value in c['params'].items()})
    rows.append(model.integrate_fixed(c['y0'][i:i + 1], steps, dt=c['dt'],
                                      t0=float(c['t0'][i]), scheme='midpoint')[:, 0])
  model.set_forcing(None)
  fixed = torch.stack(rows).cpu().numpy()
  err_fixed = rel_err(traj.cpu().numpy(), fixed)
  print('forced rollout, T = {}: {:.2e} from float64, {:.2e} from integrate_fixed, bound '
        '{:.2e}'.format(steps, err64, err_fixed, bound))
  assert err64 < bound
  assert err_fixed < bound
  # the forcing is in it: the unforced call gives another trajectory
  _, _, plain = _run(c, forcing=None, t0=None, want_grad=False, want_trajectory=True)
  assert rel_err(plain.cpu().numpy(), truth) > 100 * bound


def test_longest_horizon_forward():
  steps, batch = _lib.MAX_ROLLOUT_STEPS, 3
  model = _model('burgers', True, 32, dict())
  c = _case(model, batch, steps, 1, True, seed=3)
  means, grad, traj = _run(c, want_grad=False, want_trajectory=True)
  assert grad is None and traj.shape == (batch, steps, 32)
  assert torch.isfinite(traj).all() and torch.isfinite(means).all()
  with torch.no_grad():
    f32 = _unroll(model, c['y0'], c['flat'], steps, torch.float32, c['params'], c['t0'])
  truth = c['truth'].permute(0, 2, 1).cpu().numpy()
  bound = measured_bound(f32.permute(0, 2, 1).cpu().numpy(), truth, label='T = 256 rollout:')
  err = rel_err(traj.cpu().numpy(), truth)
  print('forced rollout, T = {}: {:.2e} from float64, bound {:.2e}'.format(steps, err, bound))
  assert err < bound


# ---- 3. gradient and step means -----------------------------------------------------------
@pytest.mark.parametrize('steps,every', [(1, 1), (4, 1), (T_LONG, 1), (T_LONG, T_LONG // 4)])
@pytest.mark.parametrize('equation,conservative,n,overrides,forced', CONFIGS, ids=IDS)
def test_gradient_and_step_means_match_float64_autograd(equation, conservative, n, overrides,
                                                        forced, steps, every):
  """Per layer kernel and bias, and for step_means, within _floor_bound of float64
  autograd through the restated unroll.

  T_LONG: the float32 restatement against the float64 one on the CPU (batch 5, save_every 1,
  the worst layer part of each configuration, the order of CONFIGS):
    T = 12: 4.8e-7, 1.4e-6, 5.4e-7, 3.7e-6, 3.2e-6, 1.6e-6
    T = 24: 4.2e-6, 1.8e-6, 1.1e-6, 1.3e-5, 1.3e-5, 8.6e-6
    T = 48: 1.8e-6, 1.3e-6, 3.5e-6, 7.0e-6, 1.5e-5, 9.9e-5
  (step_means: 1.5e-7 at most) -- all below 1e-3, so T_LONG = 48."""
  model = _model(equation, conservative, n, overrides)
  c = _case(model, 5, steps, every, forced, seed=4)
  means, grad, _ = _run(c)
  assert torch.isfinite(grad).all() and grad.abs().max().item() > 0.0
  _check_gradient(c, grad, means)


@pytest.mark.parametrize('equation,conservative,n,overrides,forced', CONFIGS, ids=IDS)
def test_gradient_matches_the_unrolled_kernel_at_four_steps(equation, conservative, n,
                                                            overrides, forced):
  """ddd_train_unrolled_loss_grad with coef_abs = c_j on the integrated heads, every other
  coefficient 0 and labels = targets computes the same loss (unforced)."""
  steps = 4
  model = _model(equation, conservative, n, overrides)
  c = _case(model, 5, steps, 1, False, seed=5)
  means, grad, _ = _run(c)
  s = _setup_unrolled(model, 5, steps)
  first = s['labels'].shape[-1] - steps
  labels = s['labels'].clone()
  labels[..., first:] = c['targets'].permute(0, 2, 1)
  heads = first + steps
  coef_abs = np.zeros(heads)
  coef_abs[first:] = c['step_weights'].cpu().numpy()
  u = dict(s, y=c['y0'], labels=labels.contiguous(), coef_abs=coef_abs,
           coef_rel=np.zeros(heads))
  u_means, u_grad, _ = _run_unrolled(u)
  print('rollout vs unrolled kernel at T = 4: gradient bit-identical: {}, means: {}'.format(
      torch.equal(grad, u_grad), torch.equal(means, u_means[0, first:])))
  want64, runs32 = _check_gradient(c, grad, means)
  norm = want64[0].norm().item()
  floor32 = max((r[0] - want64[0]).norm().item() / norm for r in runs32)
  err = (grad.double() - u_grad.double()).norm().item() / norm
  assert err < max(1e-5, 4 * floor32), (err, floor32)
  _floor_bound(u_means[0, first:], want64[1], [r[1] for r in runs32], 'unrolled means')


# ---- 4. wiring ----------------------------------------------------------------------------
def test_adjoint_is_wired_saved_step_by_saved_step():
  steps, every = 4, 2
  model = _model('burgers', False, 32, dict())
  c = _case(model, 4, steps, every, False, seed=6)
  for j in range(steps // every):
    one_hot = torch.zeros(steps // every, device='cuda')
    one_hot[j] = 1.0
    one = dict(c, step_weights=one_hot)
    _, grad, _ = _run(one)
    # the composed route: the unroll in torch over ddd_result_vjp, the MSE of that step
    w = c['flat'].clone().requires_grad_(True)
    step_j = (j + 1) * every - 1
    traj = model_lib.differentiable_time_evolution(c['y0'], model, steps, w)[..., step_j]
    ((traj - c['targets'][:, j]) ** 2).mean().backward()
    want64 = _autograd(one, torch.float64)[0]
    _floor_bound(grad, want64, [w.grad.double(), _autograd(one, torch.float32)[0]],
                 ('saved step', j))


def test_forcing_changes_the_gradient_not_who_gets_one():
  equation, conservative, n, overrides, _ = FORCED
  model = _model(equation, conservative, n, overrides)
  c = _case(model, 4, 8, 2, True, seed=7)
  _, forced_grad, _ = _run(c)
  _, plain_grad, _ = _run(c, forcing=None, t0=None)
  assert not torch.equal(forced_grad, plain_grad)
  assert (forced_grad.double() - plain_grad.double()).norm() > 1e-3 * plain_grad.double().norm()
  offset = 0
  for w, b in zip(model.conv_kernels, model.conv_biases):
    for size in (w.size, b.size):
      sl = slice(offset, offset + size)
      offset += size
      assert forced_grad[sl].abs().max().item() > 0.0 and plain_grad[sl].abs().max().item() > 0.0


# ---- 5. determinism and paths -------------------------------------------------------------
def test_determinism_gather_and_null_paths():
  equation, conservative, n, overrides, _ = FORCED
  model = _model(equation, conservative, n, overrides)
  c = _case(model, 12, 4, 2, True, seed=8)
  m, g, p = _run(c, want_trajectory=True)
  m2, g2, p2 = _run(c, want_trajectory=True)
  assert torch.equal(m, m2) and torch.equal(g, g2) and torch.equal(p, p2)
  m_none, g_none, _ = _run(c, want_grad=False)
  assert g_none is None and torch.equal(m_none, m)
  _, g_notraj, _ = _run(c)
  assert torch.equal(g_notraj, g)
  # more samples than slabs
  forcing = dict(c['forcing'], **{key: c['forcing'][key].repeat(50, 1).contiguous()
                                  for key in ('amplitude', 'omega', 'phase', 'k_index')})
  big = dict(c, y0=c['y0'].repeat(50, 1).contiguous(),
             targets=c['targets'].repeat(50, 1, 1).contiguous(),
             t0=c['t0'].repeat(50).contiguous(), forcing=forcing)
  assert big['y0'].shape[0] == 600
  mb, gb, _ = _run(big)
  mb2, gb2, _ = _run(big)
  assert torch.equal(mb, mb2) and torch.equal(gb, gb2)
  assert torch.isfinite(gb).all() and torch.isfinite(mb).all()
  # the in-kernel gather against the call on the gathered rows: y0, targets, t0, forcing
  index = torch.tensor([7, 2, 2, 11, 0], dtype=torch.int32, device='cuda')
  m_idx, g_idx, p_idx = _run(c, sample_index=index, want_trajectory=True)
  rows = index.long()
  gathered = dict(c, y0=c['y0'][rows].contiguous(), targets=c['targets'][rows].contiguous(),
                  t0=c['t0'][rows].contiguous(),
                  forcing=dict(c['forcing'], **{key: c['forcing'][key][rows].contiguous()
                                                for key in ('amplitude', 'omega', 'phase',
                                                            'k_index')}))
  m_pre, g_pre, p_pre = _run(gathered, want_trajectory=True)
  assert torch.equal(m_idx, m_pre) and torch.equal(g_idx, g_pre) and torch.equal(p_idx, p_pre)
  assert torch.equal(p_idx[1], p[2]) and torch.equal(p_idx[3], p[11])
  bad = torch.tensor([0, 12], dtype=torch.int32, device='cuda')
  m_bad, _, p_bad = _run(c, sample_index=bad, want_grad=False, want_trajectory=True)
  assert torch.isnan(m_bad).all()
  assert torch.isnan(p_bad[1]).all() and torch.equal(p_bad[0], p[0])


# ---- 6. end to end ------------------------------------------------------------------------
def _exact_data(hp, samples, num_times, save_every):
  """Forced-Burgers exact data at the smallest size: integrate_exact_batch on the fine
  grid of hp from a warmed-up state, saved every save_every model steps."""
  fine, coarse = equations.from_hparams(hp)
  eqs = [type(fine)(**dict(fine.params(), random_seed=seed)) for seed in range(samples)]
  times = coarse.time_step * save_every * np.arange(num_times)
  warmup = 2.0
  result = integrate.integrate_exact_batch(eqs, times, warmup=warmup)
  return np.asarray(result['y']), warmup + times


def test_fine_tune_on_rollouts_end_to_end(tmp_path):
  hp = make_hparams('burgers', conservative=True, num_points=32, resample_factor=4,
                    eval_interval=3)
  _, coarse = equations.from_hparams(hp)
  y_exact, times = _exact_data(hp, 3, 10, 2)
  assert y_exact.shape == (3, 10, 128) and np.isfinite(y_exact).all()
  windows = training.make_rollout_windows(y_exact, times, hp, 4, 2)
  assert windows.num_windows == 24 and windows.y0.is_cuda

  def run(name):
    model = model_lib.LearnedStencilModel(coarse, hp, init_seed=0)
    return training.fine_tune_on_rollouts(
        model, y_exact, times, hp, str(tmp_path / name), horizons=((6, 4), (6, 12)),
        save_every=2, batch=8, learning_rate=1e-3, seed=0)

  rows = run('a')
  assert [(r['step'], r['num_steps']) for r in rows] == [
      (0, 4), (3, 4), (6, 4), (6, 12), (9, 12), (12, 12)]
  assert [len(r['step_means']) for r in rows] == [2, 2, 2, 6, 6, 6]
  losses = [r['loss'] for r in rows]
  print('rollout loss on the training windows: {}'.format(losses))
  assert np.isfinite(losses).all() and rows[-1]['skipped_steps'] == 0
  assert rows[2]['loss'] < rows[0]['loss'], rows
  # two seeded runs give bit-identical rows and weights
  assert json.dumps(run('b')) == json.dumps(rows)
  with np.load(str(tmp_path / 'a' / 'model.npz')) as a, \
       np.load(str(tmp_path / 'b' / 'model.npz')) as b:
    for key in a.files:
      np.testing.assert_array_equal(a[key], b[key])
  assert os.path.exists(str(tmp_path / 'a' / 'hparams.json'))
  loaded = model_lib.LearnedStencilModel.load(str(tmp_path / 'a'))
  assert len(loaded.conv_kernels) == hp.num_layers
  assert not np.array_equal(loaded.conv_kernels[0],
                            model_lib.LearnedStencilModel(coarse, hp, init_seed=0).conv_kernels[0])
  # a NaN target row: the step is skipped, the weights stay
  trainer = training.RolloutTrainer(loaded, hp, clip_norm=1.0)
  before = trainer.weights.detach().clone()
  trainer.step(windows, None, 1e-3)
  assert trainer.skipped_steps == 0 and not torch.equal(trainer.weights.detach(), before)
  before = trainer.weights.detach().clone()
  windows.targets[5] = float('nan')
  means = trainer.step(windows, None, 1e-3)
  assert trainer.skipped_steps == 1 and trainer.step_count == 1
  assert torch.isnan(means).all() and torch.equal(trainer.weights.detach(), before)
