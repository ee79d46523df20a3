"""The optimiser loop on the device (ddd_train_run, Trainer.run, training_loop(fused=True))
on the GPU: the gradient and the log of a step against ddd_train_loss_grad /
ddd_train_unrolled_loss_grad bit for bit, the fused Adam update against a float64
evaluation of its formulas, several steps against the existing Trainer.step loop,
continuity, determinism and error_max decided on the device."""
import copy
import functools

import numpy as np
import pytest
import torch

from helpers import make_hparams
from test_gpu_training import _model, _setup, _run
from test_gpu_train_unrolled import _setup as _setup_unrolled, _run as _run_unrolled
from ddd1d_amd import _lib, model as model_lib, training

pytestmark = pytest.mark.gpu

BETAS = (0.9, 0.99)
EPS = 1e-8


def _index(steps, batch, rows, seed=0):
  rs = np.random.RandomState(seed)
  return torch.as_tensor(rs.randint(0, rows, size=(steps, batch)).astype(np.int32),
                         device='cuda')


def _train_run(s, index, rates, weights=None, m=None, v=None, **kwargs):
  """_lib.train_run on copies: (weights, m, v, log, last_grad)."""
  w = (s['flat'] if weights is None else weights).clone()
  m = torch.zeros_like(w) if m is None else m.clone()
  v = torch.zeros_like(w) if v is None else v.clone()
  log, last = _lib.train_run(
      s['cfg'], w, m, v, s['y'], s['labels'], s['baseline'], index, rates, s['floor'],
      s['coef_abs'], s['coef_rel'], betas=BETAS, epsilon=EPS, nullspace=s['nullspace'],
      bias=s['bias'], want_last_grad=True, **kwargs)
  return w, m, v, log, last


def _rel(got, want):
  return ((got.double() - want.double()).norm() / want.double().norm()).item()


# ---- 1. one step: the gradient and the log are those of ddd_train_loss_grad ----

@pytest.mark.parametrize('equation,conservative,n,overrides,rows,batch', [
    ('burgers', False, 32, dict(), 12, 6),
    # VALU-only route at the largest N
    ('ks', False, 256, dict(kernel_size=7, filter_size=64, num_layers=1), 12, 6),
    # more samples than slabs (512 workgroups)
    ('burgers', False, 32, dict(), 700, 600),
    # the MFMA route on all four wavefronts (four 32-row tiles); last, so that the
    # cases above keep their ids
    ('burgers', False, 128, dict(), 12, 6),
])
def test_one_step_gradient_and_log_are_exact(equation, conservative, n, overrides, rows, batch):
  model = _model(equation, conservative, n, overrides)
  s = _setup(model, rows, seed=4)
  index = _index(1, batch, rows, seed=1)
  means, grad, _ = _run(s, sample_index=index[0].contiguous())
  w, m, v, log, last = _train_run(s, index, [1e-3])
  assert torch.equal(last, grad)
  assert torch.equal(log[0], means)
  assert torch.isfinite(w).all() and not torch.equal(w, s['flat'])


# ---- 2. one step: the update ----

def test_one_step_update_matches_float64_formulas():
  """Bound per vector: max(1e-6, 4 x floor) relative in norm, floor = the distance of
  torch.optim.Adam in float32 (single-tensor path, same gradient and state) from the
  float64 evaluation of the formulas on the float32 inputs; a floor above 1e-5 fails.
  The weights move by about lr per element, far less than their norm, so the update
  itself (new weights minus old) is checked too: each new weight is one float32 rounding
  (2^-24 relative to the weight) away from the exact sum, the bound is four times that,
  relative to the norm of the update, plus 1e-5 for the few roundings of the step."""
  model = _model('burgers', False, 32, dict())
  s = _setup(model, 12, seed=5)
  index = _index(1, 6, 12, seed=2)
  _, g, _ = _run(s, sample_index=index[0].contiguous())
  rs = np.random.RandomState(3)
  scale = g.abs().mean().item()
  m0 = torch.as_tensor((scale * rs.randn(g.numel())).astype(np.float32), device='cuda')
  v0 = torch.as_tensor((scale ** 2 * rs.uniform(0.1, 2.0, g.numel())).astype(np.float32),
                       device='cuda')
  lr, first = 1e-2, 4
  w, m, v, _, last = _train_run(s, index, [lr], m=m0, v=v0, first_step=first)
  assert torch.equal(last, g)

  t = first + 1
  g64, w0 = g.double(), s['flat'].double()
  m64 = m0.double() + (g64 - m0.double()) * (1 - BETAS[0])
  v64 = BETAS[1] * v0.double() + (1 - BETAS[1]) * g64 * g64
  denom = v64.sqrt() / np.sqrt(1 - BETAS[1] ** t) + EPS
  w64 = w0 - (lr / (1 - BETAS[0] ** t)) * m64 / denom

  param = torch.nn.Parameter(s['flat'].clone())
  adam = torch.optim.Adam([param], lr=lr, betas=BETAS, eps=EPS, foreach=False)
  adam.state[param] = dict(step=torch.tensor(float(first)), exp_avg=m0.clone(),
                           exp_avg_sq=v0.clone())
  param.grad = g.clone()
  adam.step()
  state = adam.state[param]
  for name, got, want, torch_got in (('weights', w, w64, param.detach()),
                                     ('m', m, m64, state['exp_avg']),
                                     ('v', v, v64, state['exp_avg_sq'])):
    floor = _rel(torch_got, want)
    err = _rel(got, want)
    print('{}: err {:.2e}, torch.optim.Adam float32 floor {:.2e}'.format(name, err, floor))
    assert floor < 1e-5, (name, floor)
    assert err < max(1e-6, 4 * floor), (name, err, floor)
  update = w64 - w0
  rounding = 2.0 ** -24 * w0.norm().item() / update.norm().item()
  err = _rel(w.double() - w0, update)
  print('update: err {:.2e}, rounding of the weights {:.2e}'.format(err, rounding))
  assert err < 1e-5 + 4 * rounding, (err, rounding)


# ---- 3. / 4. several steps against the existing loop ----

def _trainer_setup(error_max=0.0, seed=6):
  model = _model('burgers', False, 32, dict())
  s = _setup(model, 12, seed=seed)
  hp = model.hparams
  hp.absolute_error_weight, hp.relative_error_weight = 1.0, 1.0
  hp.space_derivatives_weight, hp.time_derivative_weight = 1.0, 1.0
  hp.error_floor = list(s['floor'])
  hp.error_scale = list(np.concatenate([s['coef_abs'], s['coef_rel']]))
  hp.error_max = error_max
  hp.learning_rates = [1e-3, 1e-4]
  hp.learning_stops = [3, 6]
  data = model_lib.DeviceDataset(s['y'], s['labels'], s['baseline'], 6, True, 0)
  return model, hp, s, data


def _state(trainer):
  st = trainer.optimizer.state[trainer.weights]
  return trainer.weights.detach(), st['exp_avg'], st['exp_avg_sq']


@functools.lru_cache(maxsize=None)
def _step_loop_and_float64(steps):
  """The yardstick of the multi-step bounds, computed once per length: `steps` x
  Trainer.step (losses, final weights) and the same steps with gradients from
  ddd_train_loss_grad, the Adam state and update in float64 and the weights rounded to
  float32 for each kernel call.  Returns both and `floor`, the larger of their relative
  distances in the per-step losses and in the final weights."""
  model, hp, s, data = _trainer_setup()
  index = _index(steps, 6, 12, seed=7)
  looped = training.Trainer(model, hp)
  loop_losses = np.stack([looped.step(data, index[k].contiguous()) for k in range(steps)])
  loop_weights = looped.weights.detach().clone()

  floor_c, coef_abs, coef_rel = looped.coefficients(3)
  scale = np.array(hp.error_scale, np.float64).reshape(2, -1)
  w = s['flat'].double()
  m, v = torch.zeros_like(w), torch.zeros_like(w)
  losses = []
  for k in range(steps):
    means, g, _ = _lib.train_loss_grad(
        s['cfg'], w.float(), s['y'], s['labels'], s['baseline'], floor_c, coef_abs, coef_rel,
        nullspace=s['nullspace'], bias=s['bias'], sample_index=index[k].contiguous())
    losses.append(means.double().cpu().numpy() * scale)
    g, t = g.double(), k + 1
    m = m + (g - m) * (1 - BETAS[0])
    v = BETAS[1] * v + (1 - BETAS[1]) * g * g
    denom = v.sqrt() / np.sqrt(1 - BETAS[1] ** t) + EPS
    w = w - (training.learning_rate(hp, k) / (1 - BETAS[0] ** t)) * m / denom
  losses = np.stack(losses)
  floor = max(_rel(loop_weights, w),
              np.linalg.norm(loop_losses - losses) / np.linalg.norm(losses))
  print('{} steps: Trainer.step loop against float64 Adam: floor {:.2e}'.format(steps, floor))
  assert floor < 1e-3, floor
  return index, loop_losses, loop_weights, losses, w, floor


def _assert_near_the_loop(losses, weights, steps):
  _, loop_losses, loop_weights, losses64, w64, floor = _step_loop_and_float64(steps)
  bound = max(1e-5, 4 * floor)
  for want_l, want_w, name in ((loop_losses, loop_weights, 'Trainer.step loop'),
                               (losses64, w64, 'float64 Adam')):
    err_l = np.linalg.norm(losses - want_l) / np.linalg.norm(want_l)
    err_w = _rel(weights, want_w)
    print('against {}: losses {:.2e}, weights {:.2e}, bound {:.2e}'.format(
        name, err_l, err_w, bound))
    assert err_l < bound and err_w < bound, (name, err_l, err_w, floor)


def test_six_steps_match_the_step_loop():
  model, hp, _, data = _trainer_setup()
  index = _step_loop_and_float64(6)[0]
  fused = training.Trainer(model, hp)
  losses = fused.run(data, 6, index)
  assert losses.shape == (6, 2, 3) and fused.step_count == 6
  assert fused.optimizer.param_groups[0]['lr'] == 1e-4
  # (the rate changes inside the run: learning_stops = [3, 6])
  _assert_near_the_loop(losses, fused.weights.detach(), 6)


def test_continuity_and_determinism():
  model, hp, _, data = _trainer_setup()
  index = _step_loop_and_float64(6)[0]
  whole, again, halves = (training.Trainer(model, hp) for _ in range(3))
  log = whole.run(data, 6, index)
  log_again = again.run(data, 6, index)
  log_halves = np.concatenate([halves.run(data, 3, index[:3]), halves.run(data, 3, index[3:])])
  for other, other_log in ((again, log_again), (halves, log_halves)):
    for a, b in zip(_state(whole), _state(other)):
      assert torch.equal(a, b)
    np.testing.assert_array_equal(log, other_log)
    assert other.step_count == 6
    assert float(other.optimizer.state[other.weights]['step']) == 6.0


def test_step_and_run_interleave():
  model, hp, _, data = _trainer_setup()
  index = _step_loop_and_float64(4)[0]
  mixed = training.Trainer(model, hp)
  losses = [mixed.step(data, index[0].contiguous())[None]]
  losses.append(mixed.run(data, 2, index[1:3]))
  losses.append(mixed.step(data, index[3].contiguous())[None])
  assert mixed.step_count == 4
  assert float(mixed.optimizer.state[mixed.weights]['step']) == 4.0
  fused = training.Trainer(model, hp)
  fused_losses = fused.run(data, 4, index)
  assert fused.step_count == 4
  mixed_losses = np.concatenate(losses)
  floor = _step_loop_and_float64(4)[-1]
  bound = max(1e-5, 4 * floor)
  err_l = np.linalg.norm(mixed_losses - fused_losses) / np.linalg.norm(fused_losses)
  err_w = _rel(mixed.weights.detach(), fused.weights.detach())
  print('step, run(2), step against run(4): losses {:.2e}, weights {:.2e}, bound {:.2e}'.format(
      err_l, err_w, bound))
  assert err_l < bound and err_w < bound, (err_l, err_w, floor)
  _assert_near_the_loop(mixed_losses, mixed.weights.detach(), 4)
  _assert_near_the_loop(fused_losses, fused.weights.detach(), 4)


# ---- 5. error_max on the device ----

def _with(hp, **overrides):
  out = copy.deepcopy(hp)
  for name, value in overrides.items():
    setattr(out, name, value)
  return out


def test_error_max_is_decided_on_the_device():
  model, hp, s, data = _trainer_setup()
  index = _index(1, 6, 12, seed=8)
  first = index[0].contiguous()
  unclipped, _, _ = training.Trainer(model, hp).loss_and_grad(data, first, want_grad=False)
  hp.error_max = float(np.median(unclipped))
  two_call = training.Trainer(model, hp)
  per_head, grad, _ = two_call.loss_and_grad(data, first)
  # the precondition, on the existing two-call path: a clipped and an unclipped entry
  assert (per_head == hp.error_max).any() and (per_head < hp.error_max).any()
  plain_grad = training.Trainer(model, _with(hp, error_max=0.0)).loss_and_grad(
      data, first)[1]
  assert not torch.equal(grad, plain_grad)

  floor_c, coef_abs, coef_rel = two_call.coefficients(3)
  scale = np.array(hp.error_scale, np.float64).reshape(2, -1)
  kwargs = dict(error_scale=scale)
  _, _, _, log, last = _train_run(dict(s, floor=floor_c, coef_abs=coef_abs, coef_rel=coef_rel),
                                  index, [1e-3], error_max=hp.error_max, **kwargs)
  assert torch.equal(last, grad)
  np.testing.assert_array_equal(log[0].double().cpu().numpy() * scale, unclipped)
  losses = training.Trainer(model, hp).run(data, 1, index)
  np.testing.assert_array_equal(losses[0], per_head)
  assert losses.max() == hp.error_max

  # an error_max above every entry: the bits of error_max = 0
  six = _index(3, 6, 12, seed=9)
  s3 = dict(s, floor=floor_c, coef_abs=coef_abs, coef_rel=coef_rel)
  plain = _train_run(s3, six, [1e-3] * 3)
  high = _train_run(s3, six, [1e-3] * 3, error_max=2.0 * float(unclipped.max()) + 1.0,
                    **kwargs)
  for a, b in zip(plain, high):
    assert torch.equal(a, b)


# ---- 6. through time ----

def test_one_step_through_time_is_exact():
  model = _model('kdv', True, 32, dict(model_target='time_derivative', num_layers=4))
  s = _setup_unrolled(model, 12, 2, seed=1)
  index = _index(1, 6, 12, seed=3)
  means, grad, _ = _run_unrolled(s, sample_index=index[0].contiguous())
  w, _, _, log, last = _train_run(s, index, [1e-3], num_time_steps=2, time_step=s['dt'])
  assert tuple(log.shape) == (1,) + tuple(means.shape) and means.shape[-1] == 3 + 2
  assert torch.equal(last, grad)
  assert torch.equal(log[0], means)
  assert torch.isfinite(w).all() and not torch.equal(w, s['flat'])


# ---- 7. an index outside the dataset ----

@pytest.mark.parametrize('num_time_steps', [0, 2])
def test_bad_index_poisons_the_update(num_time_steps):
  """An index outside [0, S) in step 0 (the solo mirror of test_replicas_are_isolated,
  test_gpu_train_population.py): the kernel reads nothing for that sample; that step's
  logged means, the gradient and, through the update, the weights and the Adam state
  become NaN (the contract include/ddd1d.h states), and nothing behind them is touched."""
  model = _model('burgers', False, 32, dict())
  rows, batch, sentinel = 8, 4, -123.25
  if num_time_steps:
    s = _setup_unrolled(model, rows, num_time_steps, seed=4)
    kwargs = dict(num_time_steps=num_time_steps, time_step=s['dt'])
  else:
    s = _setup(model, rows, seed=4)
    kwargs = dict()
  index = _index(2, batch, rows, seed=8)
  index[0, 2] = rows   # out of range

  def padded(t):   # a sentinel row behind the vector
    return torch.stack([t, torch.full_like(t, sentinel)]).contiguous()
  rs = np.random.RandomState(1)
  w = padded(s['flat'])
  m = padded(torch.as_tensor(1e-3 * rs.randn(s['flat'].numel()).astype(np.float32),
                             device='cuda'))
  v = padded(torch.as_tensor(rs.uniform(1e-6, 1e-5, s['flat'].numel()).astype(np.float32),
                             device='cuda'))
  log, last = _lib.train_run(
      s['cfg'], w[0], m[0], v[0], s['y'], s['labels'], s['baseline'], index, [1e-3, 1e-3],
      s['floor'], s['coef_abs'], s['coef_rel'], betas=BETAS, epsilon=EPS,
      nullspace=s['nullspace'], bias=s['bias'], want_last_grad=True, **kwargs)
  assert tuple(log.shape) == (2, 2, 3 + num_time_steps)
  assert tuple(last.shape) == (s['flat'].numel(),)
  print('NaN in log[0] {} of {}, in the weights {} of {}'.format(
      int(torch.isnan(log[0]).sum()), log[0].numel(), int(torch.isnan(w[0]).sum()),
      w.shape[1]))
  assert torch.isnan(log[0]).all()
  for t in (w[0], m[0], v[0], last):
    assert torch.isnan(t).all()
  for t in (w, m, v):
    assert (t[1] == sentinel).all()


# ---- 8. training_loop(fused=True) ----

def test_training_loop_fused(tmp_path):
  """The shape of the reference's training_test: 100 random snapshots of 256 points,
  learning_stops = [20], eval_interval = 10."""
  snapshots = np.random.RandomState(0).randn(100, 256).astype(np.float32)
  hp = make_hparams('burgers', conservative=True, num_points=64, resample_factor=4,
                    learning_stops=[20], eval_interval=10)
  plain = training.training_loop(snapshots, str(tmp_path / 'plain'), hp)
  fused = training.training_loop(snapshots, str(tmp_path / 'fused'), hp, fused=True)
  assert [r['step'] for r in fused] == [r['step'] for r in plain] == [0, 10, 20]
  assert all(np.isfinite(r['loss']) for r in fused)
  assert fused[0] == plain[0]
  loaded = model_lib.LearnedStencilModel.load(str(tmp_path / 'fused'))
  assert all(np.isfinite(k).all() for k in loaded.conv_kernels)
