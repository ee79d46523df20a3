"""The vector-Jacobian product kernel (ddd_result_vjp) and the torch.autograd functions
over it on the GPU: forward parity with the inference kernels, gradient parity with
float64 torch.autograd through a restatement of predict_result with respect to the state
and the weights, determinism and the NULL paths, the autograd binding, the midpoint
unroll of differentiable_time_evolution and an end-to-end fit of an integrated-solution
loss."""

import numpy as np
import pytest
import torch

from helpers import make_model, make_hparams, random_phase_ic, rel_err
from test_gpu_training import restated_result
from ddd1d_amd import _lib, equations, model as model_lib, training

pytestmark = pytest.mark.gpu

CONFIGS = [
    # (equation, conservative, N, overrides); the 32 -> 32 layers take the MFMA route
    # where N is a multiple of 32 and filter_size = 32, every other layer the VALU route
    ('burgers', False, 32, dict()),
    ('burgers', True, 64, dict(polynomial_accuracy_order=0)),
    ('kdv', False, 8, dict(model_target='space_derivatives', kernel_size=3, filter_size=16,
                           nonlinearity='tanh')),
    ('kdv', True, 32, dict(model_target='time_derivative', num_layers=4)),
    ('ks', False, 64, dict(kernel_size=7, filter_size=64, num_layers=1)),
    ('ks', True, 32, dict(polynomial_accuracy_order=0, ensure_unbiased_coefficients=False,
                          nonlinearity='tanh')),
    ('burgers', False, 32, dict(polynomial_accuracy_order=0,
                                ensure_unbiased_coefficients=True)),
    ('kdv', False, 64, dict(kernel_size=7, nonlinearity='relu6')),
    ('burgers', False, 256, dict(model_target='space_derivatives', filter_size=64)),
    ('burgers', True, 32, dict(kernel_size=3, nonlinearity='softplus')),
    ('ks', False, 64, dict(filter_size=16, nonlinearity='elu')),
]
IDS = ['{}-{}-N{}-{}'.format(e, 'cons' if c else 'plain', n,
                             '-'.join('{}={}'.format(k, v) for k, v in o.items()) or 'default')
       for e, c, n, o in CONFIGS]


def _model(equation, conservative, n, overrides):
  return make_model(equation, conservative=conservative, num_points=n,
                    resample_factor=4 if n < 256 else 2, **overrides)


def _setup(model, batch, seed=0):
  cfg = model_lib._vjp_setup(model)
  nullspace, bias = model_lib._vjp_tables(model)
  y = torch.as_tensor(random_phase_ic(model.equation, batch, seed0=700 + seed),
                      device='cuda').contiguous()
  flat = torch.as_tensor(model_lib.model_weights(model), device='cuda')
  heads = len(model.equation.DERIVATIVE_ORDERS) + 1
  rs = np.random.RandomState(seed)
  cot = torch.as_tensor(rs.randn(batch, y.shape[1], heads).astype(np.float32), device='cuda')
  with torch.no_grad():
    scale = restated_result(model, y, flat, torch.float64).abs().amax(dim=(0, 1))
  # cotangents scaled so that every head contributes alike
  cot = (cot / scale.clamp_min(1e-3).float()).contiguous()
  return dict(cfg=cfg, nullspace=nullspace, bias=bias, y=y, flat=flat, cot=cot)


def _vjp(s, cot='default', **kwargs):
  return _lib.result_vjp(s['cfg'], s['flat'], s['y'], s['cot'] if cot == 'default' else cot,
                         nullspace=s['nullspace'], bias=s['bias'], **kwargs)


def _floor_bound(got, want64, want32s, what):
  """rel. error of got against the float64 reference, bounded by max(1e-5, 4 x the
  float32 floor) measured under two reduction orders; the floor itself is capped."""
  norm = want64.norm().item()
  if norm == 0.0:
    assert got.abs().max().item() == 0.0, what
    return
  floor32 = max((w32 - want64).norm().item() / norm for w32 in want32s)
  assert floor32 < 1e-2, (what, floor32)
  err = (got.double() - want64).norm().item() / norm
  assert err < max(1e-5, 4 * floor32), (what, err, floor32)


@pytest.mark.parametrize('equation,conservative,n,overrides', CONFIGS, ids=IDS)
def test_forward_parity(equation, conservative, n, overrides):
  model = _model(equation, conservative, n, overrides)
  s = _setup(model, 5)
  pred, grad_y, grad_w = _vjp(s, cot=None)
  assert grad_y is None and grad_w is None
  pred = pred.double()
  if model.hparams.model_target == 'time_derivative':
    assert pred[..., :-1].abs().max().item() == 0.0
  else:
    want_space = model.space_derivatives(s['y']).double()
    assert rel_err(pred[..., :-1].cpu(), want_space.cpu()) < 1e-5
  want_time = model_lib.predict_time_derivative(s['y'], model).double()
  assert rel_err(pred[..., -1].cpu(), want_time.cpu()) < 1e-5


@pytest.mark.parametrize('equation,conservative,n,overrides', CONFIGS, ids=IDS)
def test_vjp_matches_float64_autograd(equation, conservative, n, overrides):
  model = _model(equation, conservative, n, overrides)
  s = _setup(model, 4, seed=1)
  pred, grad_y, grad_w = _vjp(s, want_predictions=True)

  def autograd(dtype, device='cuda'):
    y = s['y'].detach().to(device, dtype).requires_grad_(True)
    w = s['flat'].detach().to(device, dtype).requires_grad_(True)
    out = restated_result(model, y, w, dtype)
    (out * s['cot'].to(device, dtype)).sum().backward()
    return out.detach().double().cuda(), y.grad.double().cuda(), w.grad.double().cuda()

  out64, gy64, gw64 = autograd(torch.float64)
  runs32 = [autograd(torch.float32), autograd(torch.float32, 'cpu')]
  _floor_bound(pred, out64, [r[0] for r in runs32], 'predictions')
  _floor_bound(grad_y, gy64, [r[1] for r in runs32], 'grad_y')
  offset = 0
  for l, (w, b) in enumerate(zip(model.conv_kernels, model.conv_biases)):
    for part, size in (('kernel', w.size), ('bias', b.size)):
      sl = slice(offset, offset + size)
      offset += size
      _floor_bound(grad_w[sl], gw64[sl], [r[2][sl] for r in runs32], (l, part))


def test_determinism_and_null_paths():
  model = _model('burgers', False, 32, dict())
  s = _setup(model, 9, seed=2)
  pred, grad_y, grad_w = _vjp(s, want_predictions=True)
  again = _vjp(s, want_predictions=True)
  assert all(torch.equal(a, b) for a, b in zip((pred, grad_y, grad_w), again))
  _, none_y, only_w = _vjp(s, want_grad_y=False)
  assert none_y is None and torch.equal(only_w, grad_w)
  _, only_y, none_w = _vjp(s, want_grad_weights=False)
  assert none_w is None and torch.equal(only_y, grad_y)
  fwd, no_y, no_w = _vjp(s, cot=None)
  assert no_y is None and no_w is None and torch.equal(fwd, pred)
  # through the ABI: a NULL cotangent writes the predictions and nothing else
  import ctypes
  lib = _lib.load_library()
  heads = pred.shape[-1]
  out = torch.full((9, 32, heads), 7.0, device='cuda')
  ws = torch.empty(lib.ddd_vjp_workspace_bytes(ctypes.byref(s['cfg']), 9), dtype=torch.uint8,
                   device='cuda')
  args = _lib.DDDVjpArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDVjpArgs)
  args.batch = 9
  args.weights, args.y = s['flat'].data_ptr(), s['y'].data_ptr()
  args.nullspace, args.bias = s['nullspace'].data_ptr(), s['bias'].data_ptr()
  args.predictions = out.data_ptr()
  args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
  _lib.check(lib.ddd_result_vjp(ctypes.byref(s['cfg']), ctypes.byref(args),
                                _lib.current_stream()))
  assert torch.equal(out, pred)
  # a batch wider than the 512 workgroups: the slabs hold several samples each
  big = dict(s, y=s['y'].repeat(70, 1)[:600].contiguous(),
             cot=s['cot'].repeat(70, 1, 1)[:600].contiguous())
  _, gy_big, gw_big = _vjp(big)
  _, gy_big2, gw_big2 = _vjp(big)
  assert torch.equal(gy_big, gy_big2) and torch.equal(gw_big, gw_big2)
  assert torch.equal(gy_big[:9], grad_y)


def test_autograd_binding_matches_the_abi():
  model = _model('ks', True, 32, dict(polynomial_accuracy_order=0,
                                      ensure_unbiased_coefficients=False))
  s = _setup(model, 6, seed=3)
  y = s['y'].clone().requires_grad_(True)
  w = s['flat'].clone().requires_grad_(True)
  out = model_lib.differentiable_result(y, model, w)
  assert out.shape == (6, 32, 4)
  (out * s['cot']).sum().backward()
  pred, grad_y, grad_w = _vjp(s, want_predictions=True)
  assert torch.equal(out.detach(), pred)
  assert torch.equal(y.grad, grad_y) and torch.equal(w.grad, grad_w)
  # the model's own weights: a constant
  y2 = s['y'].clone().requires_grad_(True)
  (model_lib.differentiable_result(y2, model) * s['cot']).sum().backward()
  assert torch.equal(y2.grad, grad_y)
  # the time head alone: the cotangent of the other heads is zero
  y3 = s['y'].clone().requires_grad_(True)
  model_lib.differentiable_time_derivative(y3, model, w).sum().backward()
  cot_t = torch.zeros_like(s['cot'])
  cot_t[..., -1] = 1.0
  assert torch.equal(y3.grad, _vjp(s, cot=cot_t)[1])
  # double backward is refused
  y4 = s['y'].clone().requires_grad_(True)
  loss = (model_lib.differentiable_result(y4, model, w) * s['cot']).sum()
  (gy,) = torch.autograd.grad(loss, y4, create_graph=True)
  with pytest.raises(RuntimeError):
    gy.sum().backward()
  # bad weights are refused before any device work
  with pytest.raises(ValueError, match='weights'):
    model_lib.differentiable_result(s['y'], model, s['flat'][:-1])
  with pytest.raises(ValueError, match='weights'):
    model_lib.differentiable_result(s['y'], model, s['flat'].cpu())
  with pytest.raises(ValueError, match='weights'):
    model_lib.differentiable_result(s['y'], model, s['flat'].double())
  # training.Trainer.weights shares the layout
  trainer = training.Trainer(model)
  assert torch.equal(trainer.weights.detach(), s['flat'])


def _restated_unroll(model, y, w, steps, dtype):
  dt = model.equation.time_step
  out = []
  for _ in range(steps):
    k1 = restated_result(model, y, w, dtype)[..., -1]
    k2 = restated_result(model, y + (0.5 * dt) * k1, w, dtype)[..., -1]
    y = y + dt * k2
    out.append(y)
  return torch.stack(out, dim=-1)


@pytest.mark.parametrize('equation,conservative,overrides', [
    ('burgers', False, dict()),
    ('ks', True, dict(model_target='space_derivatives', nonlinearity='tanh')),
])
@pytest.mark.parametrize('steps', [1, 4])
def test_time_evolution_forward_and_gradient(equation, conservative, overrides, steps):
  model = _model(equation, conservative, 32, overrides)
  s = _setup(model, 4, seed=4)
  dt = model.equation.time_step
  traj = model_lib.differentiable_time_evolution(s['y'], model, steps)
  assert traj.shape == (4, 32, steps)
  want = model_lib.integrate_ode(model, s['y'], steps, dt)
  assert rel_err(traj.cpu(), want.cpu()) < 1e-5
  probe = torch.as_tensor(np.random.RandomState(5).randn(4, 32, steps).astype(np.float32),
                          device='cuda')
  y = s['y'].clone().requires_grad_(True)
  w = s['flat'].clone().requires_grad_(True)
  (model_lib.differentiable_time_evolution(y, model, steps, w) * probe).sum().backward()

  def autograd(dtype, device='cuda'):
    y0 = s['y'].detach().to(device, dtype).requires_grad_(True)
    w0 = s['flat'].detach().to(device, dtype).requires_grad_(True)
    (_restated_unroll(model, y0, w0, steps, dtype) * probe.to(device, dtype)).sum().backward()
    return y0.grad.double().cuda(), w0.grad.double().cuda()

  gy64, gw64 = autograd(torch.float64)
  runs32 = [autograd(torch.float32), autograd(torch.float32, 'cpu')]
  _floor_bound(y.grad, gy64, [r[0] for r in runs32], 'grad_y0')
  _floor_bound(w.grad, gw64, [r[1] for r in runs32], 'grad_weights')


def _fit(model, y0, target, steps, seed):
  torch.manual_seed(seed)
  w = torch.nn.Parameter(torch.as_tensor(model_lib.model_weights(model), device='cuda'))
  opt = torch.optim.Adam([w], lr=1e-3, betas=(0.9, 0.99))
  losses = []
  for _ in range(steps):
    opt.zero_grad()
    traj = model_lib.differentiable_time_evolution(y0, model, target.shape[-1], w)
    loss = ((traj - target) ** 2).mean()
    loss.backward()
    opt.step()
    losses.append(loss.item())
  with torch.no_grad():
    traj = model_lib.differentiable_time_evolution(y0, model, target.shape[-1], w)
    losses.append(((traj - target) ** 2).mean().item())
  return w.detach().clone(), losses


def test_integrated_solution_fit_end_to_end():
  """Adam on the reference's integrated-solution loss (num_time_steps, model.py:643-661):
  the MSE of a 4-step midpoint unroll against the exact solver's trajectory, resampled
  to the coarse grid."""
  hp = make_hparams('burgers', conservative=False, num_points=32, resample_factor=4)
  fine, coarse = equations.from_hparams(hp)
  model = model_lib.LearnedStencilModel(coarse, hp, init_seed=0)
  steps, dt = 4, coarse.time_step
  # Burgers starts from rest and its forcing drives it: the trajectory starts at t = 1
  times = np.concatenate([[0.0], 1.0 + dt * np.arange(steps + 1)])
  snaps = training.create_training_snapshots(fine, range(8), times)
  snaps = torch.as_tensor(snaps.reshape(8, steps + 2, -1)[:, 1:], device='cuda')
  coarse_snaps = model_lib._resample_device(snaps, 'subsample', 4, axis=2)
  y0 = coarse_snaps[:, 0].contiguous()
  target = coarse_snaps[:, 1:].permute(0, 2, 1).contiguous()   # [batch, x, T]
  w_a, losses = _fit(model, y0, target, 150, seed=0)
  ratio = losses[-1] / losses[0]
  print('integrated-solution loss {:.3e} -> {:.3e}, ratio {:.3f}'.format(
      losses[0], losses[-1], ratio))
  assert np.isfinite(losses).all()
  # final loss over the initial one after 150 steps: measured 0.066 on an MI355X
  # (7.8e-6 -> 5.2e-7); the bound leaves a factor of about four above it
  assert ratio < 0.25, losses[::10]
  # two seeded runs give bit-identical weights
  w_b, _ = _fit(model, y0, target, 20, seed=0)
  w_c, _ = _fit(model, y0, target, 20, seed=0)
  assert torch.equal(w_b, w_c)
