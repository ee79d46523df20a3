"""The tangent-linear model on the GPU: ddd_result_jvp (model.tangent_result) against float64
forward mode through a restatement of predict_result, the adjoint identity against
ddd_result_vjp with no restatement, the indexing of tangents and samples, forward-mode
torch through the autograd function, ddd_tangent_rollout (model.tangent_time_evolution)
and evaluation.lyapunov_exponents."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import make_model, random_phase_ic
from test_gpu_training import restated_result
from test_gpu_result_vjp import _floor_bound
from ddd1d_amd import _lib, evaluation, model as model_lib

pytestmark = pytest.mark.gpu

CONFIGS = [
    # (equation, conservative, N, overrides, M)
    ('burgers', False, 8, dict(kernel_size=3, filter_size=16, nonlinearity='tanh'), 3),
    ('burgers', True, 32, dict(), 3),
    ('ks', True, 64, dict(polynomial_accuracy_order=0), 3),
    ('burgers', False, 32, dict(polynomial_accuracy_order=0,
                                ensure_unbiased_coefficients=True), 3),
    ('kdv', False, 96, dict(nonlinearity='relu6'), 3),
    ('kdv', True, 40, dict(), 3),
    ('ks', False, 64, dict(kernel_size=7, filter_size=64, num_layers=1), 3),
    ('kdv', True, 32, dict(model_target='time_derivative', num_layers=4), 3),
    ('burgers', False, 256, dict(model_target='space_derivatives', filter_size=64), 2),
]
IDS = ['{}-{}-N{}-{}'.format(e, 'cons' if c else 'plain', n,
                             '-'.join('{}={}'.format(k, v) for k, v in o.items()) or 'default')
       for e, c, n, o, _ in CONFIGS]
BATCH = 4


@functools.lru_cache(maxsize=None)
def _setup(index, batch=BATCH):
  """The model of CONFIGS[index], a batch of states, M state tangents per sample and M
  weight tangents of the weights' own scale, and a cotangent scaled per head.  Shared by
  the tests; nothing in it is modified."""
  equation, conservative, n, overrides, tangents = CONFIGS[index]
  model = make_model(equation, conservative=conservative, num_points=n,
                     resample_factor=4 if n < 256 else 2, **overrides)
  rs = np.random.RandomState(40 + index)
  y = torch.as_tensor(random_phase_ic(model.equation, batch, seed0=900 + index),
                      device='cuda').contiguous()
  flat = torch.as_tensor(model_lib.model_weights(model), device='cuda')
  ty = torch.as_tensor(rs.randn(batch, tangents, n).astype(np.float32), device='cuda')
  tw = torch.as_tensor(rs.randn(tangents, flat.numel()).astype(np.float32), device='cuda')
  tw = (tw * flat.abs().mean()).contiguous()
  heads = len(model.equation.DERIVATIVE_ORDERS) + 1
  cot = torch.as_tensor(rs.randn(batch, n, heads).astype(np.float32), device='cuda')
  with torch.no_grad():
    scale = restated_result(model, y, flat, torch.float64).abs().amax(dim=(0, 1))
  cot = (cot / scale.clamp_min(1e-3).float()).contiguous()
  nullspace, bias = model_lib._vjp_tables(model)
  return dict(model=model, cfg=model_lib._vjp_setup(model), nullspace=nullspace, bias=bias,
              y=y, flat=flat, ty=ty, tw=tw, cot=cot, M=tangents)


def _default_setup(equation, conservative, n, **overrides):
  model = make_model(equation, conservative=conservative, num_points=n, resample_factor=4,
                     **overrides)
  flat = torch.as_tensor(model_lib.model_weights(model), device='cuda')
  return model, flat


def _restated_jvp(s, dtype, device, with_y, with_w):
  """(predictions, tangents [batch, M, N, H]) by torch.func.jvp through restated_result."""
  model = s['model']
  y, w = s['y'].to(device, dtype), s['flat'].to(device, dtype)
  tans = []
  for j in range(s['M']):
    ty = s['ty'][:, j].to(device, dtype) if with_y else torch.zeros_like(y)
    tw = s['tw'][j].to(device, dtype) if with_w else torch.zeros_like(w)
    out, tan = torch.func.jvp(lambda yy, ww: restated_result(model, yy, ww, dtype), (y, w),
                              (ty, tw))
    tans.append(tan)
  return out.double().cuda(), torch.stack(tans, dim=1).double().cuda()


def _bound(want64, want32s, what):
  """max(1e-5, 4 x the float32 floor), relative to |want64|: _floor_bound's, for the
  comparisons whose two sides are both device results."""
  norm = want64.norm().item()
  floor32 = max((w32 - want64).norm().item() / norm for w32 in want32s)
  assert floor32 < 1e-2, (what, floor32)
  return max(1e-5, 4 * floor32), norm


# ---- a. parity with float64 forward mode ------------------------------------------------
@pytest.mark.parametrize('index', range(len(CONFIGS)), ids=IDS)
def test_jvp_matches_float64_forward_mode(index):
  s = _setup(index)
  fwd, _, _ = _lib.result_vjp(s['cfg'], s['flat'], s['y'], nullspace=s['nullspace'],
                              bias=s['bias'])
  for with_y, with_w in ((True, False), (False, True), (True, True)):
    what = 'state' * with_y + 'weights' * with_w
    pred, tan = model_lib.tangent_result(s['y'], s['ty'] if with_y else None, s['model'],
                                         s['flat'], s['tw'] if with_w else None)
    assert tan.shape == (BATCH, s['M']) + tuple(pred.shape[1:])
    assert torch.equal(pred, fwd), what   # bit for bit ddd_result_vjp's forward pass
    out64, tan64 = _restated_jvp(s, torch.float64, 'cuda', with_y, with_w)
    runs32 = [_restated_jvp(s, torch.float32, 'cuda', with_y, with_w),
              _restated_jvp(s, torch.float32, 'cpu', with_y, with_w)]
    _floor_bound(pred, out64, [r[0] for r in runs32], (what, 'predictions'))
    for h in range(tan.shape[-1]):   # per head: their scales differ by orders of magnitude
      _floor_bound(tan[..., h], tan64[..., h], [r[1][..., h] for r in runs32],
                   (what, 'tangent of head', h))
  if s['model'].hparams.model_target == 'time_derivative':
    assert tan[..., :-1].abs().max().item() == 0.0


# ---- b. the adjoint identity, with no restatement -----------------------------------------
def _autograd_inner_products(s, dtype, device):
  """<grad_y, ty_j> + <grad_w, tw_j> per tangent j, the gradients by autograd through the
  restatement in `dtype`, the inner products in float64 on the host."""
  y = s['y'].detach().to(device, dtype).requires_grad_(True)
  w = s['flat'].detach().to(device, dtype).requires_grad_(True)
  (restated_result(s['model'], y, w, dtype) * s['cot'].to(device, dtype)).sum().backward()
  return _inner_products(y.grad, w.grad, s)


def _inner_products(grad_y, grad_w, s):
  gy, gw = grad_y.double().cpu(), grad_w.double().cpu()
  ty, tw = s['ty'].double().cpu(), s['tw'].double().cpu()
  return torch.einsum('bn,bmn->m', gy, ty) + tw @ gw


@pytest.mark.parametrize('index', range(len(CONFIGS)), ids=IDS)
def test_adjoint_identity_against_the_vjp(index):
  """<c, J_y ty + J_w tw> from ddd_result_jvp against <grad_y, ty> + <grad_w, tw> from
  ddd_result_vjp, summed over the batch, for each of the M tangents.  The bound is 4 x the
  float32 floor of this inner product: the distance of its float32-autograd value (device
  and host) from its float64-autograd value, the largest over the M tangents, which are
  M draws of one quantity."""
  s = _setup(index)
  _, tan = model_lib.tangent_result(s['y'], s['ty'], s['model'], s['flat'], s['tw'])
  lhs = torch.einsum('bnh,bmnh->m', s['cot'].double().cpu(), tan.double().cpu())
  _, grad_y, grad_w = _lib.result_vjp(s['cfg'], s['flat'], s['y'], s['cot'],
                                      nullspace=s['nullspace'], bias=s['bias'])
  rhs = _inner_products(grad_y, grad_w, s)
  want64 = _autograd_inner_products(s, torch.float64, 'cuda')
  floor = max((_autograd_inner_products(s, torch.float32, device) - want64).abs().max().item()
              for device in ('cuda', 'cpu'))
  err = (lhs - rhs).abs().max().item()
  print('adjoint identity {}: |lhs - rhs| = {:.3e}, float32 floor {:.3e}, values {}'.format(
      IDS[index], err, floor, want64.tolist()))
  assert err <= 4 * floor, (err, floor)


# ---- c. indexing --------------------------------------------------------------------------
def test_each_tangent_alone_and_repeats():
  for index in (1, 5):   # the MFMA route and the VALU fallback
    s = _setup(index)
    pred, tan = model_lib.tangent_result(s['y'], s['ty'], s['model'], s['flat'], s['tw'])
    again = model_lib.tangent_result(s['y'], s['ty'], s['model'], s['flat'], s['tw'])
    assert torch.equal(pred, again[0]) and torch.equal(tan, again[1])
    for j in range(s['M']):
      _, alone = model_lib.tangent_result(s['y'], s['ty'][:, j:j + 1].contiguous(), s['model'],
                                          s['flat'], s['tw'][j:j + 1].contiguous())
      assert torch.equal(alone[:, 0], tan[:, j]), (index, j)


def test_thirty_two_tangents():
  s = _setup(1)
  n = s['y'].shape[1]
  rs = np.random.RandomState(7)
  ty = torch.as_tensor(rs.randn(BATCH, 32, n).astype(np.float32), device='cuda')
  _, tan = model_lib.tangent_result(s['y'], ty, s['model'], s['flat'])
  assert tan.shape[:2] == (BATCH, 32) and torch.isfinite(tan).all()
  for j in (0, 17, 31):
    _, alone = model_lib.tangent_result(s['y'], ty[:, j:j + 1].contiguous(), s['model'],
                                        s['flat'])
    assert torch.equal(alone[:, 0], tan[:, j]), j
  with pytest.raises(ValueError, match='tangents'):
    model_lib.tangent_result(s['y'], torch.zeros(BATCH, 33, n, device='cuda'), s['model'])


def test_a_workgroup_takes_a_second_sample():
  s = _setup(0)
  rows = [0, 511, 512, 514]
  y = torch.as_tensor(random_phase_ic(s['model'].equation, 515, seed0=2000), device='cuda')
  ty = torch.as_tensor(np.random.RandomState(8).randn(515, 1, y.shape[1]).astype(np.float32),
                       device='cuda')
  y[rows] = s['y']
  ty[rows] = s['ty'][:, :1]
  pred, tan = model_lib.tangent_result(y.contiguous(), ty.contiguous(), s['model'], s['flat'])
  small_pred, small_tan = model_lib.tangent_result(s['y'], s['ty'][:, :1].contiguous(),
                                                   s['model'], s['flat'])
  assert torch.equal(pred[rows], small_pred) and torch.equal(tan[rows], small_tan)
  again = model_lib.tangent_result(y.contiguous(), ty.contiguous(), s['model'], s['flat'])
  assert torch.equal(pred, again[0]) and torch.equal(tan, again[1])


def test_null_predictions_leave_their_buffer_alone():
  s = _setup(1)
  lib = _lib.load_library()
  _, want = model_lib.tangent_result(s['y'], s['ty'], s['model'], s['flat'])
  n, heads, tangents = s['y'].shape[1], want.shape[-1], s['M']
  # one allocation: where predictions would go, then the tangents
  buffer = torch.full((BATCH * n * heads * (1 + tangents),), 7.0, device='cuda')
  ws = torch.empty(lib.ddd_jvp_workspace_bytes(ctypes.byref(s['cfg']), BATCH, tangents),
                   dtype=torch.uint8, device='cuda')
  args = _lib.DDDJvpArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDJvpArgs)
  args.batch, args.tangents = BATCH, tangents
  args.weights, args.y = s['flat'].data_ptr(), s['y'].data_ptr()
  args.nullspace, args.bias = s['nullspace'].data_ptr(), s['bias'].data_ptr()
  args.tangent_y = s['ty'].data_ptr()
  args.predictions = None
  args.tangents_out = buffer.data_ptr() + 4 * BATCH * n * heads
  args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
  _lib.check(lib.ddd_result_jvp(ctypes.byref(s['cfg']), ctypes.byref(args),
                                _lib.current_stream()))
  assert (buffer[:BATCH * n * heads] == 7.0).all()
  assert torch.equal(buffer[BATCH * n * heads:].reshape(want.shape), want)


# ---- d. forward-mode torch ----------------------------------------------------------------
def test_forward_mode_torch_equals_tangent_result():
  import torch.autograd.forward_ad as fwad
  s = _setup(1)
  model, y, w = s['model'], s['y'], s['flat']
  ty, tw = s['ty'][:, 0].contiguous(), s['tw'][0].contiguous()
  pred, both = model_lib.tangent_result(y, ty[:, None], model, w, tw[None])
  _, only_y = model_lib.tangent_result(y, ty[:, None], model, w)
  _, only_w = model_lib.tangent_result(y, None, model, w, tw[None])
  # torch.func.jvp with respect to the inputs, the weights, and both
  out, tan = torch.func.jvp(lambda a: model_lib.differentiable_result(a, model, w), (y,), (ty,))
  assert torch.equal(out, pred) and torch.equal(tan, only_y[:, 0])
  out, tan = torch.func.jvp(lambda b: model_lib.differentiable_result(y, model, b), (w,), (tw,))
  assert torch.equal(out, pred) and torch.equal(tan, only_w[:, 0])
  out, tan = torch.func.jvp(lambda a, b: model_lib.differentiable_result(a, model, b), (y, w),
                            (ty, tw))
  assert torch.equal(out, pred) and torch.equal(tan, both[:, 0])
  # ... the time head alone
  out, tan = torch.func.jvp(lambda a: model_lib.differentiable_time_derivative(a, model, w),
                            (y,), (ty,))
  assert torch.equal(out, pred[..., -1]) and torch.equal(tan, only_y[:, 0, :, -1])
  # forward_ad dual tensors
  for use_y, use_w, want in ((True, False, only_y), (False, True, only_w), (True, True, both)):
    with fwad.dual_level():
      a = fwad.make_dual(y, ty) if use_y else y
      b = fwad.make_dual(w, tw) if use_w else w
      primal, tangent = fwad.unpack_dual(model_lib.differentiable_result(a, model, b))
    assert torch.equal(primal, pred) and torch.equal(tangent, want[:, 0]), (use_y, use_w)


def _restated_unroll(model, y, w, steps, dtype):
  dt = model.equation.time_step
  out = []
  for _ in range(steps):
    k1 = restated_result(model, y, w, dtype)[..., -1]
    k2 = restated_result(model, y + (0.5 * dt) * k1, w, dtype)[..., -1]
    y = y + dt * k2
    out.append(y)
  return torch.stack(out, dim=-1)


def test_time_evolution_under_forward_mode():
  s = _setup(1)
  model = s['model']
  ty, tw = s['ty'][:, 0].contiguous(), s['tw'][0].contiguous()
  out, tan = torch.func.jvp(
      lambda a, b: model_lib.differentiable_time_evolution(a, model, 2, b),
      (s['y'], s['flat']), (ty, tw))
  assert out.shape == tan.shape == (BATCH, s['y'].shape[1], 2)

  def reference(dtype, device):
    args = [t.to(device, dtype) for t in (s['y'], s['flat'], ty, tw)]
    got = torch.func.jvp(lambda a, b: _restated_unroll(model, a, b, 2, dtype),
                         tuple(args[:2]), tuple(args[2:]))
    return [g.double().cuda() for g in got]

  want64 = reference(torch.float64, 'cuda')
  runs32 = [reference(torch.float32, 'cuda'), reference(torch.float32, 'cpu')]
  _floor_bound(out, want64[0], [r[0] for r in runs32], 'trajectory')
  _floor_bound(tan, want64[1], [r[1] for r in runs32], 'trajectory tangent')


def test_backward_mode_is_unchanged():
  s = _setup(1)
  y = s['y'].clone().requires_grad_(True)
  w = s['flat'].clone().requires_grad_(True)
  out = model_lib.differentiable_result(y, s['model'], w)
  (out * s['cot']).sum().backward()
  pred, grad_y, grad_w = _lib.result_vjp(s['cfg'], s['flat'], s['y'], s['cot'],
                                         nullspace=s['nullspace'], bias=s['bias'],
                                         want_predictions=True)
  assert torch.equal(out.detach(), pred)
  assert torch.equal(y.grad, grad_y) and torch.equal(w.grad, grad_w)


# ---- e. the tangent rollout ---------------------------------------------------------------
def _restated_tangent_rollout(model, y, t, w, steps, dtype):
  """The midpoint recurrence of ddd_tangent_rollout over torch.func.jvp through the
  restatement, the M tangents of a sample stacked into the batch."""
  dt = model.equation.time_step
  b, m, n = t.shape
  f = lambda state: restated_result(model, state, w, dtype)[..., -1]
  rep = lambda a: a[:, None, :].expand(b, m, n).reshape(b * m, n)
  for _ in range(steps):
    k1, dk1 = torch.func.jvp(f, (rep(y),), (t.reshape(b * m, n),))
    y_mid = y + (0.5 * dt) * k1.reshape(b, m, n)[:, 0]
    t_mid = t + (0.5 * dt) * dk1.reshape(b, m, n)
    k2, dk2 = torch.func.jvp(f, (rep(y_mid),), (t_mid.reshape(b * m, n),))
    y = y + dt * k2.reshape(b, m, n)[:, 0]
    t = t + dt * dk2.reshape(b, m, n)
  return y, t


@pytest.mark.parametrize('index', [1, 2, 4], ids=[IDS[i] for i in (1, 2, 4)])
def test_tangent_rollout(index):
  s = _setup(index)
  model, steps = s['model'], 6
  y, t, w = s['y'][:3].contiguous(), s['ty'][:3].contiguous(), s['flat']
  state, tan = model_lib.tangent_time_evolution(y, t, model, steps, w)
  assert state.shape == y.shape and tan.shape == t.shape

  def reference(dtype, device):
    got = _restated_tangent_rollout(model, y.to(device, dtype), t.to(device, dtype),
                                    w.to(device, dtype), steps, dtype)
    return [g.double().cuda() for g in got]

  want64 = reference(torch.float64, 'cuda')
  runs32 = [reference(torch.float32, 'cuda'), reference(torch.float32, 'cpu')]
  _floor_bound(state, want64[0], [r[0] for r in runs32], 'state')
  _floor_bound(tan, want64[1], [r[1] for r in runs32], 'tangents')
  # the same recurrence composed from tangent_result calls
  loose_state, loose_tan = model_lib.tangent_time_evolution(y, t, model, steps, w, fused=False)
  for got, other, k, what in ((state, loose_state, 0, 'state'), (tan, loose_tan, 1, 'tangents')):
    bound, norm = _bound(want64[k], [r[k] for r in runs32], what)
    assert (got.double() - other.double()).norm().item() / norm < bound, what
  # the state does not depend on the tangents, nor a tangent on the others; repeats
  again = model_lib.tangent_time_evolution(y, t, model, steps, w)
  assert torch.equal(state, again[0]) and torch.equal(tan, again[1])
  for j in range(t.shape[1]):
    other = t[:, j:j + 1].contiguous() if j else (2.5 * t[:, :1]).contiguous()
    state_one, tan_one = model_lib.tangent_time_evolution(y, other, model, steps, w)
    assert torch.equal(state_one, state), j
    if j:
      assert torch.equal(tan_one[:, 0], tan[:, j]), j


def test_tangent_rollout_second_sample_per_workgroup():
  s = _setup(0)
  model = s['model']
  y = torch.as_tensor(random_phase_ic(model.equation, 515, seed0=2000), device='cuda')
  t = torch.as_tensor(np.random.RandomState(9).randn(515, 1, y.shape[1]).astype(np.float32),
                      device='cuda')
  rows = [0, 511, 512, 514]
  state, tan = model_lib.tangent_time_evolution(y, t, model, 2, s['flat'])
  small = model_lib.tangent_time_evolution(y[rows].contiguous(), t[rows].contiguous(), model, 2,
                                           s['flat'])
  assert torch.equal(state[rows], small[0]) and torch.equal(tan[rows], small[1])


# ---- f. Lyapunov exponents ----------------------------------------------------------------
def _restated_lyapunov(model, y, t, w, steps, stretch, dtype):
  """Benettin's method as evaluation.lyapunov_exponents runs it, over the restatement:
  stretches of the tangent rollout in `dtype`, the QR in float64."""
  growth = []
  for _ in range(steps // stretch):
    y, t = _restated_tangent_rollout(model, y, t, w, stretch, dtype)
    q, r = torch.linalg.qr(t.double().transpose(1, 2))
    growth.append(torch.log(torch.diagonal(r, dim1=1, dim2=2).abs()))
    t = q.transpose(1, 2).to(dtype)
  return y.double().cuda(), t.double().cuda(), torch.stack(growth).cuda()


@pytest.mark.parametrize('equation,conservative,n,overrides', [
    ('ks', True, 32, dict()),
    ('burgers', True, 32, dict()),
    ('kdv', False, 64, dict(nonlinearity='tanh')),
], ids=['ks-cons-N32', 'burgers-cons-N32', 'kdv-plain-N64-tanh'])
def test_lyapunov_exponents(equation, conservative, n, overrides):
  model, flat = _default_setup(equation, conservative, n, **overrides)
  batch, tangents, steps, stretch = 2, 3, 24, 6
  y0 = torch.as_tensor(random_phase_ic(model.equation, batch, seed0=950), device='cuda')
  got = evaluation.lyapunov_exponents(model, y0, tangents, steps, stretch, seed=3)
  dt = model.equation.time_step
  assert got['exponents'].shape == (batch, tangents)
  assert got['log_growth'].shape == (steps // stretch, batch, tangents)
  assert got['log_growth'].dtype == torch.float64
  assert got['state'].shape == (batch, n) and got['tangents'].shape == (batch, tangents, n)
  assert torch.equal(got['exponents'], got['log_growth'].sum(0) / (steps * dt))
  # the seeded draw, and the same tangents passed in
  t0 = torch.as_tensor(evaluation.lyapunov_initial_tangents(batch, tangents, n, seed=3),
                       device='cuda')
  passed = evaluation.lyapunov_exponents(model, y0, tangents, steps, stretch, tangents=t0,
                                         weights=flat)
  assert all(torch.equal(got[k], passed[k]) for k in got)

  def reference(dtype, device):
    return _restated_lyapunov(model, y0.to(device, dtype), t0.to(device, dtype),
                              flat.to(device, dtype), steps, stretch, dtype)

  want64 = reference(torch.float64, 'cuda')
  runs32 = [reference(torch.float32, 'cuda'), reference(torch.float32, 'cpu')]
  _floor_bound(got['state'], want64[0], [r[0] for r in runs32], 'state')
  _floor_bound(got['tangents'], want64[1], [r[1] for r in runs32], 'tangents')
  # the sums of log growth are ~1e-4 at this dt: an absolute bound
  sums64 = want64[2].sum(0)
  floor = max((r[2].sum(0) - sums64).abs().max().item() for r in runs32)
  err = (got['log_growth'].sum(0) - sums64).abs().max().item()
  print('log-growth sums {}: error {:.3e}, float32 floor {:.3e}, sums {}'.format(
      equation, err, floor, sums64.flatten().tolist()))
  assert floor < 1e-5, floor
  assert err <= 4 * floor, (err, floor)
  with pytest.raises(ValueError, match='multiple'):
    evaluation.lyapunov_exponents(model, y0, tangents, 25, stretch)
