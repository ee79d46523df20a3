"""The training kernels' 32 -> 32 layers on v_mfma_f32_32x32x2_f32 beyond two 32-row
tiles (N = 96 ... 256 with 32 filters): tiles on wavefronts 2 and 3, a wavefront's second
trip through its tile loop, LDS rows longer than 64 points next to the staged kernels, two
staged layers at more than one tile.

1. Tile replication.  The kernels read only num_points of the grid from ddd_config, the
   convolutions are periodic and every per-point accumulation chain keeps its order (tap,
   then channel): a state tiled m times along x, on a copy of the N = 32 configuration with
   num_points = 32 m, runs at point x + 32 j the arithmetic of point x of the base call.
   Predictions and the state gradient are the base call's, tiled, bit for bit.
2. The VALU route (base N = 16) against the MFMA route (the state tiled to N = 32, 64) of
   the same net, bit for bit.
3. Parity with float64 torch.autograd through the restatements of test_gpu_training /
   test_gpu_result_vjp / test_gpu_train_unrolled at the shapes those files leave out, with
   their floor-scaled bound, and determinism."""

import functools

import numpy as np
import pytest
import torch

from helpers import assert_near_truth, rel_err
from test_gpu_training import restated_result, weighted, _model
from test_gpu_training import _setup as _setup_single, _run as _run_single
from test_gpu_result_vjp import _setup as _setup_vjp, _vjp, _floor_bound
from test_gpu_train_unrolled import _setup as _setup_unrolled, _run as _run_unrolled
from test_gpu_train_unrolled import _autograd as _autograd_unrolled
from ddd1d_amd import model as model_lib

pytestmark = pytest.mark.gpu


def _id(equation, conservative, overrides):
  return '{}-{}-{}'.format(equation, 'cons' if conservative else 'plain',
                           '-'.join('{}={}'.format(k, v) for k, v in overrides.items())
                           or 'default')


def _tiled_config(cfg, m):
  """A copy of cfg (never cfg itself: _vjp_setup caches the struct on the model) with
  num_points m times as large; everything else, dx included, is the base grid's."""
  big = type(cfg).from_buffer_copy(cfg)
  big.num_points = cfg.num_points * m
  return big


def _tile_x(t, m):
  """t [batch, x] or [batch, x, heads] tiled m times along x."""
  return t.repeat(*((1, m) + (1,) * (t.dim() - 2)))


def _tiled(s, m, keys):
  """The setup s with the configuration of m tiles and its tensors `keys` tiled."""
  big = dict(s, cfg=_tiled_config(s['cfg'], m))
  for key in keys:
    big[key] = _tile_x(s[key], m).contiguous()
  return big


def _weight_slices(model):
  offset = 0
  for l, (w, b) in enumerate(zip(model.conv_kernels, model.conv_biases)):
    for part, size in (('kernel', w.size), ('bias', b.size)):
      yield (l, part), slice(offset, offset + size)
      offset += size


def _bounded(got, want64, want32s, what):
  """_floor_bound, with the float32 floor and the error printed first."""
  norm = want64.norm().item()
  if norm > 0.0:
    floor32 = max((w32 - want64).norm().item() / norm for w32 in want32s)
    err = (got.double() - want64).norm().item() / norm
    print('{}: floor32 {:.2e}, error {:.2e}'.format(what, floor32, err))
  _floor_bound(got, want64, want32s, what)


def _vjp_autograd(model, s, dtype, device='cuda'):
  """(predictions, grad_y, grad_weights) of <predictions, cotangent> through the
  restatement."""
  y = s['y'].detach().to(device, dtype).requires_grad_(True)
  w = s['flat'].detach().to(device, dtype).requires_grad_(True)
  out = restated_result(model, y, w, dtype)
  (out * s['cot'].to(device, dtype)).sum().backward()
  return out.detach().double().cuda(), y.grad.double().cuda(), w.grad.double().cuda()


def _loss_autograd(model, s, dtype, device='cuda'):
  """(grad, head_means [2, H]) of the weighted loss through the restatement."""
  w = s['flat'].detach().to(device, dtype).requires_grad_(True)
  pred = restated_result(model, s['y'].to(device), w, dtype)
  labels, baseline = s['labels'].to(device, dtype), s['baseline'].to(device, dtype)
  floor = torch.as_tensor(s['floor'], dtype=dtype, device=device)
  weighted(pred, labels, baseline, floor,
           torch.as_tensor(s['coef_abs'], dtype=dtype, device=device),
           torch.as_tensor(s['coef_rel'], dtype=dtype, device=device)).backward()
  with torch.no_grad():
    me = (labels - pred) ** 2
    means = torch.stack([me.mean(dim=(0, 1)),
                         (me / ((labels - baseline) ** 2 + floor)).mean(dim=(0, 1))])
  return w.grad.double().cuda(), means.double().cuda()


# ---- 1. tile replication: bit identity ----

NETS = [
    # (equation, conservative, overrides), all with 32 filters at base N = 32
    ('burgers', False, dict()),
    ('burgers', True, dict(polynomial_accuracy_order=0)),
    # two staged layers
    ('kdv', True, dict(model_target='time_derivative', num_layers=4)),
    # the weight gradient's taps 4 .. 6: a second tap on wavefronts 0 .. 2
    ('kdv', False, dict(kernel_size=7, nonlinearity='relu6')),
    # wavefront 3 owns no tap
    ('burgers', True, dict(kernel_size=3, nonlinearity='softplus')),
]
NET_IDS = [_id(*net) for net in NETS]
TILES = [3, 4, 5, 8]   # N = 96, 128, 160, 256


@functools.lru_cache(maxsize=None)
def _base_vjp(net):
  equation, conservative, overrides = NETS[net]
  model = _model(equation, conservative, 32, overrides)
  s = _setup_vjp(model, 4, seed=1)
  out = _vjp(s, want_predictions=True)
  want64 = _vjp_autograd(model, s, torch.float64)[2]
  want32s = [_vjp_autograd(model, s, torch.float32)[2],
             _vjp_autograd(model, s, torch.float32, 'cpu')[2]]
  return s, out, want64, want32s


@functools.lru_cache(maxsize=None)
def _base_loss(net):
  equation, conservative, overrides = NETS[net]
  s = _setup_single(_model(equation, conservative, 32, overrides), 5, seed=1)
  return s, _run_single(s, want_grad=False, want_predictions=True)[2]


@functools.lru_cache(maxsize=None)
def _base_unrolled(net):
  equation, conservative, overrides = NETS[net]
  s = _setup_unrolled(_model(equation, conservative, 32, overrides), 3, 2, seed=1)
  return s, _run_unrolled(s, want_grad=False, want_predictions=True)[2]


@pytest.mark.parametrize('m', TILES)
@pytest.mark.parametrize('net', range(len(NETS)), ids=NET_IDS)
def test_tiled_vjp_is_the_base_call_tiled(net, m):
  s, (pred, grad_y, _), want64, want32s = _base_vjp(net)
  got_pred, got_y, got_w = _vjp(_tiled(s, m, ('y', 'cot')), want_predictions=True)
  assert got_pred.shape == (4, 32 * m, pred.shape[-1])
  assert torch.equal(got_pred, _tile_x(pred, m))
  assert torch.equal(got_y, _tile_x(grad_y, m))
  # every tile adds the base case's weight gradient: m x the base gradient, up to the
  # rounding of sums m times as long (not bitwise), under m x the base case's float32
  # floor; slice by slice at these N: test_vjp_matches_float64_autograd below
  _bounded(got_w, m * want64, [m * w32 for w32 in want32s], 'grad_weights, m = {}'.format(m))


@pytest.mark.parametrize('m', TILES)
@pytest.mark.parametrize('net', range(len(NETS)), ids=NET_IDS)
def test_tiled_loss_predictions_are_the_base_call_tiled(net, m):
  s, pred = _base_loss(net)
  _, _, got = _run_single(_tiled(s, m, ('y', 'labels', 'baseline')), want_grad=False,
                          want_predictions=True)
  # (the head means are sums of another length: not compared bitwise)
  assert got.shape == (5, 32 * m, pred.shape[-1])
  assert torch.equal(got, _tile_x(pred, m))


@pytest.mark.parametrize('m', TILES)
@pytest.mark.parametrize('net', range(len(NETS)), ids=NET_IDS)
def test_tiled_unrolled_predictions_are_the_base_call_tiled(net, m):
  s, pred = _base_unrolled(net)
  _, _, got = _run_unrolled(_tiled(s, m, ('y', 'labels', 'baseline')), want_grad=False,
                            want_predictions=True)
  # all heads, the two trajectory heads included
  assert got.shape == (3, 32 * m, pred.shape[-1])
  assert torch.equal(got, _tile_x(pred, m))


# ---- 2. the VALU route against the MFMA route of the same net ----

@pytest.mark.parametrize('m', [2, 4])
@pytest.mark.parametrize('equation,conservative,overrides', [
    ('burgers', False, dict()),
    ('kdv', False, dict(kernel_size=7, nonlinearity='relu6')),
], ids=['burgers', 'kdv-K7'])
def test_valu_route_equals_mfma_route(equation, conservative, overrides, m):
  """Base N = 16: no multiple of 32, every layer on the VALU.  Tiled to N = 32 and 64 the
  hidden layer runs on MFMA.  The float32 MFMA is an fmaf chain and both
  routes sum tap by tap, then channel by channel: the results agree bit for bit."""
  model = _model(equation, conservative, 16, overrides)
  s = _setup_vjp(model, 4, seed=1)
  pred, grad_y, _ = _vjp(s, want_predictions=True)
  got_pred, got_y, _ = _vjp(_tiled(s, m, ('y', 'cot')), want_predictions=True)
  print('VALU against MFMA route, N = {}: predictions differ by {:.2e}, grad_y by {:.2e} '
        '(max abs)'.format(16 * m, (got_pred - _tile_x(pred, m)).abs().max().item(),
                           (got_y - _tile_x(grad_y, m)).abs().max().item()))
  assert torch.equal(got_pred, _tile_x(pred, m))
  assert torch.equal(got_y, _tile_x(grad_y, m))


# ---- 3. parity with float64 autograd at the shapes the other files leave out ----

CONFIGS = [
    # (equation, conservative, N, overrides), all with 32 filters.  The float32 floors (every
    # test prints its own) are conditions, capped at 1e-2, and these inputs keep the
    # reference inside the cap.  Measured on an MI355X, in the order of the list -- worst
    # weight slice of the gradient in the loss / VJP / through-time test:
    #   2.1e-5 / 7.1e-6 / 7.6e-6,  1.2e-5 / 3.4e-6 / 7.2e-6,  3.8e-4 / 2.2e-4 / 3.1e-4,
    #   5.9e-6 / 3.0e-6 / 5.6e-6,  1.7e-3 / 4.2e-3 / 1.8e-3,  1.7e-4 / 6.8e-5 / 7.5e-5;
    # predictions (VJP test, norm-wise) and space / time heads (forward test, max-norm):
    #   5.0e-6, 1.1e-5 / 1.4e-6;  1.1e-6, 1.2e-6 / 3.1e-6;  6.8e-6, 5.7e-5 / 8.1e-6;
    #   8.1e-7, 2.2e-7 / 3.2e-6;  9.8e-5, 4.4e-5 / 1.0e-3;  3.4e-5, 9.7e-5 / 7.8e-6;
    # head means at most 4.9e-4 (KS), grad_y at most 3.6e-7.
    ('burgers', False, 96, dict()),
    ('burgers', True, 128, dict()),
    ('kdv', False, 160, dict(kernel_size=7, nonlinearity='tanh')),
    ('kdv', True, 192, dict(kernel_size=3, polynomial_accuracy_order=0)),
    ('ks', True, 256, dict(num_layers=4)),
    ('burgers', False, 256, dict()),
]
IDS = ['{}-N{}'.format(_id(e, c, o), n) for e, c, n, o in CONFIGS]


@pytest.mark.parametrize('equation,conservative,n,overrides', CONFIGS, ids=IDS)
def test_loss_gradient_and_head_means_match_float64_autograd(equation, conservative, n,
                                                             overrides):
  model = _model(equation, conservative, n, overrides)
  s = _setup_single(model, 5, seed=1)
  means, grad, _ = _run_single(s)
  want64 = _loss_autograd(model, s, torch.float64)
  runs32 = [_loss_autograd(model, s, torch.float32),
            _loss_autograd(model, s, torch.float32, 'cpu')]
  for what, sl in _weight_slices(model):
    _bounded(grad[sl], want64[0][sl], [r[0][sl] for r in runs32], what)
  _bounded(means, want64[1], [r[1] for r in runs32], 'head_means')


@pytest.mark.parametrize('equation,conservative,n,overrides', CONFIGS, ids=IDS)
def test_vjp_matches_float64_autograd(equation, conservative, n, overrides):
  model = _model(equation, conservative, n, overrides)
  s = _setup_vjp(model, 4, seed=1)
  pred, grad_y, grad_w = _vjp(s, want_predictions=True)
  out64, gy64, gw64 = _vjp_autograd(model, s, torch.float64)
  runs32 = [_vjp_autograd(model, s, torch.float32),
            _vjp_autograd(model, s, torch.float32, 'cpu')]
  _bounded(pred, out64, [r[0] for r in runs32], 'predictions')
  _bounded(grad_y, gy64, [r[1] for r in runs32], 'grad_y')
  for what, sl in _weight_slices(model):
    _bounded(grad_w[sl], gw64[sl], [r[2][sl] for r in runs32], what)


@pytest.mark.parametrize('equation,conservative,n,overrides', CONFIGS, ids=IDS)
def test_unrolled_gradient_and_head_means_match_float64_autograd(equation, conservative, n,
                                                                 overrides):
  model = _model(equation, conservative, n, overrides)
  s = _setup_unrolled(model, 5, 2, seed=1)
  means, grad, _ = _run_unrolled(s)
  want64 = _autograd_unrolled(model, s, torch.float64)
  runs32 = [_autograd_unrolled(model, s, torch.float32),
            _autograd_unrolled(model, s, torch.float32, 'cpu')]
  for what, sl in _weight_slices(model):
    _bounded(grad[sl], want64[0][sl], [r[0][sl] for r in runs32], what)
  _bounded(means, want64[1], [r[1] for r in runs32], 'head_means')


@pytest.mark.parametrize('equation,conservative,n,overrides', CONFIGS, ids=IDS)
def test_forward_parity_with_the_inference_kernels(equation, conservative, n, overrides):
  """The training kernels' predictions against model.space_derivatives and
  predict_time_derivative.  At these shapes the float32 noise of the formulas themselves
  exceeds the 1e-5 of the small-N files, so the bound is max(1e-5, 4 x floor), the floor
  being the larger distance of the float32 restatement (device, host) from the float64
  one; where the floor decides, the predictions are also within TRUTH_RATIO x floor of
  the float64 restatement."""
  model = _model(equation, conservative, n, overrides)
  s = _setup_vjp(model, 5)
  pred = _vjp(s, cot=None)[0].double().cpu()
  with torch.no_grad():
    want64 = restated_result(model, s['y'], s['flat'], torch.float64).cpu()
    want32s = [restated_result(model, s['y'], s['flat'], torch.float32).cpu(),
               restated_result(model, s['y'].cpu(), s['flat'].cpu(), torch.float32)]
  inference = {'space': model.space_derivatives(s['y']).double().cpu(),
               'time': model_lib.predict_time_derivative(s['y'], model).double().cpu()}
  for head, sel in (('space', np.s_[..., :-1]), ('time', np.s_[..., -1])):
    floor = max(rel_err(w32[sel], want64[sel]) for w32 in want32s)
    err = rel_err(pred[sel], inference[head])
    truth = rel_err(pred[sel], want64[sel])
    print('{} heads: floor32 {:.2e}, against the inference kernel {:.2e}, against the '
          'float64 restatement {:.2e}'.format(head, floor, err, truth))
    assert floor < 1e-2, (head, floor)
    assert err < max(1e-5, 4 * floor), (head, err, floor)
    if 4 * floor > 1e-5:
      assert_near_truth(pred[sel], want64[sel], floor, head)


def test_determinism_at_five_tiles():
  """N = 160: wavefront 0 makes a second trip through its tile loop."""
  equation, conservative, n, overrides = CONFIGS[2]
  assert n == 160
  model = _model(equation, conservative, n, overrides)
  s = _setup_vjp(model, 4, seed=1)
  first, again = _vjp(s, want_predictions=True), _vjp(s, want_predictions=True)
  assert all(torch.equal(a, b) for a, b in zip(first, again))
  s = _setup_single(model, 5, seed=1)
  first, again = _run_single(s, want_predictions=True), _run_single(s, want_predictions=True)
  assert all(torch.equal(a, b) for a, b in zip(first, again))
  s = _setup_unrolled(model, 3, 2, seed=1)
  first = _run_unrolled(s, want_predictions=True)
  again = _run_unrolled(s, want_predictions=True)
  assert all(torch.equal(a, b) for a, b in zip(first, again))
