"""Which kernel each entry point runs: ddd_kernel_name after the call, for one model per route,
at a small and a large ensemble, under every ddd_set_kernel kind the model accepts (csrc/capi.hip:
plan_launch).  The large ensemble (8192 samples) is split into sample slabs on the one-launch-per-
substep / per-step paths; both sizes stay clear of the small-ensemble switches to two or four
wavefronts per group, which scale with the device's SIMD count."""
import numpy as np
import pytest

from helpers import make_model, random_phase_ic
from ddd1d_amd import equations, model as model_lib

pytestmark = pytest.mark.gpu

SMALL, LARGE = 37, 8192
KINDS = ('auto', 'generic', 'mfma', 'mfma64', 'mfma256', 'mfma64w32', 'mfma64w16')
ENTRIES = ('persistent', 'per_step', 'per_substep', 'float64', 'adaptive', 'time_derivative',
           'chained', 'ring')
NAMES = {'r64': 'mfma_f32_r64', 'r256': 'mfma_f32_r256', 'w32': 'mfma_f32_r64w32',
         'w16': 'mfma_f32_r64w16', 'h16': 'mfma_f32_r64h16', 'lean': 'valu_f32_lean',
         'stream': 'stream_fixed', 'weno': 'valu_f32_weno', 'generic': 'generic'}


def _models():
  return {
      'per_equation': lambda: make_model('burgers', True, num_points=64, resample_factor=2),
      'half': lambda: make_model('burgers', True, num_points=64, resample_factor=2, filter_size=16),
      'wide': lambda: make_model('ks', True, num_points=64, resample_factor=2,
                                 coefficient_grid_min_size=9),
      'big': lambda: make_model('burgers', True, num_points=64, resample_factor=2, kernel_size=7),
      'lean': lambda: make_model('burgers', True, num_points=64, resample_factor=2, num_layers=1),
      'stream_fixed': lambda: model_lib.BaselineModel(equations.KdVEquation(64), accuracy_order=1),
      'weno': lambda: model_lib.BaselineModel(equations.GodunovBurgersEquation(128), 3, weno=True),
      'generic': lambda: model_lib.BaselineModel(equations.GodunovBurgersEquation(96), 3, weno=True),
      'r256': lambda: make_model('burgers', True, num_points=128, resample_factor=2),
  }


def _all(token):
  return ' '.join([token] * len(ENTRIES))


# model -> kind -> one token per entry of ENTRIES; 'a/b': a at SMALL samples, b at LARGE.
# Kinds the model does not list are refused by ddd_set_kernel.  '-': not pinned here (the
# adaptive integrator under mfma64w32 runs the one-wavefront kernel: test_corrected_names).
ROUTES = {
    'per_equation': {
        'auto': 'w16/r64 r64 r64 r64 w16/r64 r64 r64 r64',
        'generic': _all('generic'), 'mfma': _all('r64'), 'mfma64': _all('r64'),
        'mfma256': _all('r256'),
        'mfma64w32': 'w32 w32 w32 w32 - w32 w32 w32',
        'mfma64w16': 'w16 r64 r64 r64 w16 r64 r64 r64',
    },
    'half': {
        'auto': 'w16/h16 h16 h16 h16 w16/h16 h16 h16 r64',
        'generic': _all('generic'), 'mfma': _all('h16'), 'mfma64': _all('h16'),
        'mfma256': _all('r256'),
        'mfma64w32': 'w32 w32 w32 w32 h16 w32 w32 w32',
        'mfma64w16': 'w16 h16 h16 h16 w16 h16 h16 h16',
    },
    'wide': {
        'auto': _all('r64'), 'generic': _all('generic'), 'mfma': _all('r64'),
        'mfma64': _all('r64'), 'mfma256': _all('r256'),
    },
    'big': {
        'auto': _all('r64'), 'generic': _all('generic'), 'mfma': _all('r64'),
        'mfma64': _all('r64'), 'mfma256': _all('r256'),
    },
    'lean': {
        'auto': 'lean r64 r64 r64 r64 r64 r64 r64',
        'generic': _all('generic'), 'mfma': _all('r64'), 'mfma64': _all('r64'),
        'mfma256': _all('r256'),
        'mfma64w32': 'w32 w32 w32 w32 - w32 w32 w32',
    },
    'stream_fixed': {
        'auto': 'lean stream stream r64 r64 stream stream stream',
        'generic': _all('generic'), 'mfma': _all('r64'), 'mfma64': _all('r64'),
        'mfma256': _all('r256'),
        'mfma64w32': 'w32 w32 w32 w32 - w32 w32 w32',
    },
    'weno': {'auto': _all('weno'), 'generic': _all('generic')},
    'generic': {'auto': _all('generic'), 'generic': _all('generic')},
    'r256': {'auto': _all('r256'), 'generic': _all('generic'), 'mfma': _all('r256'),
             'mfma256': _all('r256')},
}


def _substeps(model, y, dt, mode):
  """One midpoint step of rk_substep calls inside stream_fork .. stream_join."""
  import torch
  ystage, ynew = torch.empty_like(y), torch.empty_like(y)
  model.set_region_mode(mode)
  try:
    with model.chained_substeps():
      model.rk_substep(0.0, y, y_base=y, c1=0.5 * dt, y_out=ystage)
      model.rk_substep(0.5 * dt, ystage, acc_in=y, c2=dt, acc_out=ynew)
  finally:
    model.set_region_mode('auto')


def observe(model, batch):
  """{entry: kernel name after it} at `batch` samples under the model's current kind."""
  import torch
  y0 = random_phase_ic(model.equation, batch)
  y = torch.from_numpy(y0).cuda()
  dt = 1e-4
  seen = {}
  for mode in ('persistent', 'per_step', 'per_substep'):
    model.integrate_fixed(y, 2, dt=dt, launch_mode=mode)
    seen[mode] = model.kernel_name
  model.integrate_fixed(y.double(), 2, dt=dt, state_dtype='float64')
  seen['float64'] = model.kernel_name
  model.integrate_adaptive(y.double(), np.array([0.0, 1e-4]), max_step=1e-4)
  seen['adaptive'] = model.kernel_name
  model.time_derivative(y)
  seen['time_derivative'] = model.kernel_name
  _substeps(model, y, dt, 'auto')
  seen['chained'] = model.kernel_name
  _substeps(model, y, dt, 'ring')
  seen['ring'] = model.kernel_name
  torch.cuda.synchronize()
  return seen


def accepted(model, kind):
  try:
    model.set_kernel(kind)
    return True
  except Exception:   # (ddd_set_kernel refuses a kind the model has no kernel for)
    return False


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_route_table(route):
  model = _models()[route]()
  table = ROUTES[route]
  wrong = []
  for kind in KINDS:
    if not accepted(model, kind):
      if kind in table:
        wrong.append((kind, 'refused'))
      continue
    if kind not in table:
      wrong.append((kind, 'accepted'))
      continue
    for i, batch in enumerate((SMALL, LARGE)):
      seen = observe(model, batch)
      for entry, token in zip(ENTRIES, table[kind].split()):
        want = token.split('/')[min(i, token.count('/'))]
        if want != '-' and seen[entry] != NAMES[want]:
          wrong.append((kind, batch, entry, seen[entry], NAMES[want]))
  model.set_kernel('auto')
  assert not wrong, wrong


def test_corrected_names():
  """The name follows the most recent launch: ddd_set_kernel clears it (until the next launch
  the model's default is reported), and the adaptive integrator under mfma64w32 -- which has
  no split kernel -- reports the one-wavefront kernel it runs."""
  import torch
  model = _models()['per_equation']()
  y = torch.from_numpy(random_phase_ic(model.equation, SMALL)).cuda()
  model.integrate_fixed(y, 2, dt=1e-4)
  assert model.kernel_name == 'mfma_f32_r64w16'
  model.set_kernel('mfma64')
  assert model.kernel_name == 'mfma_f32_r64'
  model.set_kernel('mfma64w32')
  assert model.kernel_name == 'mfma_f32_r64w32'
  model.integrate_adaptive(y.double(), np.array([0.0, 1e-4]), max_step=1e-4)
  assert model.kernel_name == 'mfma_f32_r64'
  model.set_kernel('auto')
  assert model.kernel_name == 'mfma_f32_r64'
  for route, launch, name in (('lean', 'persistent', 'valu_f32_lean'),
                              ('stream_fixed', 'per_substep', 'stream_fixed')):
    model = _models()[route]()
    y = torch.from_numpy(random_phase_ic(model.equation, SMALL)).cuda()
    model.integrate_fixed(y, 2, dt=1e-4, launch_mode=launch)
    assert model.kernel_name == name
    model.set_kernel('mfma64')
    assert model.kernel_name == 'mfma_f32_r64', route
