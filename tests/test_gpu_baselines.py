"""The fixed-stencil / WENO baseline family (BaselineModel: every training label, baseline
trajectory and "exact" solution) on all of its kernels -- csrc/rhs_stream.h (substep and fused-step
kernels), rhs_lean.h, rhs_weno.h, rhs_generic.h and the tower-skipped MFMA path -- at the shapes
the neighbouring files do not reach:

1. every stencil width an accuracy order gives (G = 2 .. 8 on the streaming and lean kernels,
   mixed per-derivative widths, G = 9 .. 11 on the kernels behind them),
2. the tile walk of stream::fixed_step_kernel on a batch sized from the device (every block
   makes two trips, some three, the last tile is ragged, the last prefetch falls past the end),
3. the grid-size edges of the streaming kernels (G = N = 8, N % 8 != 0, N = 520 / 1020 / 1024),
4. NaN masks equal to the reference's on every baseline route,
5. rk_substep with aliased arrays (include/ddd1d.h: "y_out / acc_out may alias their inputs").

References: oracle/oracle.py in float32, helpers.baseline_rhs_f64 for the float32 noise floor
under it (helpers.measured_bound), and the other launch modes bit for bit.

Measured on one MI355X (102 tests): 1.1 s inside the whole suite, 3.3 s alone (pytest call times
summed; alone, the first test loads the library: 1.75 s); per-test maxima: tile walk 0.15 - 0.26 s,
spectral in-place case 0.36 s alone, everything else under 0.1 s.  Largest float32 oracle floor
per part: (1) 5.8e-6 (GodunovKS G = 6), wide stencils 6.3e-6 (KS G = 11), (2) 9.6e-6 (KS
N = 100), (3) 1.4e-3 (KdV N = 1020), (4) 3.8e-6; FLOOR_CEILING is 5e-3.  
"""
import numpy as np
import pytest

from helpers import (oracle, make_model, random_phase_ic, batch_forcing, baseline_spec,
                     baseline_rhs_f64, measured_bound, rel_err)
from ddd1d_amd import equations, model as model_lib

pytestmark = pytest.mark.gpu

TOL = 1e-5
SCHEMES = {'midpoint': oracle.SCHEME_MIDPOINT, 'bs3': oracle.SCHEME_BS3, 'rk4': oracle.SCHEME_RK4}
STREAMING = ('stream_fixed', 'valu_f32_lean')


def _baseline(cls_name, n, order, weno=False, seed=3):
  """(equation, model, oracle spec).  The spec comes from helpers.baseline_spec -- stencils
  per derivative, each centred by the oracle itself --, not from the model's zero-padded table."""
  eq = getattr(equations, cls_name)(n, random_seed=seed)
  model = model_lib.BaselineModel(eq, order, weno=weno)
  spec = dict(baseline_spec(eq, order), weno=bool(weno))
  return eq, model, spec


def _widths(spec):
  return [len(taps) for taps in spec['baseline_coefficients']]


def _rhs_bound(model, spec, y0, label, forcing=None, t=0.0):
  """time_derivative against the oracle at max(1e-5, 4 x the oracle's own float32 floor); the
  floor is printed.  Returns the bound (the trajectories are held to it too)."""
  got = model.time_derivative(y0, t).cpu().numpy()
  want = oracle.time_derivative(spec, t, y0, forcing)
  truth = baseline_rhs_f64(spec, y0, t, forcing)
  print('{} float32 floor {:.2e}'.format(label, rel_err(want, truth)))
  bound = measured_bound(want, truth, TOL, label, got=got)
  err = rel_err(got, want)
  assert err < bound, '{}: time_derivative {:.2e} from the oracle, bound {:.2e}'.format(
      label, err, bound)
  return bound


def _three_modes(model, y0, steps, dt, scheme, save_every, persistent=True):
  """{launch mode: (trajectory, kernel_name)}; the modes are asserted bit-identical."""
  runs = {}
  modes = ('per_substep', 'per_step') + (('persistent',) if persistent else ())
  for mode in modes:
    out = model.integrate_fixed(y0, steps, dt=dt, scheme=scheme, save_every=save_every,
                                launch_mode=mode).cpu().numpy()
    runs[mode] = (out, model.kernel_name)
  for mode in modes[1:]:
    np.testing.assert_array_equal(runs['per_substep'][0], runs[mode][0],
                                  err_msg='{} / per_substep vs {}'.format(scheme, mode))
  return runs


def _check_parity(cls_name, n, order, batch, dt_scale=1.0, names=STREAMING, persistent=True):
  """The assertions of parts 1 and 3 for one model: three launch modes bit-identical over
  midpoint / bs3 / rk4 (9 steps, every third saved), kernel names, right-hand side and the
  per_step trajectory of the first three samples against the oracle."""
  eq, model, spec = _baseline(cls_name, n, order)
  label = '{} N={} order {} G={} widths {}:'.format(cls_name, n, order, model.stencil_size,
                                                    _widths(spec))
  y0 = random_phase_ic(eq, batch)
  dt = dt_scale * eq.time_step
  bound = _rhs_bound(model, spec, y0, label)
  for scheme, sid in SCHEMES.items():
    runs = _three_modes(model, y0, 9, dt, scheme, 3, persistent)
    if names is STREAMING:
      # G = 2: step_supports() is false (the fused-step kernel reads aligned quads around
      # G >= 3 points), per_step then runs the substep chain: the streaming substep kernel
      assert runs['per_substep'][1] == 'stream_fixed', (label, runs['per_substep'][1])
      assert runs['per_step'][1] == 'stream_fixed', (label, runs['per_step'][1])
      if persistent and 64 % n == 0:
        assert runs['persistent'][1] == 'valu_f32_lean', (label, runs['persistent'][1])
    else:   # stencils wider than kGMax: the kernels behind the streaming ones
      for mode, (_, name) in runs.items():
        assert name not in STREAMING, (label, mode, name)
    want = oracle.integrate_fixed(spec, sid, 0.0, dt, 9, 3, y0[:3])
    assert np.isfinite(want).all(), label
    err = rel_err(runs['per_step'][0][:, :3], want)
    assert err < bound, '{} {}: per_step trajectory {:.2e} from the oracle, bound {:.2e}'.format(
        label, scheme, err, bound)


# ---- 1. every reachable stencil width ------------------------------------------------------
# (equation, lowest accuracy order that gives the width): G = max per-derivative width.  For
# G > 3 the lowest order always has MIXED per-derivative widths (KS order 2: [3, 5, 7],
# GodunovKS order 4: [4, 4, 6, 8]): the narrower stencils sit in the common window at
# width // 2 - len // 2, for even and for odd widths; test_width_table pins that.
WIDTH_CASES = [
    ('BurgersEquation', 1, 3), ('BurgersEquation', 2, 5), ('BurgersEquation', 4, 7),
    ('ConservativeBurgersEquation', 1, 2), ('ConservativeBurgersEquation', 2, 4),
    ('ConservativeBurgersEquation', 4, 6), ('ConservativeBurgersEquation', 6, 8),
    ('GodunovBurgersEquation', 1, 2), ('GodunovBurgersEquation', 2, 4),
    ('GodunovBurgersEquation', 4, 6), ('GodunovBurgersEquation', 6, 8),
    ('KdVEquation', 1, 5), ('KdVEquation', 3, 7),
    ('ConservativeKdVEquation', 1, 4), ('ConservativeKdVEquation', 3, 6),
    ('ConservativeKdVEquation', 5, 8),
    ('GodunovKdVEquation', 1, 4), ('GodunovKdVEquation', 3, 6), ('GodunovKdVEquation', 5, 8),
    ('KSEquation', 1, 5), ('KSEquation', 2, 7),
    ('ConservativeKSEquation', 1, 4), ('ConservativeKSEquation', 2, 6),
    ('ConservativeKSEquation', 4, 8),
    ('GodunovKSEquation', 1, 4), ('GodunovKSEquation', 2, 6), ('GodunovKSEquation', 4, 8),
]
# the equal-width order of the same G next to a mixed one, where there is one: the same
# kernels with every column of every derivative in use
EQUAL_WIDTH_CASES = [
    ('BurgersEquation', 3, 5), ('BurgersEquation', 5, 7),
    ('ConservativeBurgersEquation', 3, 4), ('ConservativeBurgersEquation', 5, 6),
    ('GodunovBurgersEquation', 3, 4), ('GodunovBurgersEquation', 5, 6),
]
WIDE_CASES = [('KdVEquation', 5, 9), ('KSEquation', 4, 9), ('ConservativeKSEquation', 6, 10),
              ('KSEquation', 6, 11)]


def test_width_table():
  """The (order -> G) table above is what polynomials.regular_grid gives, every G of 2 .. 8 is
  there for every equation that reaches it, and every case wider than 3 points whose order is
  the lowest one mixes per-derivative widths (so the centring offset is under test)."""
  for cls_name, order, width in WIDTH_CASES + EQUAL_WIDTH_CASES + WIDE_CASES:
    eq, model, spec = _baseline(cls_name, 64, order)
    assert model.stencil_size == max(_widths(spec)) == width, (cls_name, order, _widths(spec))
  for cls_name, order, width in WIDTH_CASES:
    eq, model, spec = _baseline(cls_name, 64, order)
    if width > 3:
      assert len(set(_widths(spec))) > 1, (cls_name, order, _widths(spec))
    lower = [max(_widths(baseline_spec(eq, o))) for o in range(1, order)]
    assert width not in lower, (cls_name, order, lower)
  for cls_name, order, width in EQUAL_WIDTH_CASES:
    assert len(set(_widths(_baseline(cls_name, 64, order)[2]))) == 1
  reached = {(c, w) for c, _, w in WIDTH_CASES}
  for cls_name in {c for c, _, _ in WIDTH_CASES}:
    eq = getattr(equations, cls_name)(64)
    for order in range(1, 7):
      width = max(_widths(baseline_spec(eq, order)))
      assert width > 8 or (cls_name, width) in reached, (cls_name, order, width)


@pytest.mark.parametrize('cls_name,order,width', WIDTH_CASES + EQUAL_WIDTH_CASES)
def test_every_stencil_width_on_the_fixed_stencil_kernels(cls_name, order, width):
  """N = 64, 37 samples: a ragged last block in both streaming kernels (16 samples per tile)
  and a ragged last wavefront on the lean kernel."""
  _check_parity(cls_name, 64, order, 37)


@pytest.mark.parametrize('cls_name,order,width', WIDE_CASES)
def test_stencils_wider_than_the_streaming_kernels_carry(cls_name, order, width):
  _check_parity(cls_name, 64, order, 37, names=None)


# ---- 2. the tile walk of fixed_step_kernel --------------------------------------------------
def _walk_sizes(n):
  """(grid, samples per tile, tiles, batch): tiles = 2 grid + 2 with a ragged last tile, where
  grid = 2 blocks per SIMD, 4 SIMDs per compute unit, is the fused-step kernel's grid."""
  import torch
  grid = 2 * 4 * torch.cuda.get_device_properties(0).multi_processor_count
  per_tile = 1024 // n            # stream::kStepTile = 1024 grid points
  tiles = 2 * grid + 2
  batch = (tiles - 1) * per_tile + per_tile // 2 + 1
  return grid, per_tile, tiles, batch


@pytest.mark.parametrize('cls_name,order,n,scheme', [
    ('ConservativeKdVEquation', 3, 64, 'rk4'),     # G = 6; 16 samples per tile
    ('KSEquation', 1, 100, 'midpoint'),            # 10 samples = 1000 points per tile
])
def test_fixed_step_kernel_tile_walk(cls_name, order, n, scheme):
  """per_step (persistent blocks walking over tiles `grid` apart, the next tile prefetched)
  equals per_substep (one block per tile, no walk) on the whole array; rows of the first
  tile of every trip and of the ragged last tile match the oracle; guard rows around the
  output stay untouched."""
  import torch
  eq, model, spec = _baseline(cls_name, n, order)
  grid, per_tile, tiles, batch = _walk_sizes(n)
  assert 0 < batch - (tiles - 1) * per_tile < per_tile and tiles > 2 * grid
  # 251 distinct rows (a prime: no period of the layout divides a tile or the grid), every
  # copy scaled by its own 1 + copy / 4096: the tiles a block visits, `grid` apart, never hold
  # the same data, so a stale or swapped tile cannot compare equal
  rows = random_phase_ic(eq, 251)
  index = np.arange(batch)
  scale = (1.0 + (index // 251) / 4096.0).astype(np.float32)
  y0 = rows[index % 251] * scale[:, None]
  for first in (0, grid, 2 * grid):
    block = y0[first * per_tile:(first + 1) * per_tile]
    for other in (0, grid, 2 * grid):
      if other != first:
        assert not np.array_equal(block, y0[other * per_tile:(other + 1) * per_tile])
  dt = eq.time_step
  guard = 2 * per_tile
  y0_dev = torch.as_tensor(y0, device='cuda')
  sentinel = 12345.0
  padded = torch.full((1, batch + 2 * guard, n), sentinel, dtype=torch.float32, device='cuda')
  view = padded[:, guard:guard + batch]     # one saved row: a contiguous [1, batch, n] view
  step = model.integrate_fixed(y0_dev, 3, dt=dt, scheme=scheme, save_every=3,
                               launch_mode='per_step', out=view)
  assert model.kernel_name == 'stream_fixed'
  assert step.data_ptr() == view.data_ptr()
  substep = model.integrate_fixed(y0_dev, 3, dt=dt, scheme=scheme, save_every=3,
                                  launch_mode='per_substep')
  assert model.kernel_name == 'stream_fixed'
  assert torch.equal(step, substep)
  assert bool((padded[:, :guard] == sentinel).all()) and bool((padded[:, guard + batch:] == sentinel).all())
  assert torch.equal(y0_dev, torch.as_tensor(y0, device='cuda'))     # the input is read only
  # first and last row of: the first tile, the first tile of the second and third trips, the
  # tile before the ragged one, the ragged last tile
  picks = []
  for tile in (0, grid, 2 * grid, tiles - 2, tiles - 1):
    lo, hi = tile * per_tile, min((tile + 1) * per_tile, batch)
    picks += [lo, hi - 1]
  picks = np.array(picks)
  label = 'tile walk {} N={} ({} tiles on {} blocks, {} samples):'.format(cls_name, n, tiles, grid, batch)
  sub = y0[picks]
  want_rhs = oracle.time_derivative(spec, 0.0, sub)
  truth = baseline_rhs_f64(spec, sub)
  print('{} float32 floor {:.2e}'.format(label, rel_err(want_rhs, truth)))
  got_rhs = model.time_derivative(sub, 0.0).cpu().numpy()
  bound = measured_bound(want_rhs, truth, TOL, label, got=got_rhs)
  want = oracle.integrate_fixed(spec, SCHEMES[scheme], 0.0, dt, 3, 3, sub)
  assert np.isfinite(want).all()
  err = rel_err(step[:, torch.as_tensor(picks, device='cuda')].cpu().numpy(), want)
  assert err < bound, '{} {:.2e} from the oracle, bound {:.2e}'.format(label, err, bound)


# ---- 3. grid-size edges of the streaming kernels -------------------------------------------
G7_G8 = [(c, o) for c, o, w in WIDTH_CASES if w in (7, 8)]
EDGE_CASES = (
    # G = 8 = N: the stencil covers the whole periodic grid (and the lean kernel's G <= N edge)
    [('ConservativeKdVEquation', 5, 8, 300, 1.0)] +
    # N % 8 != 0: one float4 row per thread in the substep kernel; N = 100: 10 samples per tile
    [(c, o, n, b, 1.0) for n, b in ((12, 100), (20, 60), (100, 23)) for c, o in G7_G8] +
    # three samples per substep block and one per step tile; four idle points per tile; a full
    # tile.  dt = 0.01 x time_step: at time_step the float32 oracle itself is unstable on these
    # grids for Burgers, and KS floors there are above FLOOR_CEILING (no KS here)
    [(c, o, n, b, 0.01) for n, b in ((520, 5), (1020, 3), (1024, 3))
     for c, o in (('KdVEquation', 1), ('ConservativeKdVEquation', 1), ('BurgersEquation', 3))])


@pytest.mark.parametrize('cls_name,order,n,batch,dt_scale', EDGE_CASES)
def test_streaming_kernels_at_the_grid_size_edges(cls_name, order, n, batch, dt_scale):
  _check_parity(cls_name, n, order, batch, dt_scale=dt_scale, persistent=n <= 256)


# ---- 4. NaN masks on every baseline route --------------------------------------------------
def _nan_state(eq, n, batch=5):
  y0 = random_phase_ic(eq, batch)
  y0[2, 10] = np.nan
  y0[4, n - 1] = np.nan          # reach wraps around the periodic boundary
  y0[4, 3] = np.nan
  return y0


def _oracle_derivs(spec, y):
  derivs = oracle.baseline_space_derivatives(y, spec)
  if spec.get('weno'):
    y32 = np.asarray(y, np.float32)
    derivs[..., 0] = np.roll(oracle.weno_reconstruct_left(y32), 1, axis=-1)
    derivs[..., 1] = np.roll(oracle.weno_reconstruct_right(y32), 1, axis=-1)
  return derivs


def _check_nan_route(model, spec, eq, n, modes, names, forcing=None, views=True, label=''):
  """np.isnan(device) == np.isnan(oracle) for one evaluation, its derivative view and three
  midpoint steps in every launch mode of `modes` (asserted equal to each other, NaNs
  included); names[entry]: the kernel each entry must have run.  Finite entries -- those of
  the NaN-bearing samples too -- at the usual bound."""
  t = 0.1
  y0 = _nan_state(eq, n)
  model.set_forcing(forcing)
  got = model.time_derivative(y0, t).cpu().numpy()
  assert model.kernel_name == names['time_derivative'], (label, model.kernel_name)
  want = oracle.time_derivative(spec, t, y0, forcing)
  mask = np.isnan(want)
  assert mask[2].any() and mask[4].any() and not mask[[0, 1, 3]].any()
  np.testing.assert_array_equal(np.isnan(got), mask, err_msg=label + ' time_derivative')
  truth = baseline_rhs_f64(spec, y0, t, forcing)
  np.testing.assert_array_equal(np.isnan(truth), mask)
  ok = ~mask
  print('{} float32 floor {:.2e}'.format(label, rel_err(want[ok], truth[ok])))
  bound = measured_bound(want[ok], truth[ok], TOL, label, got=got[ok])
  assert rel_err(got[ok], want[ok]) < bound, (label, rel_err(got[ok], want[ok]), bound)
  for row in (2, 4):   # the finite entries of a NaN-bearing sample, on its own scale
    assert rel_err(got[row][ok[row]], want[row][ok[row]]) < bound, (label, row)
  if views:
    derivs = model.space_derivatives(y0).cpu().numpy()
    want_derivs = _oracle_derivs(spec, y0)
    np.testing.assert_array_equal(np.isnan(derivs), np.isnan(want_derivs),
                                  err_msg=label + ' space_derivatives')
  dt = eq.time_step
  want = oracle.integrate_fixed(spec, oracle.SCHEME_MIDPOINT, 0.0, dt, 3, 1, y0, forcing=forcing)
  mask = np.isnan(want)
  assert not mask[:, [0, 1, 3]].any() and not mask[:, [2, 4]].all()
  first = None
  for mode in modes:
    got = model.integrate_fixed(y0, 3, dt=dt, scheme='midpoint', launch_mode=mode).cpu().numpy()
    assert model.kernel_name == names[mode], (label, mode, model.kernel_name)
    np.testing.assert_array_equal(np.isnan(got), mask, err_msg='{} {}'.format(label, mode))
    assert rel_err(got[~mask], want[~mask]) < bound, (label, mode)
    if first is None:
      first = got
    else:
      np.testing.assert_array_equal(got, first, err_msg='{} {} vs {}'.format(label, mode, modes[0]))


@pytest.mark.parametrize('cls_name,order', [('KdVEquation', 1), ('ConservativeKdVEquation', 3)])
def test_nan_mask_on_the_streaming_and_lean_kernels(cls_name, order):
  """KdV order 1: G = 5, widths [3, 5]; ConservativeKdV order 3: G = 6, widths [4, 6].  The
  zero-padded columns g >= G of the 8-column table must not be multiplied into the sum
  (0 x NaN = NaN would widen the mask of the substep kernel alone)."""
  eq, model, spec = _baseline(cls_name, 64, order)
  names = {'time_derivative': 'stream_fixed', 'per_substep': 'stream_fixed',
           'per_step': 'stream_fixed', 'persistent': 'valu_f32_lean'}
  _check_nan_route(model, spec, eq, 64, ('per_substep', 'per_step', 'persistent'), names,
                   views=False, label='{} order {}:'.format(cls_name, order))


@pytest.mark.parametrize('kind,n,name', [('mfma64', 64, 'mfma_f32_r64'),
                                         ('mfma256', 128, 'mfma_f32_r256'),
                                         ('generic', 64, 'generic')])
def test_nan_mask_of_a_forced_burgers_baseline(kind, n, name):
  """Burgers at order 3 (G = 5, both stencils 5 points) with per-sample forcing: the
  tower-skipped MFMA path in both geometries, and the generic kernel."""
  eq, model, spec = _baseline('BurgersEquation', n, 3)
  model.set_kernel(kind)
  names = dict.fromkeys(('time_derivative', 'per_substep', 'per_step', 'persistent'), name)
  _check_nan_route(model, spec, eq, n, ('persistent', 'per_substep', 'per_step'), names,
                   forcing=batch_forcing(5), label='forced Burgers baseline on {}:'.format(kind))


@pytest.mark.parametrize('cls_name,order', [('KdVEquation', 1), ('ConservativeKdVEquation', 3),
                                            ('GodunovKSEquation', 2)])
def test_nan_mask_of_mixed_width_stencils_on_the_generic_kernel(cls_name, order):
  """The widest stencil's window contains the narrower ones, so the right-hand side's mask
  equals the reference's.  (Not the derivative VIEW of a narrower stencil: the [D][G] table
  of ddd_baseline_create pads it with zeros inside the common window, DESIGN.md section 5,
  test_gpu_rhs.py::test_nan_mask_of_fixed_stencil_models.)"""
  eq, model, spec = _baseline(cls_name, 64, order)
  model.set_kernel('generic')
  names = dict.fromkeys(('time_derivative', 'per_substep', 'persistent'), 'generic')
  _check_nan_route(model, spec, eq, 64, ('persistent', 'per_substep'), names, views=False,
                   label='{} order {} on the generic kernel:'.format(cls_name, order))


WENO_NAN_CASES = [('GodunovBurgersEquation', 64, False), ('GodunovBurgersEquation', 64, True),
                  ('GodunovBurgersEquation', 128, False), ('GodunovBurgersEquation', 128, True),
                  ('GodunovKdVEquation', 64, False)]


@pytest.mark.parametrize('kind,name', [('auto', 'valu_f32_weno'), ('generic', 'generic')])
@pytest.mark.parametrize('cls_name,n,forced', WENO_NAN_CASES)
def test_nan_mask_of_the_weno_solver(cls_name, n, forced, kind, name):
  """u_minus reaches x - 3 .. x + 1, u_plus x - 2 .. x + 2: the Godunov flux is NaN where
  EITHER is (np.minimum / np.maximum), not where the selected branch's operand is."""
  eq, model, spec = _baseline(cls_name, n, 3, weno=True)
  if kind != 'auto':
    model.set_kernel(kind)
  names = dict.fromkeys(('time_derivative', 'per_substep', 'persistent'), name)
  _check_nan_route(model, spec, eq, n, ('persistent', 'per_substep'), names,
                   forcing=batch_forcing(5) if forced else None,
                   label='{} N={} WENO{} on {}:'.format(cls_name, n, ', forced' if forced else '', name))


def test_nan_samples_fail_the_adaptive_weno_solver_next_to_healthy_ones():
  eq, model, spec = _baseline('GodunovBurgersEquation', 64, 3, weno=True)
  y0 = _nan_state(eq, 64).astype(np.float64)
  times = np.linspace(0.0, 0.02, 3)
  y, nfev, status = model.integrate_adaptive(y0, times)
  assert model.kernel_name == 'valu_f32_weno'
  y, status = y.cpu().numpy(), status.cpu().numpy()
  np.testing.assert_array_equal(status, [0, 0, -1, 0, -1])
  assert np.isnan(y[1:, [2, 4]]).all()
  assert np.isfinite(y[:, [0, 1, 3]]).all()


# ---- 5. in-place substeps ------------------------------------------------------------------
def _stream_model():
  eq, model, _ = _baseline('ConservativeKdVEquation', 64, 1)
  return model


def _learned(n, kind='auto', **overrides):
  model = make_model('burgers', True, num_points=n, resample_factor=2, **overrides)
  if kind != 'auto':
    model.set_kernel(kind)
  model.set_forcing(batch_forcing(37))
  return model


INPLACE_ROUTES = {
    'stream_fixed': _stream_model,
    'mfma_f32_r64': lambda: _learned(64),
    'mfma_f32_r256': lambda: _learned(128),
    'valu_f32_weno': lambda: _baseline('GodunovBurgersEquation', 64, 3, weno=True)[1],
    'generic': lambda: _learned(64, 'generic'),
    'spectral_f64': lambda: model_lib.SpectralModel(equations.KdVEquation(64, random_seed=3)),
}


@pytest.mark.parametrize('name', sorted(INPLACE_ROUTES))
def test_rk_substep_in_place(name):
  """include/ddd1d.h: "y_out / acc_out may alias their inputs".  (a) y_out is y_base (not
  y_in) and acc_out is acc_in, one call; (b) the in-place Euler step y_in is y_base is y_out.
  Each equals the same call with separate output arrays, bit for bit."""
  import torch
  model = INPLACE_ROUTES[name]()
  batch = 37
  dtype = torch.float64 if name == 'spectral_f64' else torch.float32
  dev = lambda seed0: torch.as_tensor(random_phase_ic(model.equation, batch, seed0=seed0),
                                      device='cuda').to(dtype)
  y, base, acc = dev(1000), dev(2000), dev(3000)
  c1, c2, t = 0.25 * model.equation.time_step, -0.5 * model.equation.time_step, 0.3
  # separate outputs
  out_y, out_acc = torch.empty_like(y), torch.empty_like(y)
  model.rk_substep(t, y, y_base=base, c1=c1, y_out=out_y, acc_in=acc, c2=c2, acc_out=out_acc)
  assert model.kernel_name == name
  assert bool(torch.isfinite(out_y).all()) and bool(torch.isfinite(out_acc).all())
  assert not torch.equal(out_y, base) and not torch.equal(out_acc, acc)
  # (a)
  base_a, acc_a, y_a = base.clone(), acc.clone(), y.clone()
  model.rk_substep(t, y_a, y_base=base_a, c1=c1, y_out=base_a, acc_in=acc_a, c2=c2, acc_out=acc_a)
  assert model.kernel_name == name
  assert torch.equal(base_a, out_y) and torch.equal(acc_a, out_acc) and torch.equal(y_a, y)
  # (b)
  euler = torch.empty_like(y)
  model.rk_substep(t, y, y_base=y, c1=c1, y_out=euler)
  y_b = y.clone()
  model.rk_substep(t, y_b, y_base=y_b, c1=c1, y_out=y_b)
  assert model.kernel_name == name
  assert torch.equal(y_b, euler) and not torch.equal(euler, y)
