"""Forcing tables, GPU tier: every kernel that implements the time-dependent forcing, at every
table shape it branches on (tests/forcing_cases.py; DESIGN 5, "Forcing tables").

a. Forcing in isolation: at the zero state the stencils give exactly 0, so the right-hand side
   IS the forcing; |device - oracle.forcing_f64| <= forcing_cases.bound per sample, for every
   shape, t in {0, 3.3, 47} and route, through the substep kernels (time_derivative) and the
   persistent integrators (one Euler step of dt = 1 from t: y1 = 0 + 1 f, exactly).
b. Every launch shape sees the same tables: persistent == per_step == per_substep bit for bit,
   float64 state within 1e-6, rows against oracle.integrate_fixed at 1e-5.
c. Per-sample times in one group: the adaptive integrator, solo and as a population.
d. Table lifetime: replacing, clearing, prefixes, refusal."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import forcing_cases as fc
from helpers import make_model, oracle, random_phase_ic, rel_err
from ddd1d_amd import _lib, equations, model as model_lib

pytestmark = pytest.mark.gpu

R64, R256, W32, W16, H16 = ('mfma_f32_r64', 'mfma_f32_r256', 'mfma_f32_r64w32',
                            'mfma_f32_r64w16', 'mfma_f32_r64h16')
LEAN, WENO, GENERIC = 'valu_f32_lean', 'valu_f32_weno', 'generic'
# groups beyond which the automatic choice is the one-wavefront kernel on every MI355X
# (capi.hip plan_mfma: 2 groups > SIMDs, 1024 of them)
ONE_WAVE_GROUPS = 514


def _spg(num_points, rows):
  return rows // num_points


def _rows(num_points, kind=None):
  return 256 if kind == 'mfma256' or num_points > 64 or 64 % num_points else 64


@functools.lru_cache(maxsize=None)
def _case(name, batch, num_points, resample_factor, conservative, period):
  """(forcing, {t: (float64 truth [batch, N], bound [batch])}), computed once per case."""
  forcing = fc.draw(name, batch, num_points)
  per_time = {}
  for t in fc.TIMES:
    per_time[t] = (oracle.forcing_f64(t, forcing, num_points, resample_factor, period,
                                      conservative), fc.bound(forcing, t))
  return forcing, per_time


def _device_forcing(model, batch, t, entry):
  zeros = torch.zeros((batch, model.num_points), dtype=torch.float32, device='cuda')
  if entry == 'substep':
    return model.time_derivative(zeros, t).cpu().numpy()
  return model.integrate_fixed(zeros, 1, dt=1.0, t0=t, scheme='euler')[0].cpu().numpy()


def _check_route(label, model, batch, expected_name, entries=('substep', 'persistent'),
                 kind=None, shapes=None):
  """Every shape of the model's grid x every time x the entries: inside the bound, and on the
  kernel expected_name(forcing, entry) says (None: not pinned)."""
  grid = model.equation.grid
  n, rf = grid.solution_num_points, grid.resample_factor
  conservative = bool(model.equation.CONSERVATIVE)
  worst, worst_at, wrong = 0.0, None, []
  if kind is not None:
    model.set_kernel(kind)
  for name in (shapes or fc.shapes_for(n)):
    forcing, per_time = _case(name, batch, n, rf, conservative, float(grid.period))
    model.set_forcing(forcing)
    for entry in entries:
      for t in fc.TIMES:
        got = _device_forcing(model, batch, t, entry)
        want_name = expected_name(forcing, entry)
        if want_name is not None and model.kernel_name != want_name:
          wrong.append((name, entry, model.kernel_name, want_name))
        truth, limit = per_time[t]
        assert np.isfinite(got).all(), (label, name, entry, t)
        ratio = (np.abs(got.astype(np.float64) - truth).max(axis=1) / limit)
        if ratio.max() > worst:
          worst, worst_at = ratio.max(), (name, entry, t, int(ratio.argmax()))
        assert (ratio <= 1.0).all(), (
            '{}: shape {} via {} at t = {}: |device - float64| / B per sample = {}'.format(
                label, name, entry, t, np.round(ratio, 3)))
  print('forcing route {}: worst measured / B = {:.3f} at {}'.format(label, worst, worst_at))
  assert not wrong, wrong


# ---------------------------------------------------------------------------
# a. forcing in isolation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('conservative', [True, False])
@pytest.mark.parametrize('num_points,resample_factor', [(64, 4), (32, 8), (16, 1)])
@pytest.mark.parametrize('kind', ['auto', 'mfma64', 'mfma64w32', 'mfma64w16'])
def test_default_net_64_row_kernels(kind, num_points, resample_factor, conservative):
  model = make_model('burgers', conservative, num_points=num_points,
                     resample_factor=resample_factor)
  spg = _spg(num_points, 64)
  batch = (ONE_WAVE_GROUPS - 1) * spg + 1 if kind == 'auto' else 2 * spg + 1

  def expected(forcing, entry):
    if kind == 'mfma64w32':
      return W32
    if kind == 'mfma64w16' and entry == 'persistent' and fc.is_fast(forcing, num_points, 64):
      return W16   # (four-wavefront groups: per-equation integrators only)
    return R64
  _check_route('default/{}/N{}/{}'.format(kind, num_points, 'flux' if conservative else 'plain'),
               model, batch, expected, kind=kind)


@pytest.mark.parametrize('num_points,resample_factor,kind', [
    (64, 4, 'mfma256'), (128, 2, 'auto'), (96, 2, 'auto'), (256, 2, 'auto')])
def test_default_net_256_row_kernels(num_points, resample_factor, kind):
  """N = 256: one sample per group, where `P < 256` (the unsigned char runs) is the live edge."""
  model = make_model('burgers', True, num_points=num_points, resample_factor=resample_factor)
  batch = 2 * _spg(num_points, 256) + 1
  _check_route('default/{}/N{}'.format(kind, num_points), model, batch, lambda f, e: R256,
               kind=kind)


@pytest.mark.parametrize('num_points,resample_factor', [(64, 4), (32, 8)])
@pytest.mark.parametrize('kind,name', [('mfma64', R64), ('mfma64w32', W32), ('mfma256', R256)])
@pytest.mark.parametrize('overrides', [dict(num_layers=4), dict(num_layers=2),
                                       dict(nonlinearity='tanh')], ids=['L4', 'L2', 'tanh'])
def test_runtime_parameterised_nets(overrides, kind, name, num_points, resample_factor):
  """Not hoisted: for n_k <= 4 the trig table is read from the activation buffers' row padding."""
  model = make_model('burgers', True, num_points=num_points, resample_factor=resample_factor,
                     **overrides)
  batch = 2 * _spg(num_points, _rows(num_points, kind)) + 1
  _check_route('runtime/{}/{}/N{}'.format(sorted(overrides.items()), kind, num_points),
               model, batch, lambda f, e: name, kind=kind)


@pytest.mark.parametrize('num_points,resample_factor', [(64, 4), (96, 2)])
@pytest.mark.parametrize('overrides', [
    dict(kernel_size=7), dict(filter_size=64), dict(kernel_size=7, filter_size=64),
    dict(kernel_size=3)], ids=['k7', 'c64', 'k7c64', 'k3'])
def test_streamed_towers(overrides, num_points, resample_factor):
  model = make_model('burgers', True, num_points=num_points, resample_factor=resample_factor,
                     **overrides)
  rows = _rows(num_points)
  _check_route('tower/{}/N{}'.format(sorted(overrides.items()), num_points), model,
               2 * _spg(num_points, rows) + 1, lambda f, e: R64 if rows == 64 else R256)


@pytest.mark.parametrize('num_points,resample_factor,conservative', [(64, 4, True), (32, 8, False)])
def test_wide_flavour(num_points, resample_factor, conservative):
  model = make_model('burgers', conservative, num_points=num_points,
                     resample_factor=resample_factor, coefficient_grid_min_size=9)
  _check_route('wide/N{}'.format(num_points), model, 2 * _spg(num_points, 64) + 1,
               lambda f, e: R64)


@pytest.mark.parametrize('num_points,resample_factor,conservative', [(64, 4, True), (32, 8, False)])
def test_sixteen_channel_tiles(num_points, resample_factor, conservative):
  model = make_model('burgers', conservative, num_points=num_points,
                     resample_factor=resample_factor, filter_size=16)
  # (per-equation kernels only: other tables run the run-time-parameterised one-wave kernel)
  _check_route('h16/N{}'.format(num_points), model, 2 * _spg(num_points, 64) + 1,
               lambda f, e: H16 if fc.is_fast(f, num_points, 64) else R64, kind='mfma64')


def _fixed_models(num_points, resample_factor, conservative):
  cls = equations.ConservativeBurgersEquation if conservative else equations.BurgersEquation
  return {
      'one_layer': lambda: make_model('burgers', conservative, num_points=num_points,
                                      resample_factor=resample_factor, num_layers=1),
      'baseline': lambda: model_lib.BaselineModel(cls(num_points, resample_factor),
                                                  accuracy_order=3),
  }


@pytest.mark.parametrize('num_points,resample_factor,conservative', [(64, 4, True), (32, 8, False)])
@pytest.mark.parametrize('which', ['one_layer', 'baseline'])
@pytest.mark.parametrize('kind', ['auto', 'mfma64', 'mfma256'])
def test_fixed_stencils_and_one_layer_nets(kind, which, num_points, resample_factor,
                                           conservative):
  """The lean kernel where rhs_lean.h supports() holds (persistent, automatic choice), else and
  under an explicit kind the MFMA-path kernels with the tower skipped."""
  model = _fixed_models(num_points, resample_factor, conservative)[which]()
  rows = _rows(num_points, kind)

  def expected(forcing, entry):
    if kind == 'auto' and entry == 'persistent' and fc.lean_supports(forcing, num_points):
      return LEAN
    return R256 if rows == 256 else R64
  _check_route('{}/{}/N{}'.format(which, kind, num_points), model,
               2 * _spg(num_points, rows) + 1, expected, kind=kind)


def test_weno_kernels_and_their_generic_fallback():
  model = model_lib.BaselineModel(equations.GodunovBurgersEquation(128, 2), 3, weno=True)
  _check_route('weno/N128', model, 5,
               lambda f, e: WENO if fc.weno_supports(f) else GENERIC,
               shapes=fc.shapes_for(128) + ('p64', 'p65'))


@pytest.mark.parametrize('num_points,resample_factor,conservative', [
    (64, 4, True), (32, 8, False), (128, 2, True), (16, 1, False)])
def test_generic_kernel(num_points, resample_factor, conservative):
  model = make_model('burgers', conservative, num_points=num_points,
                     resample_factor=resample_factor)
  _check_route('generic/N{}'.format(num_points), model, 5, lambda f, e: GENERIC, kind='generic')


# ---------------------------------------------------------------------------
# b. every launch shape sees the same tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('num_points,resample_factor', [(64, 4), (32, 8)])
@pytest.mark.parametrize('overrides', [dict(), dict(num_layers=4), dict(kernel_size=7)],
                         ids=['default', 'L4', 'k7'])
def test_launch_modes_agree(overrides, num_points, resample_factor):
  """The pipelined prepare_next sums of the persistent kernels, the step kernels and
  substep_multi_kernel's per-group fetch_samples all compute the same forcing."""
  model = make_model('burgers', True, num_points=num_points, resample_factor=resample_factor,
                     **overrides)
  spg = _spg(num_points, 64)
  batch = 2 * spg + 1
  y0 = random_phase_ic(model.equation, batch)
  rows = sorted({0, spg, batch - 1})
  dt = 1e-3
  for name in ('one', 'four', 'five', 'eight', 'run20', 'edge', 'over'):
    forcing = fc.draw(name, batch, num_points)
    model.set_forcing(forcing)
    some = {k: v[rows] for k, v in forcing.items()}
    for scheme, steps, oracle_scheme in (('midpoint', 12, oracle.SCHEME_MIDPOINT),
                                         ('rk4', 5, oracle.SCHEME_RK4)):
      run = lambda **kw: model.integrate_fixed(y0, steps, dt=dt, scheme=scheme, save_every=steps,
                                               **kw).cpu().numpy()
      persistent = run()
      np.testing.assert_array_equal(persistent, run(launch_mode='per_step'), err_msg=name)
      np.testing.assert_array_equal(persistent, run(launch_mode='per_substep'), err_msg=name)
      wide = run(state_dtype='float64')
      assert rel_err(wide, persistent) < 1e-6, (name, scheme, rel_err(wide, persistent))
      want = oracle.integrate_fixed(model.spec(), oracle_scheme, 0.0, dt, steps, steps, y0[rows],
                                    forcing=some)
      err = rel_err(persistent[:, rows], want)
      assert err < 1e-5, (name, scheme, err)


def test_sample_slabs_shift_the_tables():
  """An ensemble of twice the machine's resident groups is advanced, in the per-substep mode,
  as two sample slabs side by side (capi.hip plan_slabs): launch_params moves `frc` and `runs`
  to each slab's first sample.  4097 groups of four N = 16 samples; the forcing in isolation
  through that path, and the slabs against the one persistent launch."""
  num_points, groups = 16, 4097   # (>= 2 x 2 wavefronts x 1024 SIMDs)
  model = make_model('burgers', False, num_points=num_points, resample_factor=1)
  batch = (groups - 1) * _spg(num_points, 64) + 1
  zeros = torch.zeros((batch, num_points), dtype=torch.float32, device='cuda')
  t = 3.3
  for name in ('two7', 'edge'):
    forcing = fc.draw(name, batch, num_points)
    assert fc.is_fast(forcing, num_points, 64)   # (else: no per-equation kernel, no slabs)
    model.set_forcing(forcing)
    run = lambda **kw: model.integrate_fixed(zeros, 1, dt=1.0, t0=t, scheme='euler',
                                             **kw)[0].cpu().numpy()
    slabs = run(launch_mode='per_substep')
    assert model.kernel_name == R64
    truth = oracle.forcing_f64(t, forcing, num_points, 1, float(model.equation.grid.period), False)
    ratio = np.abs(slabs.astype(np.float64) - truth).max(axis=1) / fc.bound(forcing, t)
    print('forcing route slabs/N16 {}: worst measured / B = {:.3f}'.format(name, ratio.max()))
    assert (ratio <= 1.0).all(), (name, int(ratio.argmax()), ratio.max())
    np.testing.assert_array_equal(slabs, run())


# ---------------------------------------------------------------------------
# c. per-sample times in one group
# ---------------------------------------------------------------------------
ADAPTIVE_TIMES = np.array([0.0, 0.013, 0.1, 0.2])


def _population_adaptive(models, y0, times):
  """ddd_population_integrate_adaptive_f64 (the population form, replicas on grid.y)."""
  lib = _lib.load_library()
  handles = (ctypes.c_void_p * len(models))(*[m._handle.value for m in models])
  handle = ctypes.c_void_p()
  assert lib.ddd_population_create(handles, len(models), ctypes.byref(handle)) == 0, (
      lib.ddd_last_error().decode())
  y0 = torch.from_numpy(np.ascontiguousarray(y0, dtype=np.float64)).cuda()
  times = np.ascontiguousarray(times, dtype=np.float64)
  y = torch.full((len(models), times.size) + tuple(y0.shape), 7.0, dtype=torch.float64,
                 device='cuda')
  nfev = torch.zeros((len(models), y0.shape[0]), dtype=torch.int32, device='cuda')
  status = torch.zeros_like(nfev)
  try:
    _lib.check(lib.ddd_population_integrate_adaptive_f64(
        handle, times.ctypes.data_as(_lib._D), times.size, 1e-3, 1e-6, 0.01, 0,
        y0.data_ptr(), y.data_ptr(), nfev.data_ptr(), status.data_ptr(), y0.shape[0],
        _lib.current_stream()))
    torch.cuda.synchronize()
  finally:
    assert lib.ddd_population_destroy(handle) == 0
  return y.cpu().numpy(), nfev.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('num_points,resample_factor,shape', [(16, 4, 'two7'), (32, 4, 'four')])
def test_adaptive_controllers_share_a_group(num_points, resample_factor, shape):
  """Four (two) samples per wavefront, each with its own controller and its own t: the forcing
  sums of a group are computed for as many times as it has samples."""
  models = [make_model('burgers', True, num_points=num_points, resample_factor=resample_factor,
                       init_seed=seed) for seed in range(2)]
  batch = 2 * _spg(num_points, 64) + 1
  forcing = fc.draw(shape, batch, num_points)
  y0 = (0.3 * random_phase_ic(models[0].equation, batch)).astype(np.float64)
  solo = []
  for model in models:
    model.set_forcing(forcing)
    y, nfev, status = model.integrate_adaptive(y0, ADAPTIVE_TIMES, max_step=0.01)
    solo.append((y.cpu().numpy(), nfev.cpu().numpy(), status.cpu().numpy()))
  y, nfev, status = solo[0]
  assert (status == 0).all()
  spec = models[0].spec()
  for b in range(batch):
    want, want_nfev = oracle.odeint_rk23(spec, y0[b], ADAPTIVE_TIMES,
                                         {k: v[b] for k, v in forcing.items()})
    assert want_nfev == nfev[b], (b, int(nfev[b]), want_nfev)
    err = rel_err(y[:, b], want)
    assert err < 1e-5, (b, err)
  got = _population_adaptive(models, y0, ADAPTIVE_TIMES)
  for r in range(2):
    for have, want in zip(got, solo[r]):
      np.testing.assert_array_equal(have[r], want, err_msg='replica {}'.format(r))


# ---------------------------------------------------------------------------
# d. table lifetime
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('overrides', [dict(), dict(num_layers=4)], ids=['default', 'L4'])
def test_table_lifetime(overrides):
  build = lambda: make_model('burgers', True, num_points=32, resample_factor=8, **overrides)
  model = build()
  batch = 9
  y0 = random_phase_ic(model.equation, batch)
  run = lambda m, y: m.integrate_fixed(y, 6, dt=1e-3, save_every=3).cpu().numpy()
  table_a, table_b = fc.draw('six', batch, 32), fc.draw('two', batch, 32)
  model.set_forcing(table_a)
  first = run(model, y0)
  model.set_forcing(table_b)   # another P and n_k, over the first
  second = run(model, y0)
  fresh = build()
  fresh.set_forcing(table_b)
  np.testing.assert_array_equal(second, run(fresh, y0))
  assert not np.array_equal(first, second)
  # a prefix of the samples the tables were set for: the same rows
  np.testing.assert_array_equal(run(model, y0[:5]), second[:, :5])
  want = oracle.integrate_fixed(model.spec(), oracle.SCHEME_MIDPOINT, 0.0, 1e-3, 6, 3, y0[:5],
                                forcing={k: v[:5] for k, v in table_b.items()})
  assert rel_err(second[:, :5], want) < 1e-5
  # tables for fewer samples than the batch are refused
  model.set_forcing({k: v[:5] for k, v in table_b.items()})
  with pytest.raises(Exception, match='exceeds'):
    run(model, y0)
  # cleared: the unforced model
  model.set_forcing(None)
  unforced = build()
  np.testing.assert_array_equal(run(model, y0), run(unforced, y0))
  assert not np.array_equal(run(model, y0), second)
