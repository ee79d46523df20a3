"""Float64-state fixed-step integrators (ddd_integrate_fixed_f64) against ONE step of host
float64 arithmetic over the device's own right-hand side, on every kernel family
launch_integrate<double> reaches.

The reference (part 1).  The device runs n steps with save_every=1; with y0 prepended that is
Y[0..n] in the device's bits.  Y[k+1] is then predicted from Y[k] on the host in NumPy float64,
by the statement of rhs_mfma.h integrate_kernel, rhs_generic.h integrate_kernel and
oracle.integrate_fixed,

    t = t0 + k dt ; ynew = y
    us = y                                              (s = 0)
    us = y + float64(f_prev) * (float64(float32(a[s])) * dt)
    f  = model.time_derivative(float32(us), t + c[s] dt)        (the device, float32)
    if b[s] != 0: ynew = ynew + (float64(float32(b[s])) * dt) * float64(f)

and for SpectralModel with the exact double b weights (capi.hip: tableau_weights_f64) and the
float64 time_derivative.  Every step starts from the device's own bits, so nothing accumulates:
host and kernel can differ only where a compiler contracts y + c f into an fma, at most one
float64 ulp of the state per operation, at most 2 x stages <= 8 operations per step.  The bound
is therefore derived, not measured: |got - want| <= 16 x 2.2e-16 x max|Y[k]| (per sample).

A one-ulp difference in a stage input moves float32(us) only when us sits within a few float64
ulps of a float32 rounding boundary (about 2^-27 of the elements).  Such (sample, step) pairs
are found on the host, printed and left out of that step's comparison; at most one per case.

The test proves its own power (part 2): on every BS3 and RK4 case two wrong references -- the
other b-weight convention (exact doubles where the contract rounds through float32, and the
reverse for spectral), and a state rounded through float32 after the step -- must each lie more
than 100 x the bound from the device on at least one step, and every step must move the state
by at least 2e-5 of max|y|, so that no case can go blind unnoticed.  Time steps: Burgers 1e-3,
KdV and KS 10 x equation.time_step (increments 2e-3, 5e-4, 5e-5 of max|y| under
oracle.integrate_fixed in float64; stable over 6 steps).

Part 4 keeps the oracle in the loop: the first three samples of one BS3 run per route against
oracle.integrate_fixed(state_dtype=float64) at the project's 1e-5.

Premise: the in-kernel right-hand side has the bits of ddd_time_derivative on (float)us,
(float)t (for float32 state the launch-mode tests pin this bit for bit).  A route that broke it
would miss the bound by a float32 ulp of f, eight orders of magnitude.

Measured on one MI355X: 146 tests, 3.6 s for the module run alone (2.2 s of it the first test,
which loads the library; every other test under 0.05 s, the first spectral one 0.3 s).  Largest
error per route, in units of 2.2e-16 max|y|: 0.00 on every one of them -- per-equation r64,
per-equation r256, half tile, streamed towers, wide, run-time kernel and its two-wavefront
split, generic, fixed stencils, WENO, spectral: the library is built without fma contraction,
so the kernels' float64 updates have the host's bits.  No (sample, step) pair was left out.
Nearest wrong reference: the other b weights at 2.56e3 of that unit (fixed stencils, KS
N = 100, BS3; the threshold is 1.6e3), the float32-rounded state at 1.8e8.  BS3 against the
oracle: at most 8.8e-9 (per-equation r256 under mfma256), spectral 1.5e-16.
"""
import collections
import functools

import numpy as np
import pytest

from helpers import oracle, make_model, random_phase_ic, batch_forcing, rel_err
from ddd1d_amd import equations, model as model_lib

pytestmark = pytest.mark.gpu

EPS = 2.2e-16          # float64 ulp of 1
ULPS = 16              # 2 x (2 x stages <= 8 operations) ulps of the state per step
MUTANT = 100 * ULPS    # a wrong reference must be further than this, in the same unit
MIN_INCREMENT = 2e-5   # of max|y|, every step
TOL = 1e-5             # the project's trajectory bound against the oracle
TOL64 = 1e-9           # ... and where the right-hand side is float64 too (test_gpu_exact_solvers)

SCHEMES = {'euler': oracle.SCHEME_EULER, 'midpoint': oracle.SCHEME_MIDPOINT,
           'bs3': oracle.SCHEME_BS3, 'rk4': oracle.SCHEME_RK4}
ALL = ('euler', 'midpoint', 'bs3', 'rk4')
# the exact double b weights (capi.hip: tableau_weights_f64)
EXACT_B = {'euler': (1.0,), 'midpoint': (0.0, 1.0), 'bs3': (2.0 / 9.0, 1.0 / 3.0, 4.0 / 9.0),
           'rk4': (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)}

Case = collections.namedtuple('Case', 'route build batch steps name kernel schemes time_steps')


def _learned(equation, conservative, n, **overrides):
  return lambda: make_model(equation, conservative, num_points=n, resample_factor=2, **overrides)


def _case(route, build, batch, steps, name, kernel='auto', schemes=ALL, time_steps=10):
  """time_steps: dt of an unforced equation in units of equation.time_step."""
  return Case(route, build, batch, steps, name, kernel, schemes, time_steps)


R64, R256 = 'mfma_f32_r64', 'mfma_f32_r256'

# id -> case: the smallest shapes that take each branch.  Batches of 3 .. 9; where a group
# holds several samples the batch leaves the last group ragged.
CASES = collections.OrderedDict([
    # per-equation kernels, 64 rows: the six instantiations at N = 64 ...
    ('burgers64', _case('per-equation r64', _learned('burgers', False, 64), 4, 5, R64)),
    ('burgers_cons64', _case('per-equation r64', _learned('burgers', True, 64), 3, 6, R64)),
    ('kdv64', _case('per-equation r64', _learned('kdv', False, 64), 5, 4, R64)),
    ('kdv_cons64', _case('per-equation r64', _learned('kdv', True, 64), 3, 5, R64)),
    ('ks64', _case('per-equation r64', _learned('ks', False, 64), 4, 6, R64)),
    ('ks_cons64', _case('per-equation r64', _learned('ks', True, 64), 6, 4, R64)),
    # ... and 2, 4, 8 samples per group, the last group ragged
    ('burgers_cons32', _case('per-equation r64', _learned('burgers', True, 32), 5, 5, R64)),
    ('ks16', _case('per-equation r64', _learned('ks', False, 16), 7, 4, R64)),
    ('kdv_cons8', _case('per-equation r64', _learned('kdv', True, 8), 9, 6, R64)),
    # per-equation kernels, 256 rows: 2, 1, 2, 2 samples per group
    ('burgers_cons128', _case('per-equation r256', _learned('burgers', True, 128), 3, 5, R256)),
    ('ks_cons256', _case('per-equation r256', _learned('ks', True, 256), 3, 4, R256)),
    ('kdv96', _case('per-equation r256', _learned('kdv', False, 96), 5, 6, R256)),
    ('burgers100', _case('per-equation r256', _learned('burgers', False, 100), 7, 4, R256)),
    # the 16-channel half tile
    ('half64', _case('half tile', _learned('burgers', True, 64, filter_size=16), 4, 5,
                     'mfma_f32_r64h16')),
    ('half32', _case('half tile', _learned('kdv', True, 32, filter_size=16), 5, 4,
                     'mfma_f32_r64h16')),
    # the streamed towers
    ('taps7', _case('streamed towers', _learned('burgers', True, 64, kernel_size=7), 3, 4, R64)),
    ('filters64', _case('streamed towers', _learned('kdv', False, 64, filter_size=64), 3, 4, R64)),
    ('taps3', _case('streamed towers', _learned('ks', True, 32, kernel_size=3), 5, 5, R64)),
    # the wide flavour
    ('wide', _case('wide', _learned('ks', True, 64, coefficient_grid_min_size=9), 4, 4, R64)),
    # the run-time-parameterised kernel
    ('runtime', _case('run-time kernel', _learned('burgers', True, 64, num_layers=4,
                                                  nonlinearity='tanh'), 4, 5, R64)),
    # the default model under an explicit kernel kind (BS3 only)
    ('burgers_w32', _case('run-time kernel, two-wavefront split', _learned('burgers', True, 64),
                          4, 5, 'mfma_f32_r64w32', 'mfma64w32', ('bs3',))),
    ('kdv_w32', _case('run-time kernel, two-wavefront split', _learned('kdv', False, 64), 3, 4,
                      'mfma_f32_r64w32', 'mfma64w32', ('bs3',))),
    ('burgers_mfma256', _case('per-equation r256', _learned('burgers', True, 64), 6, 5, R256,
                              'mfma256', ('bs3',))),
    ('kdv_mfma256', _case('per-equation r256', _learned('kdv', False, 64), 5, 4, R256,
                          'mfma256', ('bs3',))),
    ('burgers_generic', _case('generic', _learned('burgers', True, 64), 4, 5, 'generic',
                              'generic', ('bs3',))),
    ('kdv_generic', _case('generic', _learned('kdv', False, 64), 3, 4, 'generic', 'generic',
                          ('bs3',))),
    # nets only the generic kernel carries
    ('taps9', _case('generic', _learned('burgers', True, 64, kernel_size=9), 3, 4, 'generic')),
    ('filters96', _case('generic', _learned('kdv', True, 48, filter_size=96), 4, 4, 'generic')),
    # fixed stencils: the MFMA-path kernels with the tower skipped
    ('fixed_kdv', _case('fixed stencils', lambda: model_lib.BaselineModel(
        equations.KdVEquation(64), accuracy_order=1), 5, 5, R64)),
    ('fixed_burgers3', _case('fixed stencils', lambda: model_lib.BaselineModel(
        equations.BurgersEquation(64), accuracy_order=3), 4, 6, R64)),
    ('fixed_ks100', _case('fixed stencils', lambda: model_lib.BaselineModel(
        equations.ConservativeKSEquation(100), accuracy_order=1), 3, 4, R256)),
    # WENO5 + Godunov flux, forced
    ('weno128', _case('WENO', lambda: model_lib.BaselineModel(
        equations.GodunovBurgersEquation(128), 3, weno=True), 5, 5, 'valu_f32_weno')),
    ('weno96', _case('generic', lambda: model_lib.BaselineModel(
        equations.GodunovBurgersEquation(96), 3, weno=True), 4, 4, 'generic')),
    # the spectral substep chain: the circulant kernel and the in-LDS FFT
    ('spectral64', _case('spectral', lambda: model_lib.SpectralModel(equations.KdVEquation(64)),
                         4, 5, 'spectral_f64')),
    # (N = 512: u_xxx is 512 x stiffer.  At 10 x time_step RK4 reaches 1e129 in four steps; at
    # 1 x the increments are 4e-5 of max|y| and four steps of every scheme stay at max|y| = 1.63)
    ('spectral512', _case('spectral', lambda: model_lib.SpectralModel(equations.KdVEquation(512)),
                          3, 4, 'spectral_f64', time_steps=1)),
])

# one BS3 run per route against the oracle (part 4)
ORACLE_CASES = ('kdv64', 'ks64', 'kdv_cons8', 'kdv96', 'half64', 'taps7', 'wide', 'runtime',
                'kdv_w32', 'burgers_mfma256', 'kdv_generic', 'filters96', 'fixed_kdv',
                'fixed_burgers3', 'fixed_ks100', 'weno128', 'weno96', 'spectral64')


def _is_spectral(model):
  return isinstance(model, model_lib.SpectralModel)


def _forced(model):
  return not _is_spectral(model) and model.equation.has_time_dependent_forcing


def _dt(case_id):
  model = _setup(case_id)[0]
  return 1e-3 if _forced(model) else CASES[case_id].time_steps * model.equation.time_step


def _t0(model):
  return 1.5 if _forced(model) else 0.0


@functools.lru_cache(maxsize=None)
def _setup(case_id):
  """(model, y0 float64 [batch, N], forcing): built once per case, never changed."""
  case = CASES[case_id]
  model = case.build()
  forcing = batch_forcing(case.batch, seed0=3) if _forced(model) else None
  if forcing is not None:
    model.set_forcing(forcing)
  if case.kernel != 'auto':
    model.set_kernel(case.kernel)
  # (scaled off the float32 grid: a state float32 cannot hold from the first load on.  With a
  # float32-exact y0 and these decimal time steps, y + f (a dt) lands on float32 rounding
  # boundaries once in about 500 elements instead of 2^-27: f (a dt) / ulp32 is then a
  # multiple of 1 / 500)
  y0 = random_phase_ic(model.equation, case.batch, seed0=1000 + len(case_id)).astype(np.float64)
  y0 = y0 * (1.0 + 1e-3 / np.pi)
  y0.setflags(write=False)
  return model, y0, forcing


def _run(case_id, y0, scheme, steps, save_every=1):
  model = _setup(case_id)[0]
  return model.integrate_fixed(y0.copy(), steps, dt=_dt(case_id), t0=_t0(model), scheme=scheme,
                               save_every=save_every, state_dtype='float64').cpu().numpy()


@functools.lru_cache(maxsize=None)
def _trajectory(case_id, scheme):
  """Y[0 .. n] in the device's own bits (y0 prepended), read-only."""
  case = CASES[case_id]
  model, y0, _ = _setup(case_id)
  got = _run(case_id, y0, scheme, case.steps)
  assert model.kernel_name == case.name, (case_id, model.kernel_name)
  assert got.dtype == np.float64 and got.shape == (case.steps,) + y0.shape
  traj = np.concatenate([y0[None], got])
  traj.setflags(write=False)
  return traj


def _rhs(model, us, t):
  """The device's right-hand side on the stage input, as float64."""
  if _is_spectral(model):
    return model.time_derivative(np.array(us), t).cpu().numpy()
  return model.time_derivative(us.astype(np.float32), t).cpu().numpy().astype(np.float64)


def _near_float32_boundary(us):
  """Elements whose float32 rounding a difference of a few float64 ulps could flip."""
  with np.errstate(invalid='ignore'):
    d = 4 * np.spacing(np.abs(us))
    return np.isfinite(us) & ((us + d).astype(np.float32) != (us - d).astype(np.float32))


def _host_step(model, scheme, y, t, dt):
  """One step from y [batch, N] (float64): (the contract's result, the other b-weight
  convention, the state rounded through float32, samples with a stage input at a float32
  rounding boundary)."""
  a, b, c = oracle.TABLEAUS[SCHEMES[scheme]]
  spectral = _is_spectral(model)
  rounded_b = [np.float64(np.float32(v)) for v in b]
  exact_b = EXACT_B[scheme]
  b_want, b_other = (exact_b, rounded_b) if spectral else (rounded_b, exact_b)
  want, other = y, y
  fragile = np.zeros(y.shape[0], dtype=bool)
  f = None
  for s in range(len(a)):
    us = y
    if s > 0:
      us = y + f * (np.float64(np.float32(a[s])) * dt)
      if not spectral:   # (a float64 right-hand side rounds nothing)
        fragile |= _near_float32_boundary(us).any(axis=1)
    f = _rhs(model, us, t + c[s] * dt)
    if b[s] != 0.0:
      want = want + (b_want[s] * dt) * f
      other = other + (b_other[s] * dt) * f
  return want, other, want.astype(np.float32).astype(np.float64), fragile


def _ulps(got, want, scale):
  """max |got - want| per sample in units of EPS x the sample's max|y| (NaN where both are)."""
  with np.errstate(invalid='ignore'):
    return np.nanmax(np.abs(got - want), axis=1, initial=0.0) / (EPS * scale)


def _check_steps(case_id, scheme, model, traj, label):
  """Every step of traj against the host composition; returns the largest error in ulps."""
  dt, t0 = _dt(case_id), _t0(model)
  worst = 0.0
  far_b = far_round = 0.0
  left_out = []
  for k in range(traj.shape[0] - 1):
    y, got = traj[k], traj[k + 1]
    want, other_b, rounded, fragile = _host_step(model, scheme, y, t0 + k * dt, dt)
    scale = np.abs(y).max(axis=1)
    increment = np.abs(got - y).max() / np.abs(y).max()
    assert increment >= MIN_INCREMENT, (label, k, increment)
    left_out += [(int(sample), k) for sample in np.flatnonzero(fragile)]
    keep = ~fragile
    assert np.isfinite(got).all() and np.isfinite(want).all(), (label, k)
    worst = max(worst, _ulps(got[keep], want[keep], scale[keep]).max(initial=0.0))
    far_b = max(far_b, _ulps(got[keep], other_b[keep], scale[keep]).max(initial=0.0))
    far_round = max(far_round, _ulps(got[keep], rounded[keep], scale[keep]).max(initial=0.0))
  if left_out:
    print(label, '(sample, step) pairs left out (float32 rounding boundary):', left_out)
  print('{}: route {!r}, largest error {:.2f} x 2.2e-16 max|y|; other b weights {:.3g}, '
        'float32-rounded state {:.3g}'.format(label, CASES[case_id].route, worst, far_b, far_round))
  assert len(left_out) <= 1, (label, left_out)
  assert worst <= ULPS, (label, worst)
  if scheme in ('bs3', 'rk4'):
    assert far_b > MUTANT, (label, 'the other b-weight convention is not told apart', far_b)
    assert far_round > MUTANT, (label, 'a float32-rounded state is not told apart', far_round)
  return worst


PARAMS = [(case_id, scheme) for case_id, case in CASES.items() for scheme in case.schemes]


@pytest.mark.parametrize('case_id,scheme', PARAMS)
def test_one_step_of_host_float64_over_the_device_rhs(case_id, scheme):
  model, _, _ = _setup(case_id)
  traj = _trajectory(case_id, scheme)
  _check_steps(case_id, scheme, model, traj, '{}/{}'.format(case_id, scheme))


@pytest.mark.parametrize('case_id', ORACLE_CASES)
def test_bs3_against_the_oracle(case_id):
  """The first three samples of the BS3 run against oracle.integrate_fixed with a float64
  state (SpectralModel: the float64 right-hand side of oracle.spectral_time_derivative under
  the same tableau arithmetic, exact b weights)."""
  case = CASES[case_id]
  model, y0, forcing = _setup(case_id)
  got = _trajectory(case_id, 'bs3')[1:, :3]
  dt, t0 = _dt(case_id), _t0(model)
  if _is_spectral(model):
    spec = model.spec()
    a, b, _ = oracle.TABLEAUS[oracle.SCHEME_BS3]
    y, rows = y0[:3], []
    for _ in range(case.steps):
      ynew, f = y, None
      for s in range(3):
        us = y if s == 0 else y + f * (a[s] * dt)
        f = oracle.spectral_time_derivative(spec['equation'], us, spec['derivative_orders'],
                                            spec['period'], spec['eta'], spec['dx'])
        ynew = ynew + (EXACT_B['bs3'][s] * dt) * f
      y = ynew
      rows.append(y)
    want = np.stack(rows)
  else:
    sub = None if forcing is None else {k: v[:3] for k, v in forcing.items()}
    want = oracle.integrate_fixed(model.spec(), oracle.SCHEME_BS3, t0, dt, case.steps, 1,
                                  y0[:3], forcing=sub, state_dtype=np.float64)
  err = rel_err(got, want)
  print(case_id, 'route {!r}: BS3 against the oracle {:.2e}'.format(case.route, err))
  assert err < (TOL64 if _is_spectral(model) else TOL)


EDGE_CASES = ('burgers_cons32', 'fixed_ks100')


@pytest.mark.parametrize('case_id', EDGE_CASES)
def test_save_every_that_does_not_divide_the_steps(case_id):
  model, y0, _ = _setup(case_id)
  full = _run(case_id, y0, 'bs3', 5)
  sparse = _run(case_id, y0, 'bs3', 5, save_every=2)
  assert sparse.shape == (2,) + y0.shape
  np.testing.assert_array_equal(sparse[0], full[1])
  np.testing.assert_array_equal(sparse[1], full[3])


@pytest.mark.parametrize('case_id', EDGE_CASES)
def test_zero_steps(case_id):
  model, y0, _ = _setup(case_id)
  none = model.integrate_fixed(y0.copy(), 0, dt=_dt(case_id), scheme='bs3', state_dtype='float64')
  assert tuple(none.shape) == (0,) + y0.shape and str(none.dtype) == 'torch.float64'


@pytest.mark.parametrize('case_id', EDGE_CASES)
def test_nan_in_one_grid_point(case_id):
  """A NaN in one grid point of one sample: after every step the device's NaN mask is the
  host composition's (the same right-hand side, stage by stage), every other sample stays
  finite and within the bound."""
  case = CASES[case_id]
  model, y0, _ = _setup(case_id)
  poisoned = 1
  y0 = y0.copy()
  y0[poisoned, y0.shape[1] // 3] = np.nan
  traj = np.concatenate([y0[None], _run(case_id, y0, 'bs3', case.steps)])
  dt, t0 = _dt(case_id), _t0(model)
  others = np.arange(case.batch) != poisoned
  left_out = []
  for k in range(case.steps):
    y, got = traj[k], traj[k + 1]
    want, _, _, fragile = _host_step(model, 'bs3', y, t0 + k * dt, dt)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[poisoned]).sum() > np.isnan(y[poisoned]).sum() or np.isnan(got[poisoned]).all()
    assert np.isfinite(got[others]).all()
    left_out += [(int(sample), k) for sample in np.flatnonzero(fragile & others)]
    keep = others & ~fragile
    worst = _ulps(got[keep], want[keep], np.abs(y[keep]).max(axis=1)).max()
    assert worst <= ULPS, (case_id, k, worst)
  print(case_id, 'NaN grid points of the poisoned sample per step:',
        np.isnan(traj[:, poisoned]).sum(axis=1).tolist(), 'left out:', left_out)
  assert len(left_out) <= 1, left_out
