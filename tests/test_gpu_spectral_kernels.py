"""rhs_spectral.h (substep_kernel, adaptive_kernel<kPts>, circulant_apply_kernel, the in-LDS
FFT) on full-spectrum states, ragged grids and failing samples.

Every state of the right-hand-side tests carries all wavenumbers 0 .. N/2 (spectral_cases.
trig_state), so each Fourier multiplier, each row of the uploaded tables and the Nyquist bin
move the result; the reference is the long-double term-by-term derivative, held to the host FFT
calls at TOL64 / 4 in test_cpu_spectral_cases.py.  Grids: spectral_cases.GRIDS (DESIGN 5,
"Spectral kernels")."""
import functools

import numpy as np
import pytest

import spectral_cases as sc
from helpers import oracle, rel_err
from ddd1d_amd import _lib, equations, integrate, model as model_lib

pytestmark = pytest.mark.gpu
TOL64 = sc.TOL64
U = 2.0 ** -53   # float64 unit roundoff


@functools.lru_cache(maxsize=None)
def _model(cls_name, n, convention):
  return model_lib.SpectralModel(sc.make_equation(cls_name, n), convention=convention)


def _grid_cases(fn):
  fn = pytest.mark.parametrize('convention', sc.CONVENTIONS)(fn)
  fn = pytest.mark.parametrize('cls_name', sc.EQUATIONS)(fn)
  return pytest.mark.parametrize('n,mode', sc.GRIDS)(fn)


# ---------------------------------------------------------------------------
# 1. the right-hand side on a full spectrum
# ---------------------------------------------------------------------------
@_grid_cases
def test_full_spectrum_rhs_vs_long_double_truth(n, mode, cls_name, convention):
  """SpectralModel.time_derivative of three different full-spectrum samples against
  equation_of_motion over the exact derivatives in long double: TOL64 of each sample's max
  norm, in circulant and in FFT mode alike (no k_max^order allowance: on these states the
  result is as large as its highest multiplier).  A sample evaluated alone equals its row of
  the batched call bit for bit."""
  model = _model(cls_name, n, convention)
  eq = model.equation
  u, _, truth = sc.batch_states(eq, convention)
  # the grid reaches the form its row of the table names
  circulant_fma = len(eq.DERIVATIVE_ORDERS) * n
  assert (model.fma_per_point == circulant_fma) == (mode == 'circulant'), model.fma_per_point
  got = model.time_derivative(u).cpu().numpy()
  assert got.dtype == np.float64 and got.shape == u.shape
  device = sc.rel_max(got, truth)
  host = sc.rel_max(sc.host_rhs(eq, convention, u), truth)
  print('rhs', cls_name, n, mode, convention,
        'device/truth {:.2e} host/truth {:.2e}'.format(device, host))
  assert device < TOL64
  for b in range(sc.BATCH):
    alone = model.time_derivative(u[b:b + 1]).cpu().numpy()
    np.testing.assert_array_equal(alone[0], got[b])


# ---------------------------------------------------------------------------
# 2. the host-built impulse responses, one derivative at a time
# ---------------------------------------------------------------------------
@_grid_cases
def test_impulse_responses_per_derivative(n, mode, cls_name, convention):
  """circulant_apply(model.kernels[d], u) against the exact derivative d -- on the FFT grids
  too, where the model itself never applies its kernels directly (ddd_circulant_apply_f64
  takes any n <= 2048).  With the test above it ties the FFT form to the circulant form on
  one input."""
  model = _model(cls_name, n, convention)
  eq = model.equation
  spec = eq.kernel_spec()
  u, derivs, _ = sc.batch_states(eq, convention)
  for d, order in enumerate(spec['derivative_orders']):
    got = _lib.circulant_apply(model.kernels[d], u).cpu().numpy()
    device = sc.rel_max(got, derivs[..., d])
    host = sc.rel_max(sc.host_derivative(convention, u, order, spec['period']), derivs[..., d])
    print('deriv', cls_name, n, mode, convention, 'order', order,
          'device/truth {:.2e} host/truth {:.2e}'.format(device, host))
    assert device < TOL64, (order, device)


# ---------------------------------------------------------------------------
# 3. ddd_rk_substep_f64, argument by argument
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', (258, 512))
def test_rk_substep_f64_arguments(n):
  """y_out = y_base + c1 f, acc_out = acc_in + c2 f with every pointer absent, present and
  aliased; f = the device's own time_derivative(y_in).  Expected: base + c f in NumPy float64;
  allowed: 2^-53 |c f| + 2^-53 |result| per element (the compiler may fuse base + c f, which
  is one rounding of the product).  include/ddd1d.h declares ddd_rk_substep_f64 as
  ddd_rk_substep in float64, whose "y_out / acc_out may alias their inputs": y_out is y_in is
  allowed and tested."""
  import torch
  model = _model('KSEquation', n, 'fftpack')
  u, _, _ = sc.batch_states(model.equation, 'fftpack')
  y_in = torch.from_numpy(u).cuda()
  f = model.time_derivative(y_in).cpu().numpy()
  rs = np.random.RandomState(n)
  base_np = rs.uniform(-1.0, 1.0, size=u.shape) * np.abs(f).max()
  acc_np = rs.uniform(-1.0, 1.0, size=u.shape) * np.abs(f).max()
  c1, c2 = 0.37, -1.25   # c1 != c2, one negative

  def expect(base, c):
    cf = c * f
    want = cf if base is None else base + cf
    return want, U * np.abs(cf) + U * np.abs(want)

  def check(got, base, c, label):
    want, allowed = expect(base, c)
    excess = np.abs(got.cpu().numpy() - want) - allowed
    assert excess.max() <= 0.0, (n, label, float(excess.max()))

  def fresh():
    return (torch.from_numpy(base_np).cuda(), torch.from_numpy(acc_np).cuda(),
            torch.full_like(y_in, np.nan), torch.full_like(y_in, np.nan))

  # y_out only: y_base absent, present, y_base is y_in
  base, acc, y_out, acc_out = fresh()
  model.rk_substep(0.0, y_in, None, c1, y_out)
  check(y_out, None, c1, 'y_out only')
  model.rk_substep(0.0, y_in, base, c1, y_out)
  check(y_out, base_np, c1, 'y_out, y_base')
  model.rk_substep(0.0, y_in, y_in, c1, y_out)
  check(y_out, u, c1, 'y_out, y_base is y_in')
  # acc_out only: acc_in absent, present, acc_out is acc_in
  model.rk_substep(0.0, y_in, acc_in=None, c2=c2, acc_out=acc_out)
  check(acc_out, None, c2, 'acc_out only')
  model.rk_substep(0.0, y_in, acc_in=acc, c2=c2, acc_out=acc_out)
  check(acc_out, acc_np, c2, 'acc_out, acc_in')
  model.rk_substep(0.0, y_in, acc_in=acc, c2=c2, acc_out=acc)
  check(acc, acc_np, c2, 'acc_out is acc_in')
  # both outputs, two different coefficients
  base, acc, y_out, acc_out = fresh()
  model.rk_substep(0.0, y_in, base, c1, y_out, acc, c2, acc_out)
  check(y_out, base_np, c1, 'both: y_out')
  check(acc_out, acc_np, c2, 'both: acc_out')
  y_out.fill_(np.nan); acc_out.fill_(np.nan)
  model.rk_substep(0.0, y_in, None, c2, y_out, None, c1, acc_out)
  check(y_out, None, c2, 'both, no bases: y_out')
  check(acc_out, None, c1, 'both, no bases: acc_out')
  # no input was written
  np.testing.assert_array_equal(y_in.cpu().numpy(), u)
  np.testing.assert_array_equal(base.cpu().numpy(), base_np)
  np.testing.assert_array_equal(acc.cpu().numpy(), acc_np)
  # y_out is y_in (and y_base): the stage input is read whole before any point is written
  state = y_in.clone()
  model.rk_substep(0.0, state, state, c1, state, acc, c2, acc_out)
  check(state, u, c1, 'y_out is y_in is y_base')
  check(acc_out, acc_np, c2, 'y_out is y_in: acc_out')
  with pytest.raises(_lib.DDDError, match='both y_out and acc_out are NULL'):
    model.rk_substep(0.0, y_in, base, c1, None, acc, c2, None)


# ---------------------------------------------------------------------------
# 4. ddd_integrate_fixed_f64 on spectral models
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', (258, 512))
@pytest.mark.parametrize('scheme', ('euler', 'midpoint', 'bs3', 'rk4'))
def test_fixed_step_f64_every_scheme(scheme, n):
  """Seven steps, rows after steps 3 and 6, against NumPy float64 stepping over the host
  FFT right-hand side (test_cpu_spectral_cases.py: the same stepping over a float64 circulant
  product of model.kernels stays within TOL64 / 4 of it); num_steps = 0 writes no row."""
  eq, y0, dt = sc.fixed_step_case(n)
  model = _model('KdVEquation', n, 'fftpack')
  got = model.integrate_fixed(y0, 7, dt=dt, scheme=scheme, save_every=3).cpu().numpy()
  want = sc.step_fixed(lambda y: sc.host_rhs(eq, 'fftpack', y), scheme, y0, dt, 7, 3)
  assert got.shape == want.shape == (2, sc.BATCH, n) and got.dtype == np.float64
  err = max(sc.rel_max(got[r], want[r]) for r in range(2))
  print('fixed', scheme, n, 'device/host {:.2e}'.format(err))
  assert err < TOL64
  assert np.abs(want[1] - want[0]).max() > 1e-6   # the rows are different states
  none = model.integrate_fixed(y0, 0, dt=dt, scheme=scheme, save_every=3)
  assert tuple(none.shape) == (0, sc.BATCH, n)


# ---------------------------------------------------------------------------
# 5. the adaptive solver at 2, 3 and 5 points per thread
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('cls_name,n', [('KdVEquation', 384), ('KdVEquation', 640),
                                        ('KdVEquation', 1280), ('KSEquation', 384)])
def test_adaptive_ragged_grids(cls_name, n):
  """adaptive_kernel<2 / 4 / 8> with masked trips (384 = 1.5, 640 = 2.5, 1280 = 5 x 256
  points), from t0 = 0.3, with unequally spaced output times of which two fall inside one
  accepted step -- against SciPy's RK23 over SpectralDifferentiator: equal evaluation
  counts, status 0, 1e-9.  Saturated controller: max_step = half the RK23 stability limit
  of the stiffest term (sqrt(3) / k_max^3 for u_xxx, 2.5 / k_max^4 for u_xxxx), 40 steps."""
  import scipy.integrate
  eqs = [getattr(equations, cls_name)(n, random_seed=s) for s in (3, 5)]
  eq = eqs[0]
  kmax = 2 * np.pi * (n // 2) / eq.grid.period
  limit = np.sqrt(3) / kmax ** 3 if cls_name == 'KdVEquation' else 2.5 / kmax ** 4
  max_step = 0.5 * limit
  times = 0.3 + max_step * np.array([0.0, 7.31, 7.52, 19.9, 33.3, 40.0])
  y0 = np.stack([e.initial_value() for e in eqs]).astype(np.float64)
  model = model_lib.SpectralModel(eq)
  y, nfev, status = model.integrate_adaptive(y0, times, max_step=max_step)
  y, nfev, status = y.cpu().numpy(), nfev.cpu().numpy(), status.cpu().numpy()
  diff = integrate.SpectralDifferentiator(eq)
  for b in range(2):
    sol = scipy.integrate.solve_ivp(diff, (times[0], times[-1]), y0[b], t_eval=times,
                                    max_step=max_step, method='RK23', dense_output=True)
    steps = sol.sol.ts   # the accepted steps' ends, t0 first
    owner = np.searchsorted(steps, times[1:], side='left')   # step whose (t_old, t] holds it
    assert len(steps) - 1 >= 40 and (np.diff(owner) == 0).any(), (len(steps), owner)
    assert sol.status == 0 and status[b] == 0
    assert int(nfev[b]) == sol.nfev, (cls_name, n, b, int(nfev[b]), sol.nfev)
    err = rel_err(y[:, b], sol.y.T)
    print('adaptive', cls_name, n, 'sample', b, 'nfev', sol.nfev, 'rel err {:.2e}'.format(err))
    assert err < 1e-9
    np.testing.assert_array_equal(y[0, b], y0[b])


# ---------------------------------------------------------------------------
# 6. a sample that fails next to samples that finish
# ---------------------------------------------------------------------------
def test_adaptive_failure_between_healthy_samples():
  """KdV from 30 x initial_value(seed 3): the step size falls below 10 ulp(t) and SciPy's
  RK23 over the host FFT right-hand side stops with status -1 (N = 64: after 746 evaluations
  with 2 of 4 rows delivered).  On the device the sample ends the same way -- status -1, the
  same rows delivered and the same rows NaN, row 0 = y0, evaluation count within 2 % of
  SciPy's (the allowance test_failure_path_nan_rows_and_status gives a chaotic tail) --
  while the samples on either side of it finish as if alone.  max_attempts = 4 x SciPy's
  attempts, so a kernel that missed the failure would stop with status -2 instead of
  spinning.  (No FFT-mode twin: at N = 512 SciPy on the host integrates the same three
  states to the end, status 0 after 15 788 evaluations for the middle one.)"""
  import scipy.integrate
  n = 64
  eq3, eq5 = (equations.KdVEquation(n, random_seed=s) for s in (3, 5))
  model = model_lib.SpectralModel(eq3, convention='fftpack')
  spec = eq3.kernel_spec()
  times = np.linspace(0.0, 0.05, 4)
  y0 = np.stack([eq3.initial_value(), 30 * eq3.initial_value(),
                 eq5.initial_value()]).astype(np.float64)
  rhs = lambda t, v: oracle.spectral_time_derivative(
      spec['equation'], v, spec['derivative_orders'], spec['period'], spec['eta'], spec['dx'])
  sols = [scipy.integrate.solve_ivp(rhs, (times[0], times[-1]), y0[b], t_eval=times,
                                    max_step=0.01, method='RK23') for b in range(3)]
  bad = sols[1]
  assert bad.status == -1 and (bad.nfev, bad.y.shape[1]) == (746, 2), (bad.status, bad.nfev)
  attempts = (bad.nfev - 2) // 3
  y, nfev, status = model.integrate_adaptive(y0, times, max_attempts=4 * attempts)
  y, nfev, status = y.cpu().numpy(), nfev.cpu().numpy(), status.cpu().numpy()
  print('failure', 'scipy nfev', bad.nfev, 'rows', bad.y.shape[1], 'device nfev', nfev,
        'status', status)
  assert status[1] == -1
  delivered = bad.y.shape[1]
  assert np.isfinite(y[:delivered, 1]).all() and np.isnan(y[delivered:, 1]).all()
  np.testing.assert_array_equal(y[0, 1], y0[1])
  assert abs(int(nfev[1]) - bad.nfev) <= 0.02 * bad.nfev, (int(nfev[1]), bad.nfev)
  for b in (0, 2):
    assert sols[b].status == 0 and status[b] == 0
    assert int(nfev[b]) == sols[b].nfev, (b, int(nfev[b]), sols[b].nfev)
    assert rel_err(y[:, b], sols[b].y.T) < 1e-9


# ---------------------------------------------------------------------------
# 7. ddd_circulant_apply_f64 at the sizes its loops branch on
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 2, 7, 255, 257, 1000, 2048))
def test_circulant_apply_shapes(n):
  """Five rows, random kernel and input, against the long-double circulant product.  Bound,
  derived: the kernel forms each output as n fused multiply-adds in sequence, so its error is
  at most n 2^-53 sum_j |c_(x - j)| |in_j| (Higham, Accuracy and Stability, 3.1: gamma_n, with
  n u << 1).  In place equals out of place bit for bit."""
  import torch
  rs = np.random.RandomState(100 + n)
  kernel = rs.uniform(-1.0, 1.0, size=n)
  x = rs.uniform(-1.0, 1.0, size=(5, n))
  got = _lib.circulant_apply(kernel, x).cpu().numpy()
  want = sc.circulant_product(kernel, x, np.longdouble)
  bound = n * U * sc.circulant_product(np.abs(kernel), np.abs(x), np.longdouble)
  excess = np.abs(got.astype(np.longdouble) - want) - bound
  print('circulant', n, 'largest error / bound {:.3f}'.format(
      float((np.abs(got.astype(np.longdouble) - want) / bound).max())))
  assert excess.max() <= 0
  lib = _lib.load_library()
  k_dev = torch.from_numpy(kernel).cuda()
  in_place = torch.from_numpy(x).cuda()
  _lib.check(lib.ddd_circulant_apply_f64(k_dev.data_ptr(), in_place.data_ptr(),
                                         in_place.data_ptr(), 5, n, _lib.current_stream()))
  np.testing.assert_array_equal(in_place.cpu().numpy(), got)


def test_circulant_apply_zero_rows_and_refusals():
  import torch
  lib = _lib.load_library()
  kernel = torch.ones(8, dtype=torch.float64, device='cuda')
  x = torch.ones(8, dtype=torch.float64, device='cuda')
  out = torch.full((8,), -3.0, dtype=torch.float64, device='cuda')
  call = lambda rows, n: lib.ddd_circulant_apply_f64(
      kernel.data_ptr(), x.data_ptr(), out.data_ptr(), rows, n, _lib.current_stream())
  _lib.check(call(0, 8))   # zero rows: nothing is launched, nothing is written
  torch.cuda.synchronize()
  assert (out.cpu().numpy() == -3.0).all()
  for n in (0, 2049):
    with pytest.raises(_lib.DDDError, match='1 <= n <= 2048'):
      _lib.check(call(1, n))
  with pytest.raises(_lib.DDDError, match='1 <= n <= 2048'):
    _lib.check(call(-1, 8))
  with pytest.raises(_lib.DDDError, match='1 <= n <= 2048'):
    _lib.circulant_apply(np.ones(2049), np.ones((1, 2049)))
  assert (out.cpu().numpy() == -3.0).all()


# ---------------------------------------------------------------------------
# 8. what ddd_spectral_create refuses
# ---------------------------------------------------------------------------
def test_spectral_create_refusals():
  y = lambda n: np.zeros((1, n))
  # (fftpack.diff takes an odd N on the host; the rfft form already refuses it there)
  odd = model_lib.SpectralModel(equations.KdVEquation(63), convention='fftpack')
  with pytest.raises(_lib.DDDError, match=r'even num_points <= 2048 \(got 63\)'):
    odd.time_derivative(y(63))
  big = model_lib.SpectralModel(equations.KdVEquation(2050), convention='fftpack')
  with pytest.raises(_lib.DDDError, match=r'even num_points <= 2048 \(got 2050\)'):
    big.time_derivative(y(2050))
  # (SpectralModel refuses a flux-form equation on the host: hand the library one anyway)
  flux = model_lib.SpectralModel(equations.KdVEquation(64), convention='fftpack')
  flux.equation = equations.ConservativeKdVEquation(64)
  with pytest.raises(_lib.DDDError, match='non-flux equations only'):
    flux.time_derivative(y(64))
  short = model_lib.SpectralModel(equations.KSEquation(64), convention='rfft')
  short.kernels = np.ascontiguousarray(short.kernels[:, :-1])
  with pytest.raises(_lib.DDDError, match=r'kernels must hold D\*N = 192 doubles, got 189'):
    short.time_derivative(y(64))
  # and the entry points still take a well-formed model afterwards
  good = _model('KSEquation', 64, 'rfft')
  assert np.isfinite(good.time_derivative(sc.batch_states(good.equation, 'rfft')[0])
                     .cpu().numpy()).all()
