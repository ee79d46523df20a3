"""On-device batched adaptive RK23 (`ddd_integrate_adaptive_f64`) against the
reference's per-sample SciPy loop (integrate.odeint, integrate.py:143-169;
scripts/run_evaluation.py:152-174): per-sample nfev EQUAL to solve_ivp's and
trajectories within 1e-5, for the three equation families, one-wave and
four-wave geometries, saturated and controller-limited step sizes, and the
failure path (NaN rows + status -1).

The checker is `oracle.odeint_rk23` = the installed SciPy over the NumPy
right-hand side -- SciPy is the reference's own third-party integrator."""
import numpy as np
import pytest

from helpers import (FLOOR_CEILING, assert_near_truth, batch_forcing, make_model, oracle,
                     random_phase_ic, rel_err)
from ddd1d_amd import equations, integrate, model as model_lib

pytestmark = pytest.mark.gpu

TOL = 1e-5   # north_star: fp32 trajectories within 1e-5 rel of the reference
# Where the dynamics amplify rounding noise (controller-limited steps of the
# dispersive / fourth-order equations, untrained stencils) the float32
# right-hand side itself is only defined up to its rounding: the reference's
# own SciPy run moves by `floor` when the stencil apply + equation of motion
# are evaluated in float64 instead of float32 (same float32 coefficients, same
# controller).  The device trajectory must stay within max(TOL, 4 floor) of the
# reference run -- `floor` is measured per sample and printed, never assumed.


def _one(forcing, b):
  return None if forcing is None else {k: np.asarray(v)[b] for k, v in forcing.items()}


def _check(model, y0, times, forcing=None, max_step=0.01, tol=TOL, samples=None,
           hip_samples=(), **solver):
  """Device controllers vs SciPy per sample.

  Every sample in ``samples`` (default: all) is compared with the reference run
  (SciPy over the NumPy right-hand side): nfev mismatches are collected in
  ``bad``, trajectories must agree to max(tol, 4 x the measured float32 noise
  floor of that reference run).  Every sample in ``hip_samples`` is also
  compared with SciPy driving the SAME HIP right-hand side one sample at a time
  (the reference's execution shape, integrate.py:48-71 + 143-169): there the
  only difference left is the summation order of the error norm, so nfev must
  be equal and the trajectories agree to float64 rounding amplified by the
  dynamics (1e-9).
  """
  if forcing is not None:
    model.set_forcing(forcing)
  y, nfev, status = model.integrate_adaptive(y0, times, max_step=max_step, **solver)
  y = y.cpu().numpy()
  nfev = nfev.cpu().numpy()
  status = status.cpu().numpy()
  assert y.shape == (len(times),) + y0.shape and y.dtype == np.float64
  spec = model.spec()
  bad = []
  worst = 0.0
  for b in (range(y0.shape[0]) if samples is None else samples):
    want, want_nfev = _scipy(spec, y0[b], times, _one(forcing, b), max_step, **solver)
    if want_nfev != nfev[b]:
      bad.append((b, int(nfev[b]), want_nfev))
    finite = np.isfinite(want).all(axis=1)
    if want_nfev == nfev[b]:
      np.testing.assert_array_equal(np.isfinite(y[:, b]).all(axis=1), finite)
      assert (status[b] == 0) == bool(finite.all())
    finite &= np.isfinite(y[:, b]).all(axis=1)
    err = rel_err(y[finite, b], want[finite])
    worst = max(worst, err)
    if err >= tol:
      truth, _ = _scipy(spec, y0[b], times, _one(forcing, b), max_step,
                        f64_apply=True, **solver)
      both = finite & np.isfinite(truth).all(axis=1)
      floor = rel_err(truth[both], want[both])
      print('sample {}: err {:.1e}, float32 noise floor of the reference run {:.1e}'
            .format(b, err, floor))
      assert floor < FLOOR_CEILING and err < 4 * floor, (b, err, floor)
      # ... and the device run is as close to the float64-apply run as the reference run is
      # (x TRUTH_RATIO), not merely inside the triangle bound
      assert_near_truth(y[both, b], truth[both], floor, 'adaptive sample %d' % b)
  for b in hip_samples:
    want, want_nfev = _scipy_over_hip_rhs(model, y0[b], times, _one(forcing, b), max_step,
                                          **solver)
    assert want_nfev == nfev[b], (b, int(nfev[b]), want_nfev)
    np.testing.assert_array_equal(np.isfinite(y[:, b]), np.isfinite(want))
    finite = np.isfinite(want).all(axis=1)
    err = rel_err(y[finite, b], want[finite])
    assert err < 1e-9, (b, err)
  if forcing is not None and len(hip_samples):
    model.set_forcing(forcing)
  return nfev, status, bad, worst


def _scipy_over_hip_rhs(model, y0, times, forcing, max_step, rtol=1e-3, atol=1e-6):
  """solve_ivp on the host, one sample, calling ddd_time_derivative (batch 1)."""
  import scipy.integrate
  if forcing is not None:
    model.set_forcing({k: np.asarray(v)[None] for k, v in forcing.items()})

  def fun(t, y):
    return model.time_derivative(np.asarray(y, np.float32)[None], t)[0].cpu().numpy()
  sol = scipy.integrate.solve_ivp(fun, (times[0], times[-1]), np.asarray(y0, np.float64),
                                  t_eval=times, max_step=max_step, method='RK23',
                                  rtol=rtol, atol=atol)
  y = sol.y.T
  if len(times) - y.shape[0]:
    y = np.pad(y, ((0, len(times) - y.shape[0]), (0, 0)), mode='constant',
               constant_values=np.nan)
  return y, sol.nfev


def _scipy(spec, y0, times, forcing, max_step, rtol=1e-3, atol=1e-6, f64_apply=False):
  import scipy.integrate
  one = None if forcing is None else {k: np.asarray(v)[None] for k, v in forcing.items()}

  def fun(t, y):
    if not f64_apply:
      return oracle.time_derivative(spec, t, y[None, :], one)[0]
    # float32 coefficients (the conv tower as the reference runs it), then stencil
    # apply, equation of motion and forcing in float64; returned as float32
    y32 = np.asarray(y[None, :], np.float32)
    if spec.get('baseline_coefficients') is not None:
      return oracle.time_derivative(spec, t, y[None, :], one)[0]
    coeff = oracle.predict_coefficients(y32, spec).astype(np.float64)
    patches = oracle.extract_patches(y32.astype(np.float64), coeff.shape[3])
    derivs = np.einsum('bxdi,bxi->bxd', coeff, patches)
    y_t = oracle.equation_of_motion(spec['equation'], y32.astype(np.float64), derivs,
                                    spec['eta'], spec['dx'])
    if spec.get('forced', False) and one is not None:
      y_t = y_t + oracle.forcing_f64(t, one, spec['num_points'], spec['resample_factor'],
                                     spec['period'], spec['conservative'])
    return y_t[0].astype(np.float32)
  sol = scipy.integrate.solve_ivp(fun, (times[0], times[-1]), np.asarray(y0, np.float64),
                                  t_eval=times, max_step=max_step, method='RK23',
                                  rtol=rtol, atol=atol)
  y = sol.y.T
  if len(times) - y.shape[0]:
    y = np.pad(y, ((0, len(times) - y.shape[0]), (0, 0)), mode='constant',
               constant_values=np.nan)
  return y, sol.nfev


@pytest.mark.parametrize('equation,conservative', [
    ('burgers', True), ('burgers', False), ('kdv', True), ('kdv', False),
    ('ks', True), ('ks', False)])
def test_reference_settings_n64(equation, conservative):
  """max_step = 0.01, rtol 1e-3, atol 1e-6 (integrate.py:154): B = 64 samples in
  one launch, each with its own controller, forcing and nfev."""
  batch = 64
  model = make_model(equation, conservative, num_points=64, resample_factor=4)
  assert model.kernel_name == 'mfma_f32_r64'   # (before any launch; 64 samples run four wavefronts each)
  scale = 0.3 if equation == 'burgers' else 1.0
  y0 = (scale * random_phase_ic(model.equation, batch)).astype(np.float64)
  forcing = batch_forcing(batch) if equation == 'burgers' else None
  times = np.linspace(0.0, 0.2, 5)
  nfev, status, bad, worst = _check(model, y0, times, forcing, hip_samples=(0, 37))
  print(equation, conservative, 'nfev', nfev.min(), nfev.max(), 'worst rel err {:.1e}'.format(worst))
  assert not bad, bad
  assert (status == 0).all()


@pytest.mark.parametrize('equation,num_points,max_step', [
    ('burgers', 64, np.inf), ('burgers', 32, np.inf), ('burgers', 16, 0.05),
    ('kdv', 64, np.inf), ('ks', 64, np.inf)])
def test_controller_limited_steps(equation, num_points, max_step):
  """No max_step ceiling: every step size comes from the error controller
  (initial step selection, growth, rejections), several samples per wavefront
  for N < 64."""
  batch = 40   # not a multiple of the samples per workgroup for N = 16
  model = make_model(equation, True, num_points=num_points, resample_factor=4)
  scale = 0.5 if equation == 'burgers' else 1.0
  y0 = (scale * random_phase_ic(model.equation, batch)).astype(np.float64)
  forcing = batch_forcing(batch) if equation == 'burgers' else None
  times = np.array([0.0, 0.013, 0.1, 0.25, 0.4])   # not aligned with any step
  nfev, status, bad, worst = _check(model, y0, times, forcing, max_step=max_step,
                                    hip_samples=(1, 39))
  print(equation, num_points, 'nfev', nfev.min(), nfev.max(), 'worst {:.1e}'.format(worst),
        'mismatched', bad)
  if max_step == np.inf:
    assert len(np.unique(nfev)) > 1, 'samples should need different numbers of steps'
  assert not bad, bad
  assert (status == 0).all()


def test_ks256_four_wave_groups():
  """BASELINE configs[3] geometry (KS N = 256, one sample per 256-row
  workgroup): the step is stability-limited (dt ~ 4e-4 << max_step), the
  controller rejects and regrows continuously.  In this regime accept / reject
  decisions sit on the stability boundary and amplify rounding noise: SciPy
  over the NumPy right-hand side and SciPy over the HIP right-hand side (two
  float32 evaluations of the same formulas) already take different numbers of
  steps.  So the sharp check is against SciPy over the SAME right-hand side
  (every sample: equal nfev, 1e-9); against the NumPy run the step counts
  scatter by ~10 %, like that run's own count does when its stencil apply is
  done in float64 (printed), and the trajectories stay within the measured
  float32 noise floor."""
  batch = 8
  model = make_model('ks', True, num_points=256, resample_factor=2)
  assert model.kernel_name == 'mfma_f32_r256'
  y0 = random_phase_ic(model.equation, batch).astype(np.float64)
  times = np.linspace(0.0, 0.02, 5)
  nfev, status, bad, worst = _check(model, y0, times, hip_samples=range(batch))
  print('ks256 nfev', nfev, 'worst {:.1e}'.format(worst), 'vs NumPy-RHS run', bad)
  assert nfev.min() > 100 and (status == 0).all()
  spec = model.spec()
  for b, got, want in bad:
    _, alt = _scipy(spec, y0[b], times, None, 0.01, f64_apply=True)
    print('sample {}: nfev device {} / NumPy float32 run {} / NumPy run with float64 apply {}'
          .format(b, got, want, alt))
    assert abs(got - want) <= 0.15 * want, (b, got, want, alt)


def test_ks256_saturated_controller_vs_oracle():
  """The same KS N = 256 model away from the stability boundary: max_step = 2e-4
  keeps the controller saturated (101 accepted steps to t = 0.02, no rejection:
  nfev = 2 + 3 x 101 = 305), so no accept / reject decision can amplify rounding
  noise and the ORACLE check is deterministic: per-sample nfev EQUAL to the
  reference run (SciPy over the NumPy right-hand side) and trajectories within
  max(1e-5, 4 x measured floor) over >= 100 steps -- right-hand-side parity for
  BASELINE configs[3]'s equation under the production integrator, next to the
  statistical check above."""
  batch = 8
  model = make_model('ks', True, num_points=256, resample_factor=2)
  assert model.kernel_name == 'mfma_f32_r256'
  y0 = random_phase_ic(model.equation, batch).astype(np.float64)
  times = np.linspace(0.0, 0.02, 5)
  nfev, status, bad, worst = _check(model, y0, times, max_step=2e-4, hip_samples=(0, 5))
  print('ks256 saturated: nfev', nfev, 'worst rel err vs the oracle run {:.1e}'.format(worst))
  assert not bad, bad
  assert (nfev == 305).all() and (status == 0).all()
  assert worst < TOL


def test_n128_two_samples_per_group_and_non_power_of_two():
  for num_points in (128, 96):
    model = make_model('kdv', True, num_points=num_points, resample_factor=2)
    assert model.kernel_name == 'mfma_f32_r256'
    y0 = random_phase_ic(model.equation, 5).astype(np.float64)
    times = np.linspace(0.0, 0.05, 3)
    nfev, status, bad, worst = _check(model, y0, times, hip_samples=range(5))
    print('kdv', num_points, nfev, 'worst {:.1e}'.format(worst))
    assert not bad, bad


def test_fixed_stencil_baseline_and_runtime_kernels():
  """PolynomialDifferentiator models (integrate_baseline, integrate.py:296-308)
  and a non-default net run on the run-time-parameterised adaptive kernel."""
  eq = make_model('burgers', True, num_points=32, resample_factor=4).equation
  base = model_lib.BaselineModel(eq, accuracy_order=1)
  y0 = (0.5 * random_phase_ic(eq, 6)).astype(np.float64)
  times = np.linspace(0.0, 0.3, 4)
  forcing = batch_forcing(6)
  base.set_forcing(forcing)
  y, nfev, status = base.integrate_adaptive(y0, times)
  spec = base.spec()
  for b in range(6):
    want, want_nfev = _scipy(spec, y0[b], times, _one(forcing, b), 0.01)
    assert want_nfev == int(nfev[b])
    assert rel_err(y[:, b].cpu().numpy(), want) < TOL
  deep = make_model('kdv', False, num_points=64, resample_factor=4, num_layers=4,
                    nonlinearity='tanh')
  y0 = random_phase_ic(deep.equation, 4).astype(np.float64)
  nfev, status, bad, worst = _check(deep, y0, np.linspace(0, 0.1, 3))
  assert not bad, bad


def test_failure_path_nan_rows_and_status():
  """A state that blows up: SciPy shrinks the step until it is below 10 ulp(t),
  returns status -1 and integrate.odeint NaN-pads the rows not reached
  (integrate.py:161-167).  Other samples of the same launch are unaffected."""
  model = make_model('burgers', False, num_points=64, resample_factor=4)
  y0 = (0.3 * random_phase_ic(model.equation, 4)).astype(np.float64)
  y0[2] *= 400.0   # anti-diffusive learned stencils at this amplitude: finite-time blow-up
  times = np.linspace(0.0, 0.5, 6)
  forcing = batch_forcing(4)
  model.set_forcing(forcing)
  y, nfev, status = model.integrate_adaptive(y0, times)
  y, nfev, status = y.cpu().numpy(), nfev.cpu().numpy(), status.cpu().numpy()
  want, want_nfev = _scipy(model.spec(), y0[2], times, _one(forcing, 2), 0.01)
  print('blow-up sample: nfev', nfev[2], 'scipy', want_nfev, 'status', status)
  if np.isnan(want).any():
    assert status[2] == -1
    np.testing.assert_array_equal(np.isnan(y[:, 2]).all(axis=1), np.isnan(want).all(axis=1))
    assert abs(int(nfev[2]) - want_nfev) <= 0.02 * want_nfev   # chaotic tail before the failure
  for b in (0, 1, 3):
    want_b, nfev_b = _scipy(model.spec(), y0[b], times, _one(forcing, b), 0.01)
    assert status[b] == 0 and nfev[b] == nfev_b and rel_err(y[:, b], want_b) < TOL


def test_attempt_limit_and_argument_checks():
  from ddd1d_amd import _lib
  model = make_model('kdv', True, num_points=64, resample_factor=4)
  y0 = random_phase_ic(model.equation, 3).astype(np.float64)
  y, nfev, status = model.integrate_adaptive(y0, [0.0, 1.0], max_attempts=5)
  assert (status.cpu().numpy() == -2).all() and (nfev.cpu().numpy() == 2 + 3 * 5).all()
  assert np.isnan(y[1].cpu().numpy()).all() and np.array_equal(y[0].cpu().numpy(), y0)
  with pytest.raises(_lib.DDDError):
    model.integrate_adaptive(y0, [0.0, 0.0])
  with pytest.raises(_lib.DDDError):
    model.integrate_adaptive(y0, [0.0, 1.0], rtol=0.0)
  # a single output time: nothing to integrate, one evaluation (RungeKutta.__init__)
  y, nfev, status = model.integrate_adaptive(y0, [0.25])
  assert np.array_equal(y[0].cpu().numpy(), y0) and (nfev.cpu().numpy() == 1).all()
  # the same two corners on the spectral kernel (float64 right-hand side)
  eq = equations.KdVEquation(64, random_seed=1)
  spectral = model_lib.SpectralModel(eq)
  y0 = random_phase_ic(eq, 3).astype(np.float64)
  y, nfev, status = spectral.integrate_adaptive(y0, [0.0, 1.0], max_attempts=5)
  assert (status.cpu().numpy() == -2).all() and (nfev.cpu().numpy() == 2 + 3 * 5).all()
  assert np.isnan(y[1].cpu().numpy()).all() and np.array_equal(y[0].cpu().numpy(), y0)
  y, nfev, status = spectral.integrate_adaptive(y0, [0.25])
  assert np.array_equal(y[0].cpu().numpy(), y0) and (nfev.cpu().numpy() == 1).all()
  assert (status.cpu().numpy() == 0).all()

def test_generic_kernel_models():
  """Nets the MFMA path does not carry (here kernel_size = 9, filter_size = 96) and the WENO5
  exact Burgers right-hand side: one workgroup + one controller per sample on the
  generic kernel, against the reference run and against SciPy over the same
  kernel."""
  model = make_model('kdv', True, num_points=64, resample_factor=4, kernel_size=9)
  assert model.kernel_name == 'generic'
  y0 = random_phase_ic(model.equation, 5).astype(np.float64)
  nfev, status, bad, worst = _check(model, y0, np.linspace(0, 0.1, 3), hip_samples=(0, 4))
  assert not bad and (status == 0).all()
  forced = make_model('burgers', False, num_points=48, resample_factor=2, filter_size=96)
  assert forced.kernel_name == 'generic'
  y0 = (0.4 * random_phase_ic(forced.equation, 4)).astype(np.float64)
  nfev, status, bad, worst = _check(forced, y0, np.array([0.0, 0.07, 0.2]), batch_forcing(4),
                                    max_step=np.inf, hip_samples=(1, 3))
  assert not bad and (status == 0).all()


def test_integrate_batch_adaptive_dataset():
  model = make_model('burgers', True, num_points=64, resample_factor=4)
  y0 = 0.3 * random_phase_ic(model.equation, 5)
  times = np.linspace(0, 0.1, 3)
  ds = integrate.integrate_batch(model, y0, times, forcing=batch_forcing(5), adaptive=True)
  y = integrate._dataset_array(ds, 'y')
  assert y.shape == (5, 3, 64) and y.dtype == np.float64
  np.testing.assert_array_equal(y[:, 0], y0.astype(np.float64))
  evals = np.asarray(integrate._dataset_coord(ds, 'num_evals'))
  # 11 steps: the first one is select_initial_step's, shorter than max_step
  assert evals.shape == (5,) and (evals == 2 + 3 * 11).all()


def test_start_time_is_not_zero_and_single_sample_batches():
  """t_eval starting at t0 = 1.5 (the forcing is evaluated at absolute times), a
  batch of one, and a batch whose last workgroup is half empty (N = 32: two
  samples per wavefront, three samples)."""
  model = make_model('burgers', True, num_points=32, resample_factor=4)
  times = np.array([1.5, 1.52, 1.61, 1.7])
  for batch in (1, 3):
    y0 = (0.4 * random_phase_ic(model.equation, batch, seed0=77)).astype(np.float64)
    nfev, status, bad, worst = _check(model, y0, times, batch_forcing(batch, seed0=5),
                                      hip_samples=range(batch))
    assert not bad and (status == 0).all() and worst < TOL


@pytest.mark.parametrize('overrides', [dict(kernel_size=7), dict(filter_size=64),
                                       dict(kernel_size=3),
                                       dict(kernel_size=7, filter_size=64)])
def test_other_towers_adaptive(overrides):
  """The adaptive integrator on the towers with streamed weights (7 taps, 64
  filters, both, 3 taps): per-sample nfev equal to the reference run, both geometries."""
  for num_points in (64, 96):
    model = make_model('burgers', True, num_points=num_points, resample_factor=4, **overrides)
    assert model.kernel_name.startswith('mfma_f32')
    batch = 6
    y0 = (0.3 * random_phase_ic(model.equation, batch)).astype(np.float64)
    forcing = batch_forcing(batch)
    times = np.linspace(0.0, 0.1, 3)
    nfev, status, bad, worst = _check(model, y0, times, forcing, hip_samples=(0, 5))
    print(overrides, num_points, 'nfev', nfev, 'worst {:.1e}'.format(worst))
    assert not bad, bad
    assert (status == 0).all()


@pytest.mark.parametrize('equation,conservative,num_points,max_step', [
    ('burgers', True, 64, 0.01), ('burgers', False, 32, np.inf), ('kdv', True, 64, 0.01),
    ('ks', False, 16, np.inf), ('kdv', False, 8, np.inf)])
def test_small_ensembles_on_four_wavefronts_per_group(equation, conservative, num_points, max_step):
  """ddd_integrate_adaptive_f64 for a small ensemble runs every 64-row group on FOUR 16-row
  wavefronts (rhs_mfma.h kQuad, chosen automatically while that leaves at most two wavefronts
  per SIMD).  Right-hand side and error norm keep the one-wavefront kernel's operation order,
  so evaluation counts, status and trajectories are EQUAL to the forced one-wavefront
  geometry, bit for bit -- a sample's result does not depend on the ensemble around it."""
  batch = 23
  model = make_model(equation, conservative, num_points=num_points, resample_factor=4)
  scale = 0.4 if equation == 'burgers' else 1.0
  y0 = (scale * random_phase_ic(model.equation, batch)).astype(np.float64)
  forcing = batch_forcing(batch) if equation == 'burgers' else None
  model.set_forcing(forcing)
  times = np.array([0.0, 0.013, 0.1, 0.2])
  y, nfev, status = model.integrate_adaptive(y0, times, max_step=max_step)
  assert model.kernel_name == 'mfma_f32_r64w16'
  model.set_kernel('mfma64')
  y1, nfev1, status1 = model.integrate_adaptive(y0, times, max_step=max_step)
  assert model.kernel_name == 'mfma_f32_r64'
  np.testing.assert_array_equal(nfev.cpu().numpy(), nfev1.cpu().numpy())
  np.testing.assert_array_equal(status.cpu().numpy(), status1.cpu().numpy())
  np.testing.assert_array_equal(y.cpu().numpy(), y1.cpu().numpy())
  assert (status.cpu().numpy() == 0).all() and len(np.unique(nfev.cpu().numpy())) >= 1
  model.set_kernel('mfma64w16')
  y2, nfev2, _ = model.integrate_adaptive(y0, times, max_step=max_step)
  assert model.kernel_name == 'mfma_f32_r64w16'
  np.testing.assert_array_equal(y.cpu().numpy(), y2.cpu().numpy())
