"""The reference of test_gpu_spectral_kernels.py, kept honest without a GPU.

spectral_cases.trig_state differentiates a full-spectrum trigonometric polynomial term by term
in long double.  Here the host calls the reference uses -- scipy.fftpack.diff,
duckarray.spectral_derivative, oracle.spectral_time_derivative -- are held to it at
TOL64 / 4 = 2.5e-13 on every grid, equation and convention: four times inside the bound the
device is held to, so a device failure at TOL64 is the device's.  Largest distances seen on
the host: 7.3e-16 per derivative, 8.1e-16 per right-hand side, both at N = 2046 (DESIGN 5,
"Spectral kernels").
"""
import numpy as np
import pytest

import spectral_cases as sc
from ddd1d_amd import model as model_lib

HOST_TOL = sc.TOL64 / 4


@pytest.mark.parametrize('convention', sc.CONVENTIONS)
@pytest.mark.parametrize('cls_name', sc.EQUATIONS)
@pytest.mark.parametrize('n,mode', sc.GRIDS)
def test_host_reference_vs_trig_state(n, mode, cls_name, convention):
  eq = sc.make_equation(cls_name, n)
  spec = eq.kernel_spec()
  u, derivs, rhs = sc.batch_states(eq, convention)
  assert u.dtype == np.float64 and derivs.dtype == np.longdouble
  assert u.shape == (sc.BATCH, n) and derivs.shape == (sc.BATCH, n, len(spec['derivative_orders']))
  assert np.abs(u[0] - u[1]).max() > 0.1   # different samples
  for d, order in enumerate(spec['derivative_orders']):
    err = sc.rel_max(sc.host_derivative(convention, u, order, spec['period']), derivs[..., d])
    print(cls_name, n, convention, 'order', order, 'host/truth {:.2e}'.format(err))
    assert err < HOST_TOL, (order, err)
  err = sc.rel_max(sc.host_rhs(eq, convention, u), rhs)
  print(cls_name, n, convention, 'rhs host/truth {:.2e}'.format(err))
  assert err < HOST_TOL, err


@pytest.mark.parametrize('cls_name', ('KSEquation', 'BurgersEquation'))
@pytest.mark.parametrize('n,mode', sc.GRIDS)
def test_conventions_differ_on_these_states(n, mode, cls_name):
  """KS and Burgers have even-order derivatives: on a state with a Nyquist mode the two
  conventions' right-hand sides are far apart, in the truth and in the host calls alike.
  Without this the GPU test could not tell a model built with the other convention."""
  eq = sc.make_equation(cls_name, n)
  u, _, rhs_fftpack = sc.batch_states(eq, 'fftpack')
  u_rfft, _, rhs_rfft = sc.batch_states(eq, 'rfft')
  np.testing.assert_array_equal(u, u_rfft)   # the same states, two derivative rules
  for b in range(sc.BATCH):
    assert sc.rel_max(rhs_rfft[b], rhs_fftpack[b]) > 1e-3
    assert sc.rel_max(sc.host_rhs(eq, 'rfft', u[b]), sc.host_rhs(eq, 'fftpack', u[b])) > 1e-3


def test_kdv_conventions_agree():
  """KdV differentiates at odd orders only, where both conventions drop the Nyquist mode."""
  eq = sc.make_equation('KdVEquation', 64)
  _, _, rhs_fftpack = sc.batch_states(eq, 'fftpack')
  _, _, rhs_rfft = sc.batch_states(eq, 'rfft')
  np.testing.assert_array_equal(rhs_fftpack, rhs_rfft)


def test_nyquist_rule_of_each_convention():
  """cos(pi j) alone: fftpack returns 0 at every order; the rfft form 0 at odd orders and
  (-1)^(m/2) k^m cos(pi j) at even orders."""
  n, period = 64, 32.0
  x = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
  k = 2 * np.pi * (n // 2) / period
  for order in (1, 2, 3, 4):
    assert np.abs(sc.host_derivative('fftpack', x, order, period)).max() < 1e-9 * k ** order
    want = (-1) ** (order // 2) * k ** order * x if order % 2 == 0 else 0 * x
    np.testing.assert_allclose(sc.host_derivative('rfft', x, order, period), want,
                               rtol=0, atol=1e-12 * k ** order)


def test_trig_state_is_what_it_says():
  """The helper against a slow, literal evaluation of its formula at n = 16."""
  import math
  n, period, orders, seed = 16, 3.0, (1, 2, 4), 11
  u, derivs = sc.trig_state(n, period, orders, seed, True)
  _, derivs_dropped = sc.trig_state(n, period, orders, seed, False)
  rs = np.random.RandomState(seed)
  a = rs.uniform(-1.0, 1.0, size=n // 2)
  b = rs.uniform(-1.0, 1.0, size=n // 2)
  b[0] = 0.0
  for j in range(n):
    x = period * j / n
    want = sum(a[k] * math.cos(2 * math.pi * k * x / period) +
               b[k] * math.sin(2 * math.pi * k * x / period) for k in range(n // 2))
    want += 0.7 * (-1) ** j
    assert abs(u[j] - want) < 1e-13
    w = [2 * math.pi * k / period for k in range(n // 2)]
    # second derivative, with and without the Nyquist term
    d2 = sum(-w[k] ** 2 * (a[k] * math.cos(w[k] * x) + b[k] * math.sin(w[k] * x))
             for k in range(n // 2))
    nyq = -(2 * math.pi * (n // 2) / period) ** 2 * 0.7 * (-1) ** j
    assert abs(float(derivs[j, 1]) - (d2 + nyq)) < 1e-10
    assert abs(float(derivs_dropped[j, 1]) - d2) < 1e-10
    d1 = sum(w[k] * (-a[k] * math.sin(w[k] * x) + b[k] * math.cos(w[k] * x))
             for k in range(n // 2))
    assert abs(float(derivs[j, 0]) - d1) < 1e-11
  np.testing.assert_array_equal(derivs[:, 0], derivs_dropped[:, 0])


@pytest.mark.parametrize('n', (258, 512))
@pytest.mark.parametrize('scheme', ('euler', 'midpoint', 'bs3', 'rk4'))
def test_fixed_step_reference_does_not_depend_on_the_operator_form(scheme, n):
  """The reference of the GPU fixed-step test steps over the host FFT; the device applies
  circulant products (N = 258) or its own FFT (N = 512).  Seven steps over a float64
  circulant product of model.kernels stay within TOL64 / 4 of seven steps over the host FFT
  (largest seen: 2.8e-16), so the form of the operator is not what the GPU test measures."""
  eq, y0, dt = sc.fixed_step_case(n)
  model = model_lib.SpectralModel(eq)
  spec = eq.kernel_spec()

  def circulant_rhs(y):
    derivs = np.stack([sc.circulant_product(k, y) for k in model.kernels], axis=-1)
    return sc.oracle.equation_of_motion(spec['equation'], y, derivs, spec['eta'], spec['dx'])

  want = sc.step_fixed(lambda y: sc.host_rhs(eq, 'fftpack', y), scheme, y0, dt, 7, 3)
  got = sc.step_fixed(circulant_rhs, scheme, y0, dt, 7, 3)
  assert want.shape == (2, 3, n)
  assert np.abs(want).max() < 10 and np.abs(want[-1] - y0).max() > 1e-6   # O(1), and it moved
  err = sc.rel_max(got, want)
  print(scheme, n, 'circulant / FFT stepping {:.2e}'.format(err))
  assert err < HOST_TOL
