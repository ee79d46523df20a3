"""Full-spectrum states with exact derivatives, and the grids the spectral kernels branch on.

A plain module shared by test_cpu_spectral_cases.py and test_gpu_spectral_kernels.py (DESIGN 5,
"Spectral kernels").  trig_state is the reference of both: a trigonometric polynomial with
every wavenumber 0 .. n/2 present, evaluated and differentiated term by term in long double.
It shares nothing with the code under test -- no FFT, no impulse response, no circulant sum.

The two conventions of the spectral derivative differ at the Nyquist mode only:

  fftpack   scipy.fftpack.diff (integrate.SpectralDifferentiator): the Nyquist mode gives 0 at
            every order
  rfft      duckarray.spectral_derivative (model.baseline_space_derivatives): 0 at odd orders
            (irfft drops the imaginary part of the last bin), (-1)^(m/2) k^m cos(pi j) at even
            orders m -- the exact derivative of cos(k_N x) on the grid
"""
import functools

import numpy as np

from helpers import oracle, random_phase_ic
from ddd1d_amd import equations

# float64 kernels against the long-double truth, relative to the max norm of the truth.  The
# host calls the reference uses must stay four times inside it (test_cpu_spectral_cases.py).
# (test_gpu_exact_solvers.py holds the same kernels to 1e-9 of the host FFT on smooth states.)
TOL64 = 1e-12

# (num_points, mode): rhs_spectral.h runs 256 threads per sample; a power of two >= 512 runs
# the in-LDS FFT, every other even N <= 2048 the circulant products
GRIDS = (
    (64, 'circulant'),     # 192 idle threads
    (258, 'circulant'),    # the second trip owns two points
    (384, 'circulant'),    # kPts 2, half of the second trip masked
    (640, 'circulant'),    # above the FFT threshold; 3 points per thread -> kPts 4
    (1280, 'circulant'),   # 5 points per thread -> kPts 8
    (2046, 'circulant'),   # largest circulant grid; KS needs > 64 KB of LDS
    (512, 'fft'),          # 9 stages
    (1024, 'fft'),         # 10 stages
    (2048, 'fft'),         # 11 stages
)
EQUATIONS = ('KdVEquation', 'KSEquation', 'BurgersEquation')
CONVENTIONS = ('fftpack', 'rfft')
NYQUIST_AMPLITUDE = 0.7
BATCH = 3


def make_equation(cls_name, n):
  return getattr(equations, cls_name)(n, random_seed=3)


@functools.lru_cache(maxsize=None)
def _trig_tables(n):
  """cos and sin of 2 pi r / n, r < n, in long double with a long-double pi."""
  pi = 4 * np.arctan(np.longdouble(1))
  theta = 2 * pi * np.arange(n).astype(np.longdouble) / np.longdouble(n)
  return np.cos(theta), np.sin(theta)


@functools.lru_cache(maxsize=None)
def _trig_state(n, period, orders, seed, nyquist_in_even_orders):
  if n % 2:
    raise ValueError('even n only')
  half = n // 2
  rs = np.random.RandomState(seed)
  a = rs.uniform(-1.0, 1.0, size=half)
  b = rs.uniform(-1.0, 1.0, size=half)
  b[0] = 0.0
  # theta_jk = 2 pi ((j k) mod n) / n: reduced in integers before any rounding
  r = (np.arange(n, dtype=np.int64)[:, None] * np.arange(half, dtype=np.int64)[None, :]) % n
  cos_table, sin_table = _trig_tables(n)
  cos_jk, sin_jk = cos_table[r], sin_table[r]
  a_l, b_l = a.astype(np.longdouble), b.astype(np.longdouble)
  sign = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.longdouble)   # cos(pi j)
  c = np.longdouble(NYQUIST_AMPLITUDE)
  u = (cos_jk @ a_l + sin_jk @ b_l + c * sign).astype(np.float64)
  pi = 4 * np.arctan(np.longdouble(1))
  w = 2 * pi * np.arange(half).astype(np.longdouble) / np.longdouble(period)
  w_nyquist = 2 * pi * np.longdouble(half) / np.longdouble(period)
  derivs = []
  for m in orders:
    wm = w ** m
    # d^m/dx^m (a cos + b sin): the four-cycle of cos -> -sin -> -cos -> sin
    ca, cb = ((a_l, b_l), (b_l, -a_l), (-a_l, -b_l), (-b_l, a_l))[m % 4]
    d = cos_jk @ (wm * ca) + sin_jk @ (wm * cb)
    if nyquist_in_even_orders and m % 2 == 0:
      d = d + (-1) ** (m // 2) * w_nyquist ** m * c * sign
    derivs.append(d)
  u.setflags(write=False)
  derivs = np.stack(derivs, axis=-1)
  derivs.setflags(write=False)
  return u, derivs


def trig_state(n, period, orders, seed, nyquist_in_even_orders):
  """u [n] float64 and its derivatives [n, len(orders)] in long double.

  u(x_j) = sum_{k < n/2} a_k cos(theta_jk) + b_k sin(theta_jk) + 0.7 cos(pi j), a_k and b_k
  uniform in [-1, 1] (RandomState(seed)), b_0 = 0.  u is the long-double sum rounded to
  float64; the derivatives are those of the coefficients, term by term with
  (2 pi k / period)^m, NOT those of the rounded u.  The Nyquist term enters the even-order
  derivatives when nyquist_in_even_orders (the rfft convention) and none otherwise (fftpack).
  Cached: the arrays are read-only."""
  return _trig_state(int(n), float(period), tuple(int(m) for m in orders), int(seed),
                     bool(nyquist_in_even_orders))


def rhs_truth(eq, u, derivs):
  """oracle.equation_of_motion in long double over exact derivatives, cast to float64."""
  spec = eq.kernel_spec()
  out = oracle.equation_of_motion(spec['equation'], np.asarray(u).astype(np.longdouble),
                                  np.asarray(derivs, dtype=np.longdouble),
                                  spec['eta'], spec['dx'])
  assert out.dtype == np.longdouble
  return out.astype(np.float64)


def batch_states(eq, convention, batch=BATCH, seed0=4100):
  """(u [batch, n] float64, derivs [batch, n, D] long double, rhs [batch, n] float64) of
  `batch` different trig_state samples for this equation and convention."""
  spec = eq.kernel_spec()
  n = spec['num_points']
  pairs = [trig_state(n, spec['period'], spec['derivative_orders'], seed0 + 13 * i + n,
                      convention == 'rfft') for i in range(batch)]
  u = np.stack([p[0] for p in pairs])
  derivs = np.stack([p[1] for p in pairs])
  rhs = np.stack([rhs_truth(eq, p[0], p[1]) for p in pairs])
  return u, derivs, rhs


def host_derivative(convention, u, order, period):
  """The host call of each convention, as the reference makes it, on rows of u."""
  if convention == 'fftpack':
    import scipy.fftpack
    rows = np.asarray(u).reshape(-1, np.shape(u)[-1])
    return np.stack([scipy.fftpack.diff(row, order, period) for row in rows]).reshape(np.shape(u))
  from ddd1d_amd import duckarray
  return duckarray.spectral_derivative(u, order, period)


def host_rhs(eq, convention, u):
  """The right-hand side the GPU tests have always compared with: SciPy / NumPy FFTs."""
  spec = eq.kernel_spec()
  if convention == 'fftpack':
    return oracle.spectral_time_derivative(spec['equation'], u, spec['derivative_orders'],
                                           spec['period'], spec['eta'], spec['dx'])
  derivs = np.stack([host_derivative('rfft', u, order, spec['period'])
                     for order in spec['derivative_orders']], axis=-1)
  return oracle.equation_of_motion(spec['equation'], np.asarray(u, dtype=np.float64), derivs,
                                   spec['eta'], spec['dx'])


def rel_max(got, want):
  """max |got - want| / max |want| per row of the leading axis, in long double; the largest."""
  got = np.asarray(got, dtype=np.longdouble)
  want = np.asarray(want, dtype=np.longdouble)
  got = got.reshape(got.shape[0], -1) if got.ndim > 1 else got[None]
  want = want.reshape(want.shape[0], -1) if want.ndim > 1 else want[None]
  return float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())


def circulant_product(kernel, x, dtype=np.float64):
  """out[..., i] = sum_j kernel[(i - j) mod n] x[..., j] as a dense matrix product in `dtype`."""
  kernel = np.asarray(kernel, dtype=dtype)
  n = kernel.shape[0]
  idx = (np.arange(n)[:, None] - np.arange(n)[None, :]) % n
  return np.asarray(x, dtype=dtype) @ kernel[idx].T


# -- fixed-step stepping in NumPy float64, in the order ddd_integrate_fixed_f64 applies it ----
TABLEAUS = {
    'euler': ((), (1.0,)),
    'midpoint': ((0.5,), (0.0, 1.0)),
    'bs3': ((0.5, 0.75), (2.0 / 9.0, 1.0 / 3.0, 4.0 / 9.0)),
    'rk4': ((0.5, 0.5, 1.0), (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)),
}


def step_fixed(rhs, scheme, y0, dt, num_steps, save_every):
  """Explicit RK steps of the scheme's Butcher tableau over rhs(y); rows every save_every."""
  a, b = TABLEAUS[scheme]
  y = np.array(y0, dtype=np.float64)
  rows = []
  for step in range(num_steps):
    stage, acc = y, y
    for s in range(len(b)):
      f = rhs(stage)
      if s + 1 < len(b):
        stage = y + (a[s] * dt) * f
      if b[s] != 0.0:
        acc = acc + (b[s] * dt) * f
    y = acc
    if (step + 1) % save_every == 0:
      rows.append(y.copy())
  return np.stack(rows) if rows else np.zeros((0,) + y.shape)


def fixed_step_case(n):
  """(equation, y0 [3, n], dt) of the fixed-step tests: a smooth KdV state plus 1e-3 x a
  full-spectrum one, dt k_max^3 = 0.1."""
  eq = make_equation('KdVEquation', n)
  spec = eq.kernel_spec()
  full, _, _ = batch_states(eq, 'fftpack')
  y0 = random_phase_ic(eq, BATCH).astype(np.float64) + 1e-3 * full
  kmax = 2 * np.pi * (n // 2) / spec['period']
  return eq, y0, 0.1 / kmax ** 3
