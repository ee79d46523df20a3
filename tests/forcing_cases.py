"""Forcing tables of every shape the device code branches on, and the bound they are held to.

A plain module shared by test_cpu_forcing_tables.py and test_gpu_forcing_tables.py (DESIGN 5,
"Forcing tables").  Every table is a synthetic draw with a fixed seed: amplitudes uniform in
+-[0.1, 0.5] -- a dropped or mis-paired mode moves the result by at least 0.1 somewhere on the
grid --, omega in [-0.4, 0.4] and phi in [0, 2 pi) as RandomForcing draws them.

A *shape* is (P, set of k); which branch it reaches depends on the grid:

  one          P = 1,  k = {1}                       n_k = 1
  two          P = 3,  k = {-1, 1}                   n_k = 2
  two7         P = 7,  k = {-1, 1}                   n_k = 2 (the adaptive case)
  four         P = 20, k = {-2, -1, 1, 2}            n_k = 4: last value of the LDS-padding branch
  five         P = 20, k = {-2, -1, 0, 1, 2}         n_k = 5: a constant mode, the global table
  six          P = 20, k = +-{1, 2, 3}               the suite's usual table (control)
  eight        P = 20, k = +-{1, 2, 3, 4}            n_k = 8: not fast
  run20        P = 20, k = {2} for samples 1, 4, 7, ..; {-3, 3} for the others
                                                     a run of 20 (three trips) next to empty runs
  planted      P = 17, 8 modes of k = 1 and 9 of k = 2, interleaved
                                                     runs of exactly 8 and 9; the host's sort
  edge, over   P = rows / spg and one more, k = +-{1, 2, 3}
                                                     the `spg P <= rows` edge and one past it
  p255, p256   P = 255, 256, k = +-{1, 2, 3}         `P < 256`, the unsigned char runs
  p<n>         P = n, k = +-{1, 2, 3}                 (p64, p65: the WENO kernels' edge)
"""
import numpy as np

TIMES = (0.0, 3.3, 47.0)

# (num_points, resample_factor, flux form): the four grids of the CPU tier
CPU_GRIDS = ((64, 4, True), (32, 8, False), (128, 2, True), (16, 1, False))

_K_SETS = {
    'one': (1, (1,)),
    'two': (3, (-1, 1)),
    'two7': (7, (-1, 1)),
    'four': (20, (-2, -1, 1, 2)),
    'five': (20, (-2, -1, 0, 1, 2)),
    'six': (20, (-3, -2, -1, 1, 2, 3)),
    'eight': (20, (-4, -3, -2, -1, 1, 2, 3, 4)),
}
COMMON_SHAPES = ('one', 'two', 'two7', 'four', 'five', 'six', 'eight', 'run20', 'planted')
_SEEDS = {name: 7100 + 17 * i for i, name in enumerate(
    COMMON_SHAPES + ('edge', 'over', 'p255', 'p256'))}


def edge_modes(num_points):
  """Largest P of the harmonic-sum form on an N-point grid: samples-per-group x P <= rows, in the
  64-row geometry where N divides 64 (the same P in the 256-row one: both scale by 4), else in
  the 256-row geometry."""
  if num_points <= 64 and 64 % num_points == 0:
    return num_points
  return 256 // (256 // num_points)


def shapes_for(num_points):
  """Names of the shapes that belong to an N-point grid (the issue's table)."""
  names = COMMON_SHAPES + ('edge', 'over')
  if num_points >= 128:
    names = names + ('p255', 'p256')
  return names


def num_modes(name, num_points):
  if name in _K_SETS:
    return _K_SETS[name][0]
  if name[0] == 'p' and name[1:].isdigit():   # 'p65': P = 65, k = +-{1, 2, 3}
    return int(name[1:])
  return {'run20': 20, 'planted': 17, 'edge': edge_modes(num_points),
          'over': edge_modes(num_points) + 1}[name]


def draw(name, batch, num_points):
  """dict a / omega / k / phi, each [batch, P] (float64, k int64), for shape `name`."""
  nparams = num_modes(name, num_points)
  rs = np.random.RandomState(_SEEDS.get(name, 7000) + 1000 * nparams)
  shape = (batch, nparams)
  sign = rs.choice([-1.0, 1.0], size=shape)
  out = dict(a=sign * rs.uniform(0.1, 0.5, size=shape),
             omega=rs.uniform(-0.4, 0.4, size=shape),
             phi=rs.uniform(0, 2 * np.pi, size=shape))
  if name == 'run20':
    k = rs.choice([-3, 3], size=shape)
    k[:, 0], k[:, 1] = -3, 3            # both of the other samples' runs are non-empty
    k[1::3] = 2
  elif name == 'planted':
    row = np.array([1] * 8 + [2] * 9)
    k = np.stack([rs.permutation(row) for _ in range(batch)])
  else:
    values = _K_SETS.get(name, (None, (-3, -2, -1, 1, 2, 3)))[1]
    k = rs.choice(values, size=shape)
    if nparams >= len(values):          # every wavenumber occurs: n_k is what the name says
      k[0, :len(values)] = values
  out['k'] = k.astype(np.int64)
  return out


def wavenumber_count(forcing):
  return int(np.unique(forcing['k']).size)


def is_fast(forcing, num_points, rows):
  """rhs_mfma.h forcing_is_fast, restated: the harmonic-sum form carries this table in a
  `rows`-row group.  (samples x 12 sums <= 3 rows / 4 holds for every N >= 16.)"""
  spg = rows // num_points
  nparams = forcing['k'].shape[1]
  return (spg * nparams <= rows and wavenumber_count(forcing) <= 6 and
          spg * 12 <= 3 * rows // 4 and nparams < 256)


def lean_supports(forcing, num_points):
  """rhs_lean.h supports(), the forcing clause."""
  spw = 64 // num_points
  nparams, n_k = forcing['k'].shape[1], wavenumber_count(forcing)
  return spw * nparams <= 64 and nparams < 256 and n_k <= 6 and spw * n_k * 2 <= 64


def weno_supports(forcing):
  """rhs_weno.h supports(), the forcing clause."""
  return forcing['k'].shape[1] <= 64 and wavenumber_count(forcing) <= 6


def bound(forcing, t):
  """Per-sample bound [batch] on |float32 evaluation - float64 truth| of the forcing at time t:

    B = sum_j |a_j| (8 2^-24 Phi_j + 2^-21) + P 2^-24 sum_j |a_j|,
    Phi_j = |omega_j t| + 2 pi |k_j| + |phi_j| + pi.

  Phi_j bounds every intermediate of mode j's phase in either order of evaluation (omega t, the
  spatial phase below 2 pi |k|, phi, the resample shift below pi).  Three float32 roundings of
  the table inputs (omega, phi or phi + shift, the spatial phase) and three of the phase
  arithmetic move the phase by at most 6 x 2^-24 Phi_j; 8 leaves two for the resample shift
  evaluated in float32.  |sin'| <= 1 turns that into the same absolute error of the sine;
  2^-21 = 8 ulp(1) covers sin / cos to a few ulp, the rounding of a and of the products
  a sin, (a sin) cos.  The last term is one rounding per term of the P-term sum, each partial sum
  being at most sum |a_j|."""
  a = np.abs(np.asarray(forcing['a'], dtype=np.float64))
  phi_j = (np.abs(np.asarray(forcing['omega']) * t) + 2 * np.pi * np.abs(forcing['k'])
           + np.abs(forcing['phi']) + np.pi)
  nparams = a.shape[1]
  return (np.sum(a * (8 * 2.0 ** -24 * phi_j + 2.0 ** -21), axis=1)
          + nparams * 2.0 ** -24 * np.sum(a, axis=1))


def host_runs(k_index):
  """The `runs` rows ddd_set_forcing builds, restated: per sample 8 entries, runs[kk] = first
  mode, after a stable sort by k index, whose index is >= kk.  Returns (order [batch, P], the
  sort permutation, and runs [batch, 8] int)."""
  k_index = np.asarray(k_index)
  order = np.argsort(k_index, axis=1, kind='stable')
  sorted_k = np.take_along_axis(k_index, order, axis=1)
  runs = np.zeros((k_index.shape[0], 8), dtype=np.int64)
  for b in range(k_index.shape[0]):
    mode = 0
    for kk in range(8):
      while mode < sorted_k.shape[1] and sorted_k[b, mode] < kk:
        mode += 1
      runs[b, kk] = mode
  return order, runs


def harmonic_sum_f32(tables, t):
  """NumPy float32 emulation of the device's harmonic-sum form from the tables
  model.forcing_kernel_tables hands ddd_set_forcing:

    psi = RN(RN(omega t) + phi'),  s_j = a_j sin psi,  c_j = a_j cos psi       (phase 1)
    S_k = sum of s_j, C_k = sum of c_j over the modes with wavenumber index k, in mode order
          after a stable sort by k index                                        (phase 2)
    f(x) = sum_k S_k (float)cos theta_k(x) + C_k (float)sin theta_k(x)          (phase 3)

  with theta the float32 spatial phase table.  Returns float32 [batch, N].  The `runs` rows
  are asserted on the way: they are what the kernels' sums are sliced by."""
  f32 = np.float32
  amp, omega, phase = (np.asarray(tables[key], dtype=f32)
                       for key in ('amplitude', 'omega', 'phase'))
  k_index = np.asarray(tables['k_index'])
  spatial = np.asarray(tables['spatial_phase'], dtype=f32)
  batch, nparams = amp.shape
  n_k = spatial.shape[0]
  order, runs = host_runs(k_index)
  sorted_k = np.take_along_axis(k_index, order, axis=1)
  assert (runs[:, 0] == 0).all() and (np.diff(runs, axis=1) >= 0).all()
  assert (runs[:, min(n_k, 8):] == nparams).all()
  for b in range(batch):   # first sorted mode with index >= kk, 8 entries
    assert (runs[b] == np.searchsorted(sorted_k[b], np.arange(8), side='left')).all()
  if nparams < 256:
    assert runs.max() <= 255   # unsigned char
  psi = (omega * f32(t)).astype(f32) + phase
  assert psi.dtype == f32
  s = np.take_along_axis(amp * np.sin(psi), order, axis=1)
  c = np.take_along_axis(amp * np.cos(psi), order, axis=1)
  assert s.dtype == f32 and c.dtype == f32
  cos_t = np.cos(spatial.astype(np.float64)).astype(f32)
  sin_t = np.sin(spatial.astype(np.float64)).astype(f32)
  out = np.zeros((batch, spatial.shape[1]), dtype=f32)
  for b in range(batch):
    for kk in range(n_k):
      lo = runs[b, kk] if kk < 8 else nparams
      hi = runs[b, kk + 1] if kk + 1 < 8 else nparams
      assert (sorted_k[b, lo:hi] == kk).all() and (hi - lo) == (k_index[b] == kk).sum()
      big_s, big_c = f32(0), f32(0)
      for m in range(lo, hi):
        big_s = f32(big_s + s[b, m])
        big_c = f32(big_c + c[b, m])
      out[b] = out[b] + big_s * cos_t[kk]
      out[b] = out[b] + big_c * sin_t[kk]
  return out
