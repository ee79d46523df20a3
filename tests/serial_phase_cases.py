"""Cases whose bits the one-wavefront integrators must keep when their evaluation is rescheduled.

A plain module shared by tests/golden/make_serial_phase_bits.py (which records what a library
computes for every case) and tests/test_gpu_serial_phase.py (which holds the current library
to the recorded bits).  Every case forces the 64-row one-wavefront kernels (`mfma64`) and
stays at <= 16 steps and <= 8 samples.

  geometry   N = 64: one sample per wavefront; N = 32, batch 3: two per wavefront, the last
             group half empty; N = 16, batch 5: four per wavefront, where the lanes of forcing
             phase 1 serve other samples than their own
  forcing    tests/forcing_cases.py: `one` (1 mode), `planted` (runs of 8 and 9 modes on one
             wavenumber: the second trip of phase 2), `run20` (20 modes on one wavenumber: the
             third trip), `six` (20 modes over 6 wavenumbers, the benchmark's shape), `edge` at
             N = 16 (samples x modes = 64 exactly), and the unforced model
  equations  both Burgers forms, flux-form KdV, plain KS
  scheme     euler, midpoint, bs3, rk4; float32 and float64 state; save_every 3 of 7 steps (the
             next evaluation's time across a snapshot); t0 != 0
  adaptive   integrate_adaptive on Burgers, batch 4, a short horizon: y, nfev, status
  nan        one NaN seeded in one sample of an N = 32 pair
"""
import functools

import numpy as np

import forcing_cases as fc
from helpers import make_model, random_phase_ic

KERNEL = 'mfma64'
RESAMPLE = {64: 4, 32: 8, 16: 1}


def _case(equation='burgers', conservative=True, n=64, batch=3, forcing='six', scheme='midpoint',
          steps=4, save_every=None, dtype='float32', t0=0.0, nan_at=None):
  return dict(equation=equation, conservative=conservative, n=n, batch=batch, forcing=forcing,
              scheme=scheme, steps=steps, save_every=save_every or steps, dtype=dtype, t0=t0,
              nan_at=nan_at)


CASES = {
    # geometry x the benchmark's table
    'n64_six': _case(n=64, batch=3),
    'n32_six': _case(n=32, batch=3),
    'n16_six': _case(n=16, batch=5),
    # forcing tables
    'n64_one': _case(n=64, forcing='one'),
    'n16_one': _case(n=16, batch=5, forcing='one'),
    'n64_planted': _case(n=64, forcing='planted'),
    'n16_planted': _case(n=16, batch=5, forcing='planted'),
    'n64_run20': _case(n=64, batch=5, forcing='run20'),
    'n32_run20': _case(n=32, batch=5, forcing='run20'),
    'n16_edge': _case(n=16, batch=5, forcing='edge'),
    'n64_unforced': _case(n=64, forcing=None),
    'n32_unforced': _case(n=32, forcing=None),
    # equations
    'plain_burgers_n64': _case(conservative=False, n=64),
    'plain_burgers_n16_run9': _case(conservative=False, n=16, batch=5, forcing='planted'),
    'kdv_n64': _case(equation='kdv', n=64, forcing=None),
    'kdv_n32_bs3': _case(equation='kdv', n=32, forcing=None, scheme='bs3'),
    'ks_n64': _case(equation='ks', conservative=False, n=64, forcing=None),
    # scheme and state
    'euler': _case(n=32, scheme='euler', steps=5),
    'bs3': _case(n=32, scheme='bs3', steps=3),
    'rk4': _case(n=32, scheme='rk4', steps=3),
    'rk4_plain_n64': _case(conservative=False, n=64, scheme='rk4', steps=2),
    'f64_n64': _case(n=64, dtype='float64'),
    'f64_n16': _case(n=16, batch=5, dtype='float64', forcing='planted'),
    'f64_kdv': _case(equation='kdv', n=64, forcing=None, dtype='float64'),
    'snapshots': _case(n=32, steps=7, save_every=3, t0=1.7),
    'snapshots_f64_n16': _case(n=16, batch=5, steps=7, save_every=3, t0=1.7, dtype='float64'),
    'snapshots_rk4_n64': _case(n=64, steps=7, save_every=3, t0=47.0, scheme='rk4',
                               forcing='run20', batch=5),
    # NaN through relu: sample 1 of the pair diverges, sample 0 shares its wavefront
    'nan_pair': _case(n=32, batch=2, steps=3, save_every=1, nan_at=(1, 5)),
}
ADAPTIVE = dict(n=64, batch=4, forcing='six', times=(0.0, 0.02, 0.05))


@functools.lru_cache(maxsize=None)
def model_for(equation, conservative, n):
  model = make_model(equation, conservative, num_points=n, resample_factor=RESAMPLE[n])
  model.set_kernel(KERNEL)
  return model


def _prepare(equation, conservative, n, batch, forcing):
  model = model_for(equation, conservative, n)
  model.set_forcing(None if forcing is None else fc.draw(forcing, batch, n))
  return model, random_phase_ic(model.equation, batch)


def run_case(name):
  """{key: array} of what the loaded library computes for CASES[name]."""
  c = CASES[name]
  model, y0 = _prepare(c['equation'], c['conservative'], c['n'], c['batch'], c['forcing'])
  if c['nan_at'] is not None:
    y0[c['nan_at']] = np.nan
  y0 = y0.astype(np.float64 if c['dtype'] == 'float64' else np.float32)
  y = model.integrate_fixed(y0, c['steps'], t0=c['t0'], scheme=c['scheme'],
                            save_every=c['save_every'], state_dtype=c['dtype'])
  return {name + '/y': y.cpu().numpy(),
          name + '/kernel': np.array(model.kernel_name)}


def run_adaptive():
  a = ADAPTIVE
  model, y0 = _prepare('burgers', True, a['n'], a['batch'], a['forcing'])
  y, nfev, status = model.integrate_adaptive(y0.astype(np.float64), np.array(a['times']))
  return {'adaptive/y': y.cpu().numpy(), 'adaptive/nfev': nfev.cpu().numpy(),
          'adaptive/status': status.cpu().numpy(),
          'adaptive/kernel': np.array(model.kernel_name)}
