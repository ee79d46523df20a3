"""The one-wavefront integrators keep their bits when an evaluation's serial stretch is shortened.

The relu results in registers of their own, the input layer's permutes requested together and
the forcing phases / epilogue reads issued inside the matrix streams change WHEN an operation
is issued, never its operands or its place in its chain: every saved state must equal, bit
for bit, what the library computed before those changes (tests/golden/serial_phase_bits.npz,
written by tests/golden/make_serial_phase_bits.py with the parent commit's library; the cases:
tests/serial_phase_cases.py)."""
import os

import numpy as np
import pytest

import serial_phase_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                              'serial_phase_bits.npz'))


def test_the_fixture_covers_every_case():
  keys = {name + '/y' for name in cases.CASES} | {'adaptive/y', 'adaptive/nfev', 'adaptive/status'}
  assert keys <= set(GOLDEN.files)


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_fixed_step_bits(name):
  got = cases.run_case(name)
  case = cases.CASES[name]
  want = GOLDEN[name + '/y']
  assert str(got[name + '/kernel']) == str(GOLDEN[name + '/kernel'])
  assert got[name + '/y'].dtype == want.dtype and got[name + '/y'].shape == want.shape
  assert want.shape[0] == case['steps'] // case['save_every']
  # (assert_array_equal takes NaNs in the same places for equal)
  np.testing.assert_array_equal(got[name + '/y'], want)
  if case['nan_at'] is None:
    assert np.isfinite(want).all()
  else:
    # the seeded sample diverges as before; its partner in the wavefront never sees the NaN
    sample = case['nan_at'][0]
    assert np.isnan(want[:, sample]).any()
    assert np.isfinite(np.delete(want, sample, axis=1)).all()
    np.testing.assert_array_equal(np.delete(got[name + '/y'], sample, axis=1),
                                  np.delete(want, sample, axis=1))


def test_one_wavefront_kernels_are_the_ones_under_test():
  names = {str(GOLDEN[name + '/kernel']) for name in cases.CASES}
  assert 'mfma_f32_r64' in names, names


def test_adaptive_bits():
  got = cases.run_adaptive()
  assert str(got['adaptive/kernel']) == str(GOLDEN['adaptive/kernel'])
  np.testing.assert_array_equal(got['adaptive/y'], GOLDEN['adaptive/y'])
  np.testing.assert_array_equal(got['adaptive/nfev'], GOLDEN['adaptive/nfev'])
  np.testing.assert_array_equal(got['adaptive/status'], GOLDEN['adaptive/status'])
  assert (GOLDEN['adaptive/status'] == 0).all() and (GOLDEN['adaptive/nfev'] > 0).all()
