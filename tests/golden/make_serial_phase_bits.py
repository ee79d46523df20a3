"""Record what a library computes for the cases of tests/serial_phase_cases.py.

Run on a GPU with the library of the commit whose bits are to be kept (the fixture in the
tree was written by the parent of the commit that rescheduled the one-wavefront
integrators' evaluation):

    python tests/golden/make_serial_phase_bits.py [--library path/to/libddd1d.so] [--out file]

Output: tests/golden/serial_phase_bits.npz -- per case the saved states (and the kernel's
name), for the adaptive case y, nfev and status.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
  ap = argparse.ArgumentParser(description=__doc__)
  ap.add_argument('--library', default=None)
  ap.add_argument('--out', default=os.path.join(HERE, 'serial_phase_bits.npz'))
  args = ap.parse_args()
  import helpers  # noqa: F401  (puts the package on the path)
  from ddd1d_amd import _lib
  _lib.load_library(args.library)
  import serial_phase_cases as cases
  out = {}
  for name in cases.CASES:
    out.update(cases.run_case(name))
  out.update(cases.run_adaptive())
  for key, value in out.items():
    if value.dtype.kind == 'f':
      print('{:32s} {} finite {:.0%}'.format(key, value.shape, np.isfinite(value).mean()))
    elif value.dtype.kind == 'U':
      print('{:32s} {}'.format(key, value))
  np.savez_compressed(args.out, **out)
  print('wrote', args.out, os.path.getsize(args.out), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
  main()
