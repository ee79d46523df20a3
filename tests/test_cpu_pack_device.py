"""The device packer of the population's weights without a GPU.

csrc/pack_device.h's slot functions -- the statements the kernel of csrc/pack_device.hip
runs, one output float each -- are compiled by g++ (tests/pack_device_harness.cpp),
evaluated over every output index and compared, bit for bit, with what ddd_model_create
uploads for the same values: csrc/pack_weights.h through oracle/libpackhost.so (pack_net
of test_cpu_mfma_emulation).  Then the two new entry points' refusals that come before any
device work."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from test_cpu_mfma_emulation import pack_net
from ddd1d_amd import _lib

HARNESS = os.path.join(ROOT, 'tests', 'pack_device_harness.cpp')
ERR_INVALID_ARGUMENT = -1
BUFFERS = ('w_input', 'w_hidden', 'w_final4')

# (derivatives' null-space split, stencil points, folded) of the six per-equation kernels
# (rhs_mfma.h: spec_in_size, spec_stencil, spec_folded)
EQUATIONS = {
    'burgers_flux': ((5, 4), 6, True), 'burgers': ((5, 4), 7, False),
    'kdv_flux': ((5, 3), 6, False), 'kdv': ((5, 3), 7, False),
    'ks_flux': ((5, 4, 2), 6, False), 'ks': ((5, 4, 2), 7, False)}


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
  """The harness as a shared object (for ctypes) and as a program (its own main)."""
  tmp = tmp_path_factory.mktemp('pack_device')
  shared, program = str(tmp / 'libpackdevice.so'), str(tmp / 'pack_device_harness')
  common = ['g++', '-std=c++17', '-O1', HARNESS]
  subprocess.run(common + ['-shared', '-fPIC', '-o', shared], check=True)
  subprocess.run(common + ['-o', program], check=True)
  return ctypes.CDLL(shared), program


def _net(rs, taps, filters, split, scale=0.3):
  shapes = [(taps, 1, filters), (taps, filters, filters), (taps, filters, sum(split))]
  kernels = [(scale * rs.standard_normal(s)).astype(np.float32) for s in shapes]
  biases = [(0.1 * rs.standard_normal(s[2])).astype(np.float32) for s in shapes]
  return kernels, biases


def _tables(rs, split, points):
  nullspaces = [rs.standard_normal((size, points)).astype(np.float32) for size in split]
  acc_biases = [rs.standard_normal(points).astype(np.float32) for _ in split]
  return nullspaces, acc_biases


def _bits(values):
  return np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)


def _device_pack(lib, kernels, biases, split, points, nullspaces, acc_biases, fin4_groups,
                 spec_folded):
  """The three arrays from the slot functions of csrc/pack_device.h."""
  sizes = np.zeros(3, np.int32)
  iptr, fptr = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
  lib.pack_device_sizes(sizes.ctypes.data_as(iptr))
  cfg = np.array([kernels[0].shape[0], kernels[0].shape[2], sum(split), len(split), points,
                  fin4_groups, spec_folded], np.int32)
  in_start = np.array([sum(split[:d]) for d in range(len(split))] + [0] * (4 - len(split)),
                      np.int32)
  in_size = np.array(list(split) + [0] * (4 - len(split)), np.int32)
  ns8, bias8 = np.zeros((24, 12), np.float32), np.zeros((4, 12), np.float32)
  for d, (ns, acc) in enumerate(zip(nullspaces, acc_biases)):
    ns8[in_start[d]:in_start[d] + in_size[d], :points] = ns
    bias8[d, :points] = acc
  flat = np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in zip(kernels, biases)])
  # (prefilled: every element must be written, whatever the buffers held)
  out = [np.full(int(n), np.nan, np.float32) for n in sizes]
  count = lib.pack_device_host(
      cfg.ctypes.data_as(iptr), flat.ctypes.data_as(fptr), in_start.ctypes.data_as(iptr),
      in_size.ctypes.data_as(iptr), ns8.ctypes.data_as(fptr), bias8.ctypes.data_as(fptr),
      *[o.ctypes.data_as(fptr) for o in out])
  assert count == sizes.sum()
  return dict(zip(BUFFERS, out))


def _assert_same_bits(lib, kernels, biases, split, points, nullspaces, acc_biases, folded):
  host = pack_net(kernels, biases, coefficients=(points, nullspaces, acc_biases))
  assert bool(host['spec_folded']) == folded
  got = _device_pack(lib, kernels, biases, split, points, nullspaces, acc_biases,
                     host['fin4_groups'], host['spec_folded'])
  for name in BUFFERS:
    want = host[name].astype(np.float32)   # (pack_net's float64 copies: exact both ways)
    assert got[name].shape == want.shape, name
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got[name]), nan, err_msg=name)
    np.testing.assert_array_equal(_bits(got[name])[~nan], _bits(want)[~nan], err_msg=name)
  return got, host


def test_harness_program_agrees_with_the_host_packer(harness):
  """The harness's own main: pack_weights.h against the slot functions in one program (the
  form a host-sanitizer build runs)."""
  done = subprocess.run([harness[1]], capture_output=True, text=True)
  assert done.returncode == 0, done.stdout + done.stderr
  assert done.stdout.count(': 0 floats differ') == 18


@pytest.mark.parametrize('equation', sorted(EQUATIONS))
def test_every_per_equation_shape(harness, equation):
  split, points, folded = EQUATIONS[equation]
  rs = np.random.RandomState(len(equation) + points)
  kernels, biases = _net(rs, 5, 32, split)
  nullspaces, acc_biases = _tables(rs, split, points)
  got, _ = _assert_same_bits(harness[0], kernels, biases, split, points, nullspaces,
                             acc_biases, folded)
  assert all(np.isfinite(buf).all() and np.any(buf != 0) for buf in got.values())


@pytest.mark.parametrize('taps,filters', [(4, 32), (5, 17), (5, 31), (4, 24)])
@pytest.mark.parametrize('equation', ['burgers_flux', 'ks'])
def test_nets_embedded_in_the_default_tower(harness, equation, taps, filters):
  """What plan_population admits beside the default net: 4 or 5 taps and 17 .. 32 filters
  ride the 5 x 32 tower as their zero-padded embedding (up to 3 taps: the 3-tap tower; up
  to 16 filters: the 16-channel tiles -- neither has a population kernel)."""
  split, points, folded = EQUATIONS[equation]
  rs = np.random.RandomState(100 * taps + filters)
  kernels, biases = _net(rs, taps, filters, split)
  nullspaces, acc_biases = _tables(rs, split, points)
  _assert_same_bits(harness[0], kernels, biases, split, points, nullspaces, acc_biases, folded)


@pytest.mark.parametrize('equation', ['burgers_flux', 'kdv'])
def test_signed_zeros_denormals_and_non_finite_values(harness, equation):
  split, points, folded = EQUATIONS[equation]
  rs = np.random.RandomState(7)
  kernels, biases = _net(rs, 5, 32, split)
  nullspaces, acc_biases = _tables(rs, split, points)
  specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-20, -1e-20], np.float32)
  for w in kernels:
    flat = w.reshape(-1)
    flat[::5] = specials[np.arange(flat[::5].size) % specials.size]
  for b in biases:
    b[0], b[1], b[2] = 1e-20, -0.0, -1e-20   # 1e-20 x 2^-64: a float32 denormal
  got, host = _assert_same_bits(harness[0], kernels, biases, split, points, nullspaces,
                                acc_biases, folded)
  tiny = np.float32(1e-20) * np.float32(2.0 ** -64)
  assert 0 < tiny < np.finfo(np.float32).tiny   # (kept, not flushed)
  for name in ('w_input', 'w_hidden'):
    assert np.any(got[name] == tiny) and np.any(got[name] == -tiny), name
    assert np.any(_bits(got[name]) == 0x80000000), name   # a -0.0 arrived as -0.0
  assert np.isnan(got['w_final4']).any() and np.isinf(got['w_final4']).any()


def test_result_does_not_depend_on_the_weights_beyond_the_net(harness):
  """An embedded net reads its own n_weights floats and no more: the same arrays from a
  vector followed by garbage."""
  split, points, folded = EQUATIONS['kdv_flux']
  rs = np.random.RandomState(3)
  kernels, biases = _net(rs, 4, 20, split)
  nullspaces, acc_biases = _tables(rs, split, points)
  got, _ = _assert_same_bits(harness[0], kernels, biases, split, points, nullspaces,
                             acc_biases, folded)
  padded = [b.copy() for b in biases]
  padded[-1] = np.concatenate([padded[-1], np.full(64, np.nan, np.float32)])
  again = _device_pack(harness[0], kernels, padded, split, points, nullspaces, acc_biases, 2, 0)
  for name in BUFFERS:
    np.testing.assert_array_equal(_bits(again[name]), _bits(got[name]), err_msg=name)


# ---------------------------------------------------------------------------
# the entry points, before any device work
# ---------------------------------------------------------------------------
def test_names_in_header_ctypes_table_and_exports():
  with open(os.path.join(ROOT, 'include', 'ddd1d.h')) as f:
    header = f.read()
  declared = set(re.findall(r'DDD_API\s+[\w\s\*]+?\b(ddd_\w+)\s*\(', header))
  lib = _lib.load_library()
  for name in ('ddd_population_create_replicated', 'ddd_population_load_weights'):
    assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
  assert lib.ddd_abi_version() == 1


def test_create_replicated_refuses_bad_arguments_before_device_work():
  lib = _lib.load_library()
  fake = ctypes.c_void_p(0x1000)   # (never dereferenced below)
  out = ctypes.c_void_p(0x3000)
  status = lib.ddd_population_create_replicated(None, 2, ctypes.byref(out))
  assert status == ERR_INVALID_ARGUMENT and b'model' in lib.ddd_last_error()
  assert out.value is None   # cleared before anything else
  status = lib.ddd_population_create_replicated(fake, 2, None)
  assert status == ERR_INVALID_ARGUMENT and b'out' in lib.ddd_last_error()
  for replicas in (0, -1, _lib.MAX_REPLICAS + 1):
    status = lib.ddd_population_create_replicated(fake, replicas, ctypes.byref(out))
    assert status == ERR_INVALID_ARGUMENT and b'replicas' in lib.ddd_last_error(), replicas


def test_load_weights_refuses_bad_arguments_before_device_work():
  """NULL pointers, and the ranges and sizes no population has (a negative replica or count,
  no weights at all); against a real population: test_gpu_population_weights."""
  lib = _lib.load_library()
  fake = ctypes.c_void_p(0x1000)   # (never dereferenced below)
  status = lib.ddd_population_load_weights(None, fake, 100, 0, 1, None)
  assert status == ERR_INVALID_ARGUMENT and b'population' in lib.ddd_last_error()
  status = lib.ddd_population_load_weights(fake, None, 100, 0, 1, None)
  assert status == ERR_INVALID_ARGUMENT and b'weights' in lib.ddd_last_error()
  for first, count in ((-1, 1), (0, -1)):
    status = lib.ddd_population_load_weights(fake, fake, 100, first, count, None)
    assert status == ERR_INVALID_ARGUMENT and b'negative' in lib.ddd_last_error()
  status = lib.ddd_population_load_weights(fake, fake, 0, 0, 1, None)
  assert status == ERR_INVALID_ARGUMENT and b'n_weights' in lib.ddd_last_error()
