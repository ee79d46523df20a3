"""The planner of the training entry points (csrc/train_plan.h) without a GPU.

tests/train_plan_harness.hip prints every number the planner sets -- workgroups, LDS bytes,
workspace bytes, the slab offsets and strides, the MFMA decision and the staged kernels'
offsets, the layer and projection tables, the rollout-run tail -- for a fixed table of cases,
each through the seven plans.  They are compared, field by field, with
tests/golden/train_plans.json, recorded from the configuration functions the planner
replaced, and the workspace bytes with what the library's ddd_*_workspace_bytes return."""
import ctypes
import json
import os
import subprocess

import pytest

from helpers import ROOT
from test_cpu_training import _config
from ddd1d_amd import _lib

HARNESS = os.path.join(ROOT, 'tests', 'train_plan_harness.hip')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'train_plans.json')
PLANS = ('training', 'unrolled', 'rollout', 'run', 'population', 'metrics', 'rollout_run')


def _key(row):
  return row['case'], row['plan'], row['batch'], row['T'], row['R']


@pytest.fixture(scope='module')
def golden():
  with open(GOLDEN) as f:
    return json.load(f)['rows']


@pytest.fixture(scope='module')
def planned(tmp_path_factory):
  """The harness's rows: compiled by hipcc (no kernel in it), run as a program."""
  program = str(tmp_path_factory.mktemp('train_plan') / 'train_plan_harness')
  subprocess.run(['hipcc', '--offload-arch=gfx950', '-std=c++17', '-O1', HARNESS, '-o', program],
                 check=True)
  done = subprocess.run([program], capture_output=True, text=True)
  assert done.returncode == 0, done.stdout + done.stderr
  return [json.loads(line) for line in done.stdout.splitlines()]


def test_every_planned_number_is_the_recorded_one(planned, golden):
  assert [_key(row) for row in planned] == [_key(row) for row in golden]
  for got, want in zip(planned, golden):
    assert got.keys() == want.keys(), _key(want)
    for field in want:
      assert got[field] == want[field], (_key(want), field, got[field], want[field])


def test_table_reaches_every_branch(golden):
  """What the cases are there for: the recorded rows take each path of the planner."""
  rows = {_key(row): row for row in golden}
  assert all(row['rc'] == 0 for row in golden)
  for case in sorted(set(row['case'] for row in golden)):
    assert set(row['plan'] for row in golden if row['case'] == case) == set(PLANS), case
  staged = rows['default', 'training', 4, 0, 1]
  assert staged['mfma'] == 1 and staged['wl_off'] == [-1, 0, -1] and staged['wl_floats'] == 5120
  for case in ('points40', 'filters16', 'big8x7'):
    for row in golden:
      if row['case'] == case:
        assert row['mfma'] == 0 and row['wl_floats'] == 0 and set(row['wl_off']) == {-1}, _key(row)
  # staged for one evaluation, not next to the two rows of the through-time kernels:
  # 162 816 and 164 864 bytes either side of the 160 KiB
  for row in golden:
    if row['case'] == 'big6x5':
      one_evaluation = row['plan'] == 'training' or (
          row['plan'] in ('run', 'population', 'metrics') and row['T'] == 0)
      assert row['mfma'] == (1 if one_evaluation else 0), _key(row)
      assert row['lds_bytes'] == (162816 if one_evaluation else 164864 - 4 * 5 * 32 * 32 * 4)
  assert rows['ks_projected', 'training', 4, 0, 1]['in_size'] == [5, 4, 2, 0]
  assert rows['ks_projected', 'training', 4, 0, 1]['C_out'] == 11
  assert rows['ks_order0', 'training', 4, 0, 1]['C_out'] == 21
  assert rows['ks_space_derivatives', 'training', 4, 0, 1]['C_out'] == 3
  assert [rows['batch%d' % b, 'training', b, 0, 1]['blocks'] for b in (1, 512, 4096)] == [
      1, 512, 512]
  seen = lambda plan: set((row['T'], row['R']) for row in golden if row['plan'] == plan)
  assert {t for t, _ in seen('unrolled')} == {1, 8}
  assert {t for t, _ in seen('rollout')} == {1, 9, 256}
  for plan in ('population', 'metrics'):
    assert {t for t, _ in seen(plan)} == {0, 2} and {r for _, r in seen(plan)} == {1, 2, 64}
  assert {r for _, r in seen('rollout_run')} == {1, 2, 64}
  # n_weights + T is padded to four floats: 5666 + 9 -> 5676
  assert rows['default', 'rollout', 4, 9, 1]['n_slab'] == 5676


def test_library_asks_for_the_planned_workspace(golden):
  """The shipped unit plans what the harness does: ddd_*_workspace_bytes of the built
  library, through ctypes, for every row."""
  lib = _lib.load_library()
  for row in golden:
    fields = dict(row['cfg'])
    sizes = fields.pop('input_sizes')
    cfg = _config(dx=1.0 / fields['num_points'], **fields)
    for d, size in enumerate(sizes):
      cfg.input_sizes[d] = size
    ref, batch, steps, replicas = ctypes.byref(cfg), row['batch'], row['T'], row['R']
    got = {
        'training': lambda: (lib.ddd_train_workspace_bytes(ref, batch),
                             lib.ddd_vjp_workspace_bytes(ref, batch)),
        'unrolled': lambda: (lib.ddd_train_unrolled_workspace_bytes(ref, batch, steps),),
        'rollout': lambda: (lib.ddd_train_rollout_workspace_bytes(ref, batch, steps),),
        'run': lambda: (lib.ddd_train_run_workspace_bytes(ref, batch, steps),),
        'population': lambda: (lib.ddd_train_population_workspace_bytes(ref, batch, steps,
                                                                        replicas),),
        'metrics': lambda: (lib.ddd_eval_metrics_workspace_bytes(ref, batch, steps, replicas),),
        'rollout_run': lambda: (lib.ddd_train_rollout_run_workspace_bytes(ref, batch, steps,
                                                                         replicas),),
    }[row['plan']]()
    assert all(value == row['ws_bytes'] for value in got), (_key(row), got, row['ws_bytes'],
                                                           lib.ddd_last_error())
