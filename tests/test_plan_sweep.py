"""The planner's public queries are views of ONE decision (csrc/vibo_planner.hip: Plan::path / engine / first / tail): over the
descriptors of tools/plan_sweep.py they have to agree with each other.  No launch: runs without a GPU."""
import ctypes
import os
import sys

from conftest import ROOT
from vibo_amd import _lib

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import plan_sweep  # noqa: E402

MATRIX, VALU, NARROW = 1, 2, 6          # VIBO_KERNEL_* of the row-split kernels


def test_sweep_covers_the_planner_constants():
    assert len(plan_sweep.FLAGS) == 20 and len(set(plan_sweep.FLAGS)) == 20
    cells = len(plan_sweep.ITEMS) * len(plan_sweep.ABILITY_DIMS) * len(plan_sweep.POSTERIORS) * len(plan_sweep.MASKS) * len(plan_sweep.FLAGS)
    assert cells * 24 >= 1_000_000 and len(plan_sweep.REST) >= 24
    seen = set()
    for d in plan_sweep.descriptors(per_cell=1):
        seen.add(bytes(d))
    assert len(seen) == cells


def test_planner_queries_agree_with_each_other():
    lib = _lib.load()
    n = planned = 0
    for d in plan_sweep.descriptors(per_cell=1):
        kernel, cond, ws, step, noise, multi1, multi3, multi16, err = plan_sweep.answers(lib, d)
        what = plan_sweep.line(d, (kernel, cond, ws, step, noise, multi1, multi3, multi16, err))
        n += 1
        planned += kernel >= 0
        assert (ws > 0) == (kernel >= 0), what
        assert (kernel >= 0) or err, what
        plain = d.posterior == _lib.POSTERIOR_UNCONDITIONAL and d.n_flows == 0 and d.reg_mode == _lib.REG_KL and d.want_grad
        if noise:
            assert (step & 1) and kernel == MATRIX, what
        if step:
            assert kernel in (VALU, MATRIX, NARROW) and plain, what
        if kernel < 0:
            assert cond == kernel, what                  # (both report the refusal's code)
        elif cond != 0:
            assert cond > 0 and d.posterior == _lib.POSTERIOR_CONDITIONAL and kernel in (VALU, MATRIX), what
            assert not (cond & 4) or kernel == MATRIX, what
        assert (multi1 > 0) == (multi3 > 0) == (multi16 > 0), what
        if multi1 > 0:
            twin = _lib.ViboDesc.from_buffer_copy(d)
            twin.want_grad = 0
            assert d.posterior == _lib.POSTERIOR_UNCONDITIONAL and lib.vibo_plan_kernel(ctypes.byref(twin)) in (VALU, MATRIX, NARROW), what
    assert n >= 40_000 and planned >= n // 3
