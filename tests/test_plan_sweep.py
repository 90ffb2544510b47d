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
        kernel, cond, ws, step, noise, lazy, lazy_gathered, multi1, multi3, multi16, err = plan_sweep.answers(lib, d)
        what = plan_sweep.line(d, (kernel, cond, ws, step, noise, lazy, lazy_gathered, multi1, multi3, multi16, err))
        n += 1
        planned += kernel >= 0
        assert (ws > 0) == (kernel >= 0), what
        assert (kernel >= 0) or err, what
        assert noise or not (lazy or lazy_gathered), what
        if d.mask_dtype == _lib.MASK_SIGN:
            # sign-as-mask rows (include/vibo_hip_sign_rows.h): the single-launch matrix kernel or a refusal; the step queries answer
            # for the same rows under a u8 mask, every other query refuses the format
            twin = _lib.ViboDesc.from_buffer_copy(d)
            twin.mask_dtype = _lib.MASK_U8
            assert kernel == MATRIX or kernel < 0, what
            assert (step, noise, lazy, lazy_gathered) == plan_sweep.answers(lib, twin)[3:7], what
            assert cond < 0 and multi1 == multi3 == multi16 == 0, what
            continue
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


def test_sample_optional_query_is_the_rule_it_replaced():
    """vibo_train_step_sample_optional against the rule vibo_elbo_fwd_bwd_step_noise and the trainer each wrote out before the query
    existed, stated here once as the specification: never where the step does not draw its noise; where it does, everywhere but on
    fp32 rows gathered through row_index at fewer than 8 waves of 128 items."""
    lib = _lib.load()
    capable = drawing = kept = 0
    for d in plan_sweep.descriptors(per_cell=2):
        p = ctypes.byref(d)
        got = [lib.vibo_train_step_sample_optional(p, gathered) for gathered in (0, 1)]
        if not lib.vibo_train_step_supported(p) & 1:
            assert got == [0, 0], plan_sweep.line(d, plan_sweep.answers(lib, d))
            continue
        capable += 1
        draws = lib.vibo_train_step_draws_noise(p)
        drawing += draws
        for gathered in (0, 1):
            want = 0 if not draws else int(not (gathered and d.mask_dtype != _lib.MASK_CODES and (d.num_item + 127) // 128 < 8))
            assert got[gathered] == want, (gathered, plan_sweep.line(d, plan_sweep.answers(lib, d)))
            kept += draws and not want
    assert capable >= 1000 and drawing >= 100 and kept >= 10 and drawing > kept
