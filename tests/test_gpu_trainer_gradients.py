"""Every native train step's gradient, by magnitude, against the fp64 oracle -- and Adam's arithmetic from the kernel's own moments.
The trajectory tests (test_gpu_trainer.py, test_gpu_decoder_trainer.py) see the gradients only through Adam-updated parameters,
and Adam divides the gradient by its own running magnitude: a gradient tensor wrong by a constant factor follows the same
trajectory as a right one.  Here the gradient of each of three steps is read back from Adam's first moments
(trainer_gradient_common.native_gradients) and compared with oracle.vibo_oracle.elbo_loss_and_grads in float64 AT THE PARAMETERS
THE KERNEL STARTED THAT STEP FROM (read from the device), tensor by tensor: max|g - g64| <= tol max|g64|, tol = 1e-4
(gpu_common.TOL_GRAD) for the three IRT-decoder trainers and 2e-4 (test_gpu_decoder.py's bound on vibo_decoder_fwd_bwd) for
FusedDecoderTrainer, no entry left out.  Steps 1 and 2 run at beta = 0.7, step 3 at 1.0 through set_beta.  After each step the loss
is compared to 1e-4 relative and the parameter update to Adam's formula in float64 within 1e-4 lr + 2^-23 |p|.

Input selection (CPU): `python tests/test_gpu_trainer_gradients.py` prints, per case, the worst per-tensor distance between the
oracle in float32 -- the reference's own arithmetic -- and in float64 on the case's inputs; a case is admitted only at a quarter
of its bound or less (2.5e-5 / 5e-5).  Seeds 1, 2, ... were tried per case until that held; the seed and the distance it reached
stand beside each case in trainer_gradient_common.py (measured with one CPU thread: long float32 sums depend on how many threads split them).
test_trainer_gradient_helper.py asserts the condition over all of those lists."""
import ctypes
import os

import pytest

from conftest import Golden, golden_case_files, rel_err
from golden_common import build_model
from gpu_common import dev, record, scattered_rows
from trainer_gradient_common import (ALL_PROBLEMS, CHUNK_CASES, COND_FLOW_CASES, DECODER_CASES, MEAN_CASES, PLAIN_CASES, TOL_DECODER, TOL_IRT,
                                     TOL_LOSS, assert_adam, assert_gradients, assert_second_moment_saw_the_same_gradient, decoder_problem,
                                     family, float32_oracle_distance, ident, irt_problem, moments, native_gradients, oracle_gradients,
                                     parameters, steps_of)
from vibo_amd import _lib, decoder, ops
from vibo_amd.trainer import (FusedCondFlowTrainer, FusedDecoderTrainer, FusedMeanTrainer, FusedTrainer, fused_decoder_trainer_covers,
                              fused_trainer_covers)

pytestmark = pytest.mark.gpu


def print_float32_oracle_distances():
    """Input selection for every list of trainer_gradient_common.py (CPU only)."""
    for kind, tol, case, make in ALL_PROBLEMS:
        p = make()
        dist, name, step = float32_oracle_distance(p.model, steps_of(p))
        print(kind, case, 'float32 oracle distance %.2e (%s, step %d)' % (dist, name, step), 'quarter-bound %.1e' % (tol / 4),
              'ok' if dist <= tol / 4 else 'TRY OTHER INPUTS')


# ---------------------------------------------------------------------------
# three steps: loss, gradient, Adam
# ---------------------------------------------------------------------------
def resident_rows(p, rows_mode, d):
    """-> (response, mask, row_index per step).  'dense': the problem's rows, padded as the CLI's resident matrix is.  'gathered' /
    'codes': the minibatch sits at scattered places of a larger resident matrix (fp32 rows / cell codes) and is read by row_index."""
    if rows_mode == 'dense':
        r, m = ops.pad_rows(p.resp.to(d), p.mask.bool().to(d))
        return r, m, [None if x is None else x.to(d) for x in p.rows]
    assert all(x is None for x in p.rows)
    big_r, big_m, where = scattered_rows(p.resp, p.mask, 2 * p.resp.shape[0] + 5)
    r, m = ops.pad_rows(big_r.to(d), big_m.to(d))
    if rows_mode == 'codes':
        r, m = ops.pack_cell_codes(r, m), None
    return r, m, [where.to(d)] * 3


def run_three_steps(p, what, tol, want_class, lr=5e-3, rows_mode='dense', kernel=None, **trainer_kw):
    d = dev()
    model = p.model.to(d)
    tr = FusedTrainer(model, lr=lr, **trainer_kw)
    assert type(tr) is want_class
    resp, mask, row_index = resident_rows(p, rows_mode, d)
    if kernel is not None:            # the ELBO kernel this case is pinned to (or that the planner chooses for it) is the one asserted
        r_, m_, code = ops.prepare_rows(resp, mask)
        dsc = ops._rows_desc(model.spec, p.eps_ab[0].shape[0], r_, m_, code, _lib.REG_KL, True)
        assert _lib.load().vibo_plan_kernel(ctypes.byref(dsc)) == kernel
    for t, (r_t, m_t, eps_item, eps_ab, beta) in enumerate(steps_of(p), 1):
        before, p_before = (moments(tr) if t > 1 else None), parameters(tr)
        loss64, want = oracle_gradients(model, r_t, m_t, eps_item, eps_ab, beta)
        tr.set_beta(beta)
        loss = tr.step(resp, mask, row_index=row_index[t - 1], eps_item=eps_item.to(d), eps_ability=eps_ab.to(d))
        print(f'{what} step {t}: loss {float(loss):.6f} rel_err {rel_err(loss, loss64):.2e}')
        assert rel_err(loss, loss64) < TOL_LOSS, (what, t)
        got = native_gradients(tr, before)
        assert_gradients(got, want, tol, f'{what} step {t}')
        if t == 1:
            assert_second_moment_saw_the_same_gradient(got, what)
        assert_adam(tr, p_before, before, got, lr, t, what)
    return tr


@pytest.mark.parametrize('rows_mode', ['dense', 'gathered', 'codes'])
@pytest.mark.parametrize('case', PLAIN_CASES, ids=ident)
def test_fused_trainer_gradients(case, rows_mode):
    run_three_steps(irt_problem(*case), 'plain', TOL_IRT, FusedTrainer, rows_mode=rows_mode, fold=False)


MATRIX, VALU, NARROW = 1, 2, 6          # VIBO_KERNEL_* of the row-split kernels


@pytest.mark.parametrize('case,flags,kernel', [(PLAIN_CASES[0], _lib.FLAG_KERNEL_MATRIX, MATRIX), (PLAIN_CASES[1], _lib.FLAG_KERNEL_VALU, VALU),
                                               (PLAIN_CASES[2], 0, NARROW)], ids=['matrix', 'valu', 'narrow'])
def test_fused_trainer_gradients_on_each_elbo_kernel(case, flags, kernel):
    """One case on each ELBO kernel the planner can choose for the plain model: the matrix and VALU row-split kernels pinned as
    test_folded_step_equals_the_unfolded_step pins them, the narrow-row kernel as the planner's own choice at 95 items."""
    with ops.desc_flags(flags):
        run_three_steps(irt_problem(*case), _lib.KERNEL_NAMES[kernel], TOL_IRT, FusedTrainer, kernel=kernel, fold=False)


@pytest.mark.parametrize('case', COND_FLOW_CASES, ids=ident)
def test_fused_cond_flow_trainer_gradients(case):
    run_three_steps(irt_problem(*case), 'cond/flow', TOL_IRT, FusedCondFlowTrainer)


@pytest.mark.parametrize('case', MEAN_CASES, ids=ident)
def test_fused_mean_trainer_gradients(case):
    run_three_steps(irt_problem(*case, mean=True), 'mean', TOL_IRT, FusedMeanTrainer)


@pytest.mark.parametrize('conditional,case', DECODER_CASES, ids=lambda x: ident(x) if isinstance(x, tuple) else ('cond' if x else 'uncond'))
def test_fused_decoder_trainer_gradients(conditional, case):
    run_three_steps(decoder_problem(conditional, case), 'decoder cond' if conditional else 'decoder', TOL_DECODER, FusedDecoderTrainer,
                    conditional=conditional)


@pytest.mark.parametrize('conditional,case', CHUNK_CASES, ids=lambda x: ident(x) if isinstance(x, tuple) else ('cond' if x else 'uncond'))
def test_fused_decoder_trainer_gradients_in_person_chunks(monkeypatch, conditional, case):
    """301 persons at PERSON_CHUNK 64 (chunks of 61 and a last one of 57): the chunked step against the oracle, not only itself."""
    monkeypatch.setattr(decoder, 'PERSON_CHUNK', 64)
    tr = run_three_steps(decoder_problem(conditional, case), 'decoder chunks', TOL_DECODER, FusedDecoderTrainer, conditional=conditional)
    assert list(tr._scratch) == [(301, 64)]


@pytest.mark.parametrize('trainer', ['plain', 'cond/flow', 'mean', 'decoder'])
def test_the_learning_rate_is_read_not_baked_in(trainer):
    """One case per trainer at lr = 1e-3: the same gradients, Adam's update five times shorter."""
    if trainer == 'plain':
        run_three_steps(irt_problem(*PLAIN_CASES[2]), 'plain lr 1e-3', TOL_IRT, FusedTrainer, lr=1e-3, fold=False)
    elif trainer == 'cond/flow':
        run_three_steps(irt_problem(*COND_FLOW_CASES[3]), 'cond/flow lr 1e-3', TOL_IRT, FusedCondFlowTrainer, lr=1e-3)
    elif trainer == 'mean':
        run_three_steps(irt_problem(*MEAN_CASES[2], mean=True), 'mean lr 1e-3', TOL_IRT, FusedMeanTrainer, lr=1e-3)
    else:
        run_three_steps(decoder_problem(*DECODER_CASES[3]), 'decoder lr 1e-3', TOL_DECODER, FusedDecoderTrainer, lr=1e-3)


# ---------------------------------------------------------------------------
# the reference's own recorded gradients (tests/golden/case_*.npz: grad.*)
# ---------------------------------------------------------------------------
def golden_trainer(golden, model):
    """-> (trainer kwargs, bound) of the native trainer that covers the golden's model, or skips with the reason."""
    m = golden.meta
    kind, cond, mean = m.get('generative_model') or 'irt', m['conditional_posterior'], m.get('ability_merge') == 'mean'
    if m['n_norm_flows'] == 0 and not m['use_kl_divergence']:
        pytest.skip('no native trainer covers the sampled regulariser without flows')
    if mean and cond:
        pytest.skip('no native trainer covers mean x conditional')
    if kind == 'irt':
        if not fused_trainer_covers(model):
            pytest.skip('no native trainer covers the mean merge with flows' if mean else
                        'no native trainer covers the conditional posterior / flows beyond 8 ability dimensions')
        return {}, TOL_IRT
    if not fused_decoder_trainer_covers(model, conditional=cond):
        pytest.skip('no native trainer covers an MLP decoder with flows or the mean merge')
    return dict(conditional=cond), TOL_DECODER


@pytest.mark.parametrize('path', golden_case_files(), ids=lambda p: os.path.basename(p)[5:-4])
def test_reference_gradients_through_the_native_step(path):
    """One native step with the golden's noise and annealing factor; native_gradients against the reference's own fp32 gradient
    (grad.*) by the rule golden_common.check_against_golden(strict=True) holds the module path to: within the bound of the fp64
    gradient or of the reference's; where the reference itself is >= 1e-2 from fp64 (3PL cells in the probability clamp band),
    within 6 % of the reference's own distance."""
    golden = Golden(path)
    m = golden.meta
    d = dev()
    model = build_model(golden)
    kw, tol_grad = golden_trainer(golden, model)
    model = model.to(d)
    tr = FusedTrainer(model, lr=5e-3, **kw)
    _, truth = oracle_gradients(model, golden.response, golden.mask, golden.eps_item, golden.eps_ability, m['annealing_factor'])
    resp, mask = ops.pad_rows(golden.response.to(d), golden.mask.to(d).bool())
    p_before = parameters(tr)
    loss = tr.step(resp, mask, beta=m['annealing_factor'], eps_item=golden.eps_item.to(d), eps_ability=golden.eps_ability.to(d))
    print('loss rel_err', rel_err(loss, golden.out['loss']))
    assert rel_err(loss, golden.out['loss']) < TOL_LOSS
    got = native_gradients(tr)
    assert set(got) == set(golden.grad)
    bad = []
    for name, g_ref in golden.grad.items():
        g = got[name]
        if float(g_ref.abs().max()) == 0.0:
            assert float(g.abs().max()) == 0.0, name
            continue
        e_truth, e_ref, ref_off = rel_err(g, truth[name]), rel_err(g, g_ref), rel_err(g_ref, truth[name])
        tol = tol_grad if ref_off < 1e-2 else max(tol_grad, 0.06 * ref_off)
        print(f'{name}: to fp64 {e_truth:.3e}  to the reference {e_ref:.3e}  reference to fp64 {ref_off:.3e}  bound {tol:.1e}')
        record('trainer_grad_golden', min(e_truth, e_ref), tol, what=type(tr).__name__, name=name, family=family(name), e_truth=e_truth,
               e_ref=e_ref, ref_off=ref_off)
        if not min(e_truth, e_ref) < tol:
            bad.append((name, e_truth, e_ref, ref_off))
    assert not bad, bad
    assert_adam(tr, p_before, None, got, 5e-3, 1, 'golden')


if __name__ == '__main__':
    print_float32_oracle_distances()
