"""The reference's goldens (tests/golden/case_*.npz, conftest.Golden) through a drop-in module: the model with the golden's
parameters, the reference's call pattern with the golden's noise replayed, and the comparison of loss, posterior and gradients.
test_host_logic.py runs them on the CPU stand-in, the GPU files on the HIP kernels."""
import torch

from conftest import rel_err
from gpu_common import CLS, record
from oracle import vibo_oracle as O


def build_model(golden):
    m = golden.meta
    model = CLS[m['irt_model']](m['ability_dim'], m['num_item'], hidden_dim=m['hidden_dim'],
                                ability_merge=m.get('ability_merge', 'product'), conditional_posterior=m['conditional_posterior'],
                                replace_missing_with_prior=m['replace_missing_with_prior'],
                                n_norm_flows=m['n_norm_flows'], generative_model=m.get('generative_model', 'irt'))
    model.load_state_dict(golden.sd, strict=True)      # same keys and shapes as the reference
    return model


def run_reference_pattern(model, golden, mask_dtype=torch.int64):
    """vibo.py:239-267 call pattern with the golden's eps replayed."""
    m = golden.meta
    response = golden.response.unsqueeze(2)
    mask = golden.mask.to(mask_dtype).unsqueeze(2)
    outs = model(response, mask, eps_item=golden.eps_item, eps_ability=golden.eps_ability)
    if m['n_norm_flows'] > 0:
        (r, k, rmu, ak, a0, amu, alv, aladj, ik, i0, imu, ilv, iladj) = outs
        loss = model.elbo(r, k, rmu, a0, amu, alv, i0, imu, ilv, annealing_factor=m['annealing_factor'],
                          use_kl_divergence=False, ability_k=ak, item_feat_k=ik,
                          ability_logabsdetjac=aladj, item_logabsdetjac=iladj)
    else:
        loss = model.elbo(*outs, annealing_factor=m['annealing_factor'],
                          use_kl_divergence=m['use_kl_divergence'])
    return outs, loss


def check_against_golden(model, golden, outs, loss, tol_loss=1e-4, tol_grad=3e-4, tol_truth=1.5e-3, strict=False):
    m = golden.meta
    assert rel_err(loss.detach(), golden.out['loss']) < tol_loss
    flows = m['n_norm_flows'] > 0
    amu, alv, a0 = (outs[5], outs[6], outs[4]) if flows else (outs[4], outs[5], outs[3])
    assert (amu.cpu() - golden.out['ability_mu']).abs().max() < 2e-5 * max(1.0, float(golden.out['ability_mu'].abs().max()))
    assert (alv.cpu() - golden.out['ability_logvar']).abs().max() < 2e-5 * max(1.0, float(golden.out['ability_logvar'].abs().max()))
    assert (a0.cpu() - golden.out['ability']).abs().max() < 5e-5 * max(1.0, float(golden.out['ability'].abs().max()))
    if flows:
        assert (outs[3].cpu() - golden.out['ability_k']).abs().max() < 1e-4
        assert (outs[7].cpu() - golden.out['ability_logabsdetjac']).abs().max() < 1e-4
    loss.backward()
    # The reference computes in fp32 and its own gradients carry rounding noise (up to ~8e-4 of the
    # tensor's max on 3PL cases: the probability clamp + log).  Allow  tol + |golden - fp64 oracle|.
    sd64 = {k: v.double() for k, v in golden.sd.items()}
    _, truth = O.elbo_loss_and_grads(sd64, golden.response.cpu().double(), golden.mask.cpu(),
                                     golden.eps_item.cpu().double(), golden.eps_ability.cpu().double(),
                                     **golden.cfg)
    for name, p in model.named_parameters():
        g_ref = golden.grad[name]
        g = p.grad.cpu() if p.grad is not None else torch.zeros_like(g_ref)
        scale = float(g_ref.abs().max())
        if scale == 0.0:
            assert float(g.abs().max()) < 1e-6, name
        else:
            # the fp32 CPU stand-in is as noisy as the reference (whose own fp32 gradients sit up to 1.6e-2 from fp64 on
            # the mean-merge encoder's first layer): allow the reference's own distance from the fp64 oracle on top
            if strict:
                # the HIP path (tests/test_gpu_parity.py): within tol of the exact (fp64) gradient, or -- where the reference's
                # own fp32 arithmetic sits further from it than that (3PL cells inside the probability clamp band) -- within
                # tol of the reference's gradient.  No allowance added on top of either.
                e_truth, e_ref = rel_err(g, truth[name]), rel_err(g, g_ref)
                ref_off = rel_err(g_ref, truth[name])
                # (one golden, 3pl_a8_uncond_mean_miss: the reference's own fp32 gradients are 3-18 % away from the exact ones --
                #  saturated 3PL cells; a tensor the reference gets that wrong is held to 6 % of the reference's own error instead)
                # Measured on the GPU over all goldens x kernel pins (gpurun_out/r6_tolerances_golden.jsonl, round 6): every tensor of
                # every golden but one is within 2.9e-5; the one is 3pl_a8_uncond_mean_miss, whose cells sit inside the probability
                # clamp band -- there the measured distance to the reference is <= 0.053 x the reference's own distance to fp64.
                # (2pl_a10_uncond_flows2 has such cells too -- flows push the sample out: its reference gradients are up to 4 % from
                #  fp64 -- but the kernel stays within 2.9e-5 of the reference there)
                clamp_band = ref_off >= 1e-2
                tol = tol_grad if not clamp_band else max(tol_grad, 0.06 * ref_off)
                record('golden:' + name, min(e_truth, e_ref), tol, e_truth=e_truth, e_ref=e_ref, ref_off=ref_off, irt=m['irt_model'])
                assert min(e_truth, e_ref) < tol, (name, e_truth, e_ref, ref_off)
                continue
            assert rel_err(g, truth[name]) < tol_truth + rel_err(g_ref, truth[name]), name
            assert rel_err(g, g_ref) < tol_grad + rel_err(g_ref, truth[name]), name
