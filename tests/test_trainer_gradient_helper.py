"""CPU side of test_gpu_trainer_gradients.py: the read-back helper proven on torch.optim.Adam before it judges a kernel, and the
input-selection condition over the whole committed case list."""
import pytest
import torch

from decoder_trainer_common import CLS
from oracle import vibo_oracle as O
from trainer_gradient_common import (ALL_PROBLEMS, BETAS, _by_name, adam_step_error, assert_gradients, float32_oracle_distance, ident, layout, moments,
                                     native_gradients, oracle_gradients, parameters, steps_of)
from vibo_amd.trainer import FusedTrainer


class StandIn:
    """A trainer's fields on the CPU: the parameters flattened as FusedCondFlowTrainer flattens them, the moments filled from a
    torch.optim.Adam's state."""

    def __init__(self, model):
        self.model = model
        mlp = model.ability_encoder.mlp
        self.plist = [mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, mlp[4].weight, mlp[4].bias]
        for st in (model.ability_norm_flows, model.item_norm_flows):
            for fl in st.flows:
                self.plist += [fl.u, fl.w, fl.b]
        self.par_flat, self.par_m, self.par_v = FusedTrainer._flatten(self.plist)
        self.item_mu, self.item_lv = model.item_encoder.mu_lookup.weight, model.item_encoder.logvar_lookup.weight
        n = self.item_mu.numel()
        self.item_m, self.item_v = torch.zeros(2 * n), torch.zeros(2 * n)
        self._steps = torch.zeros(2, dtype=torch.int32)

    step_count = property(lambda self: self._steps[0])

    def take(self, opt):
        """Adam's state -> the trainer's moment tensors, in plist's order (not through layout(): that is what is being tested)."""
        off = 0
        for p in self.plist:
            self.par_m[off:off + p.numel()] = opt.state[p]['exp_avg'].reshape(-1)
            self.par_v[off:off + p.numel()] = opt.state[p]['exp_avg_sq'].reshape(-1)
            off += p.numel()
        n = self.item_mu.numel()
        for k, p in enumerate((self.item_mu, self.item_lv)):
            self.item_m[k * n:(k + 1) * n] = opt.state[p]['exp_avg'].reshape(-1)
            self.item_v[k * n:(k + 1) * n] = opt.state[p]['exp_avg_sq'].reshape(-1)
        self._steps += 1


@pytest.mark.parametrize('lr', [5e-3, 1e-3])
def test_gradients_and_adam_steps_read_back_from_torch_adam(lr):
    """Three fp32 torch.optim.Adam steps on known fp32 oracle gradients: native_gradients gives them back to 2^-22 relative from
    either moment's layout, under the state_dict names, and adam_step_error's formula reproduces torch's parameters within its bound."""
    irt, A, I, B = 3, 2, 37, 20
    g = torch.Generator().manual_seed(3)
    resp, mask = O.simulate_responses(irt, B, I, A, generator=g, missing_frac=0.15)
    eps_item, eps_ab = torch.randn(3, I, A + 2, generator=g), torch.randn(3, B, A, generator=g)
    torch.manual_seed(3)
    model = CLS[irt](A, I, ability_merge='product', conditional_posterior=True, n_norm_flows=2)
    tr = StandIn(model)
    assert set(layout(tr)) == set(model.state_dict())
    opt = torch.optim.Adam(tr.plist + [tr.item_mu, tr.item_lv], lr=lr)
    names = {id(p): k for k, p in model.named_parameters()}
    for t in range(1, 4):
        _, want = oracle_gradients(model, resp, mask, eps_item[t - 1], eps_ab[t - 1], BETAS[t - 1], dtype=torch.float32)
        before, p_before = (moments(tr) if t > 1 else None), parameters(tr)
        for p in tr.plist + [tr.item_mu, tr.item_lv]:
            p.grad = want[names[id(p)]].float().reshape(p.shape)
        opt.step()
        tr.take(opt)
        got = native_gradients(tr, before)
        m_now = _by_name(tr, {'par': moments(tr)['par_m'], 'item': moments(tr)['item_m']})
        for k, w in want.items():
            # 2^-22 relative.  After the first step m = 0.1 g and that is relative to max|g|.  Later m_t still carries the earlier
            # gradients: g_t = (m_t - 0.9 m_{t-1}) / 0.1 cancels them, and what is left of m_t's own rounding is 10 ulp(m_t) whatever
            # |g_t| is -- the scale is the larger of max|g_t| and 10 max|m_t| (the same number at t = 1).
            scale = max(float(w.abs().max()), 10.0 * float(m_now[k].abs().max()))
            assert float((got[k] - w).abs().max()) <= 2.0 ** -22 * scale, (t, k)
        if t == 1:
            assert_gradients(got, want, 2.0 ** -22, f'stand-in step {t}')
        if t == 1:
            for k, w in want.items():
                assert float((got.from_v[k] - w.abs()).abs().max()) <= 2.0 ** -22 * float(w.abs().max()), (t, k)
        now, p_after = moments(tr), parameters(tr)
        for b in ('par', 'item'):
            err, bound = adam_step_error(p_before[b], p_after[b], now[b + '_m'], now[b + '_v'], lr, t)
            assert bool((err <= bound).all()), (t, b, float((err / bound).max()))
            # ... and the formula notices a step counter that is off by one, or another learning rate
            err, bound = adam_step_error(p_before[b], p_after[b], now[b + '_m'], now[b + '_v'], lr, t + 1)
            assert bool((err > bound).any()), (t, b)
            err, bound = adam_step_error(p_before[b], p_after[b], now[b + '_m'], now[b + '_v'], 1.01 * lr, t)
            assert bool((err > bound).any()), (t, b)


def test_assert_gradients_refuses_a_scaled_and_a_not_exactly_zero_gradient():
    want = {'a': torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64), 'z': torch.zeros(3, dtype=torch.float64)}
    assert_gradients({k: v.clone() for k, v in want.items()}, want, 1e-4, 'same')
    with pytest.raises(AssertionError):
        assert_gradients({'a': 1.001 * want['a'], 'z': want['z']}, want, 1e-4, 'scaled by 1.001')
    with pytest.raises(AssertionError):
        assert_gradients({'a': want['a'], 'z': want['z'] + 1e-30}, want, 1e-4, 'zero tensor not exactly zero')


@pytest.mark.parametrize('kind,tol,case,make', ALL_PROBLEMS, ids=[f'{k}-{ident(c)}' for k, _, c, _ in ALL_PROBLEMS])
def test_every_committed_case_is_well_conditioned(kind, tol, case, make):
    """The input-selection condition of test_gpu_trainer_gradients.py: on a committed case's inputs the oracle in float32 -- the
    reference's own arithmetic -- is within a quarter of the case's bound of the oracle in float64, on every tensor of every step."""
    p = make()
    dist, name, step = float32_oracle_distance(p.model, steps_of(p))
    print(kind, case, f'float32 oracle distance {dist:.2e} ({name}, step {step})')
    assert dist <= tol / 4, (name, step)
