"""The native trainers' gradients and Adam arithmetic, read back from Adam's own moments (test_gpu_trainer_gradients.py,
test_trainer_gradient_helper.py), and the cases both files run over.  Every fused trainer keeps the moments in tensors a test can
read (`mlp_m` / `par_m`, `mlp_v` / `par_v`, `item_m`, `item_v`), and adam_update (csrc/vibo_train_hook.hpp) sets m = fma(0.9f, m, 0.1f g), v = fma(0.999f, v, (0.001f g) g):
after the first step of a fresh trainer m = 0.1f g gives g back to one ulp, later g_t = (m_t - 0.9f m_{t-1}) / 0.1f.  The gradient is
thus compared by MAGNITUDE with the fp64 oracle at the parameters the kernel itself differentiated at -- no trajectory, no exclusion
rule -- and Adam's update is checked from the kernel's own m, v and parameters."""
import collections

import torch

from decoder_trainer_common import COND_ORACLE_CASES, ORACLE_CASES, make_problem
from gpu_common import CLS, record, simulated
from oracle import vibo_oracle as O

_f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
B1, W1, B2, W2 = _f32(0.9), _f32(0.1), _f32(0.999), _f32(0.001)      # adam_update's constants as the kernel holds them
U = 2.0 ** -24                                                       # half an fp32 ulp, relative
DENORM = 2.0 ** -149
TOL_LOSS = 1e-4                                                      # TOL_ELBO of the trajectory tests
TOL_IRT, TOL_DECODER = 1e-4, 2e-4                                    # gpu_common.TOL_GRAD; test_gpu_decoder.py's bound on vibo_decoder_fwd_bwd
BETAS = (0.7, 0.7, 1.0)                                              # the KL weight of the three steps


Problem = collections.namedtuple('Problem', 'model resp mask rows eps_item eps_ab')      # rows / eps_ab: one entry per step


# ---------------------------------------------------------------------------
# the cases.  Behind each: the seed's float32-oracle distance (worst tensor over the three steps), at most a quarter of the bound
# ---------------------------------------------------------------------------
# FusedTrainer, four-launch form (the folded step is tied to it bit for bit, moments included: test_folded_step_equals_the_unfolded_step)
# (IRT, A, I, B, model kwargs, seed)
# (1000 items x 300 persons: the [64, 1] first-layer gradient is one float32 sum over 3e5 rows in the reference's arithmetic -- 1.2e-4
#  from fp64 summed by one thread, 3e-6 by 32 -- and still 2.3e-5 to 4.9e-5 at 1000 x 48 and 1000 x 24; 520 x 33 has room)
PLAIN_CASES = [(2, 1, 520, 33, {}, 1),                                                          # seed 1: 1.3e-5
               (2, 8, 200, 130, {}, 1),                                                         # seed 1: 4.8e-6
               (3, 2, 95, 77, {}, 1),                                                           # seed 1: 1.7e-5
               (1, 3, 64, 50, {}, 1)]                                                           # seed 1: 3.2e-6
COND = dict(conditional_posterior=True)
COND_FLOW_CASES = [(2, 1, 200, 130, COND, 2),                                                   # seed 2: 1.1e-6
                   (2, 2, 1100, 48, COND, 1),                                                   # seed 1: 9.4e-7; two panels
                   (2, 3, 95, 50, dict(n_norm_flows=2), 1),                                     # seed 1: 4.0e-6; flows only
                   (3, 1, 120, 77, dict(COND, n_norm_flows=4), 2),                              # seed 2: 1.8e-6
                   # (wide ability + flows: at 200 items x 48 persons no seed up to 20 keeps every cell out of the probability clamp
                   #  band -- 1.0 to 9.7 on the flows' b; at 100 x 33 seed 15 does)
                   (2, 8, 100, 33, dict(COND, n_norm_flows=2), 15),                             # seed 15: 7.1e-6
                   (2, 3, 130, 60, dict(COND, n_norm_flows=2, hidden_dim=48, replace_missing_with_prior=False), 6),      # seed 6: 3.6e-6; --drop-missing
                   (3, 1, 37, 20, dict(COND, hidden_dim=10), 1)]                                # seed 1: 2.0e-6; zero-padded tile
# FusedMeanTrainer: the whole matrix (B + 20 persons) on steps 1 and 3, B gathered rows on step 2.  The mean encoder's posterior is
# wide before training (sd ~ 1 per dimension): at 8 dimensions x 200 items x 150 persons, 3PL at 95 x 97 and hidden 32 at
# 4 dimensions x 130 x 80 every seed up to 20 has cells in the clamp band (1e-2 to 0.7 on the item tensors); the shapes below are the
# largest tried that have a seed which does not.
MEAN_CASES = [(2, 1, 520, 33, {}, 9),                                                           # seed 9: 1.4e-5 (1000 x 300: as for the plain trainer)
              (2, 8, 37, 20, {}, 10),                                                           # seed 10: 1.1e-6
              (3, 2, 37, 33, {}, 6),                                                            # seed 6: 2.2e-5
              (1, 3, 64, 50, dict(replace_missing_with_prior=False), 1),                        # seed 1: 1.4e-6
              (2, 4, 130, 33, dict(hidden_dim=32), 17),                                         # seed 17: 1.9e-6
              (2, 2, 130, 60, dict(hidden_dim=128), 1)]                                         # seed 1: 2.3e-6
# FusedDecoderTrainer: the problems of decoder_trainer_common's two lists -- (decoder, IRT, A, B, I, missing, hidden, drop, seed) --
# with seeds of this file's own rule (the last conditional one sits at 6.0e-5 with that list's seed 15 and has no seed up to 20 at
# 100 persons x 30 items: 3PL at 12 dimensions; 20 x 12 has), and 301 persons for the person chunks
DECODER_SEEDS = [1, 1, 1, 1, 9]                                                                 # 1.0e-5, 3.0e-6, 2.3e-6, 1.0e-6, 6.4e-6
COND_DECODER_SEEDS = [1, 1, 1, 2]                                                               # 3.7e-6, 5.8e-7, 7.4e-7, 3.4e-6
DECODER_CASES = ([(False, c[:-1] + (s,)) for c, s in zip(ORACLE_CASES, DECODER_SEEDS)] +
                 [(True, c[:-1] + (s,)) for c, s in zip(COND_ORACLE_CASES, COND_DECODER_SEEDS)] +
                 [(True, ('residual', 3, 12, 20, 12, 0.1, 48, False, 14))])                     # seed 14: 2.2e-5
CHUNK_CASES = [(False, ('residual', 3, 3, 301, 130, 0.15, 64, False, 3)),                       # seed 3: 2.4e-5
               (True, ('deep', 2, 3, 301, 130, 0.15, 64, False, 1))]                            # seed 1: 4.7e-6


def irt_problem(irt, A, I, B, kw, seed, mean=False):
    """The data and noise of an IRT-decoder case, as make_problem draws them: responses with 15 % missing, three steps' noise."""
    P = B + 20 if mean else B
    resp, mask, g = simulated(irt, P, I, A, 0.15, seed)
    if mean:
        mask[:, 0] = 1                  # (a person without an observed item has no mean: NaN in the reference too)
        resp[:, 0] = resp[:, 0].clamp(min=0)
    rows = [None, torch.randperm(P, generator=g)[:B], None] if mean else [None] * 3
    eps_item = torch.randn(3, I, O.item_feat_dim(irt, A), generator=g)
    eps_ab = [torch.randn(P if r is None else B, A, generator=g) for r in rows]
    torch.manual_seed(seed)
    model = CLS[irt](A, I, ability_merge='mean' if mean else 'product', **kw)
    return Problem(model, resp, mask, rows, eps_item, eps_ab)


def decoder_problem(conditional, case):
    model, resp, mask, eps_item, eps_ab = make_problem(conditional, *case)
    return Problem(model, resp, mask, [None] * 3, eps_item, list(eps_ab))


def steps_of(p):
    """Per step what the oracle sees: (resp, mask, eps_item, eps_ab, beta)."""
    return [(p.resp if r is None else p.resp[r], p.mask if r is None else p.mask[r], p.eps_item[t], p.eps_ab[t], BETAS[t])
            for t, r in enumerate(p.rows)]


ALL_PROBLEMS = ([('plain', TOL_IRT, c, lambda c=c: irt_problem(*c)) for c in PLAIN_CASES] +
                [('cond/flow', TOL_IRT, c, lambda c=c: irt_problem(*c)) for c in COND_FLOW_CASES] +
                [('mean', TOL_IRT, c, lambda c=c: irt_problem(*c, mean=True)) for c in MEAN_CASES] +
                [('decoder', TOL_DECODER, c, lambda c=c: decoder_problem(*c)) for c in DECODER_CASES + CHUNK_CASES])


def ident(case):
    return '-'.join(str(x) if not isinstance(x, dict) else '+'.join(f'{k}={v}' for k, v in x.items()) or 'plain' for x in case)


# ---------------------------------------------------------------------------
# where every state_dict tensor sits in the trainer's flat buffers
# ---------------------------------------------------------------------------
def _flat_fields(tr):
    return (tr.par_flat, tr.par_m, tr.par_v) if hasattr(tr, 'par_flat') else (tr.mlp_flat, tr.mlp_m, tr.mlp_v)


def layout(tr):
    """{state_dict name: (buffer, offset, shape)}: the parameters are views of mlp_flat / par_flat ('par'), the item moments are
    [mu | logvar] ('item').  Every state_dict tensor has to be found, and the views have to tile the flat buffer."""
    flat = _flat_fields(tr)[0]
    base, n_item = flat.data_ptr(), tr.item_mu.numel()
    where, tiled = {}, 0
    for k, v in tr.model.state_dict().items():
        if v.data_ptr() == tr.item_mu.data_ptr():
            where[k] = ('item', 0, v.shape)
        elif v.data_ptr() == tr.item_lv.data_ptr():
            where[k] = ('item', n_item, v.shape)
        else:
            assert base <= v.data_ptr() < base + 4 * flat.numel(), (k, 'is not a view of the flat parameter buffer')
            where[k] = ('par', (v.data_ptr() - base) // 4, v.shape)
            tiled += v.numel()
    assert tiled == flat.numel() and len({(b, o) for b, o, _ in where.values()}) == len(where)
    return where


def _cpu64(t):
    return t.detach().double().cpu().reshape(-1)


def moments(tr):
    """Adam's moments as they are now: float64 CPU copies, {'par_m', 'par_v', 'item_m', 'item_v'}."""
    _, m, v = _flat_fields(tr)
    return {'par_m': _cpu64(m), 'par_v': _cpu64(v), 'item_m': _cpu64(tr.item_m), 'item_v': _cpu64(tr.item_v)}


def parameters(tr):
    """The parameters in the moments' layout: {'par': the flat buffer, 'item': [mu | logvar]}, float64 CPU copies."""
    return {'par': _cpu64(_flat_fields(tr)[0]), 'item': torch.cat([_cpu64(tr.item_mu), _cpu64(tr.item_lv)])}


def _zero_moments(now):
    return {k: torch.zeros_like(v) for k, v in now.items()}


def _by_name(tr, flat):
    return {k: flat[b][o:o + torch.Size(shape).numel()].reshape(shape) for k, (b, o, shape) in layout(tr).items()}


class Gradients(dict):
    """{state_dict name: gradient, float64 on the CPU} recovered from the first moments; `.from_v` holds the same gradients'
    magnitudes recovered from the second moments, `.flat` / `.flat_from_v` both in the moments' own layout."""


def native_gradients(tr, before=None):
    """The gradient the trainer's last step fed to Adam.  `before`: moments(tr) from before that step (None: a fresh trainer,
    zero).  g = (m_t - 0.9f m_{t-1}) / 0.1f; from the second moment |g| = sqrt((v_t - 0.999f v_{t-1}) / 0.001f)."""
    now = moments(tr)
    before = _zero_moments(now) if before is None else before
    flat = {b: (now[b + '_m'] - B1 * before[b + '_m']) / W1 for b in ('par', 'item')}
    flat_v = {b: ((now[b + '_v'] - B2 * before[b + '_v']) / W2).clamp_min(0.0).sqrt() for b in ('par', 'item')}
    g = Gradients(_by_name(tr, flat))
    g.from_v, g.flat, g.flat_from_v = _by_name(tr, flat_v), flat, flat_v
    return g


# ---------------------------------------------------------------------------
# the oracle at the model's current parameters
# ---------------------------------------------------------------------------
def oracle_gradients(model, resp, mask, eps_item, eps_ab, beta, dtype=torch.float64):
    """(loss, {state_dict name: gradient as float64}) of oracle.vibo_oracle.elbo_loss_and_grads at the model's CURRENT parameters,
    read from wherever they live: kernel and oracle always differentiate at the same point.  dtype=torch.float32 evaluates the
    same in the reference's own arithmetic (the input selection below)."""
    params = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()}
    return oracle_at(params, model, resp, mask, eps_item, eps_ab, beta, dtype)


def oracle_at(params, model, resp, mask, eps_item, eps_ab, beta, dtype=torch.float64):
    out, grads = O.elbo_loss_and_grads({k: v.to(dtype) for k, v in params.items()}, resp.cpu().to(dtype), mask.cpu(),
                                       eps_item.cpu().to(dtype), eps_ab.cpu().to(dtype), irt_model=model.IRT,
                                       ability_dim=model.ability_dim, conditional_posterior=model.conditional_posterior,
                                       replace_missing_with_prior=model.replace_missing_with_prior, n_norm_flows=model.n_norm_flows,
                                       annealing_factor=float(beta), generative_model=getattr(model, 'generative_model', 'irt'))
    return float(out['loss']), {k: g.double() for k, g in grads.items()}


def family(name):
    """The tensor family of a state_dict name, as the recorded maxima are reported."""
    if name.startswith('item_encoder.mu'):
        return 'item mu'
    if name.startswith('item_encoder.logvar'):
        return 'item logvar'
    if 'norm_flows' in name:
        return 'flows'
    return 'decoder stacks' if name.startswith('decoder.') else 'encoder MLP'


def assert_gradients(got, want, tol, what):
    """Tensor by tensor: max|got - want| <= tol * max|want|; a tensor whose oracle gradient is identically zero must be exactly
    zero.  No entry is left out.  Every tensor is printed and recorded (VIBO_TOL_RECORD, kind 'trainer_grad') before the assert."""
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    bad = []
    for k, w in want.items():
        g = got[k].double().cpu()
        assert g.shape == w.shape and bool(torch.isfinite(g).all()), (what, k)
        err, top = float((g - w).abs().max()), float(w.abs().max())
        ok = err <= tol * top                              # (top == 0: only an exactly zero gradient passes)
        rel = err / top if top > 0 else (0.0 if err == 0 else float('inf'))
        print(f'{what} {k}: max|g| {top:.3e}  err/max {rel:.3e}  err/bound {rel / tol:.3f}')
        record('trainer_grad', rel, tol, what=what, name=k, family=family(k))
        if not ok:
            bad.append((k, rel))
    assert not bad, (what, tol, bad)


def assert_second_moment_saw_the_same_gradient(g, what):
    """First step of a fresh trainer: v = (0.001f g) g, so sqrt(v / 0.001f) is |g| but for three fp32 roundings (two products and
    m's own 0.1f g), halved by the root -- held to 2^-22 relative; below |g| = 1e-18 v = 0.001 g^2 is subnormal or zero."""
    err = (g.flat['par'].abs() - g.flat_from_v['par']).abs(), (g.flat['item'].abs() - g.flat_from_v['item']).abs()
    top = g.flat['par'].abs(), g.flat['item'].abs()
    for e, t, b in zip(err, top, ('par', 'item')):
        worst = float((e / t.clamp_min(1e-18)).max()) if e.numel() else 0.0
        print(f'{what} {b}: |g| from v against g from m, worst relative {worst:.3e}')
        assert bool((e <= 2.0 ** -22 * t + 1e-18).all()), (what, b, worst)


# ---------------------------------------------------------------------------
# Adam's arithmetic from the kernel's own moments
# ---------------------------------------------------------------------------
def adam_step_error(p_before, p_after, m, v, lr, t):
    """|p_t - (p_{t-1} - lr (m_t / (1 - 0.9^t)) / (sqrt(v_t / (1 - 0.999^t)) + 1e-8))| and its bound 1e-4 lr + 2^-23 |p_{t-1}|, in float64.
    The bound's first term: the kernel forms 1 - 0.999^t in fp32 (adam_bias), up to 2^-24 / 0.001 = 6e-5 relative at t = 1, halved
    by the root; the rest is a handful of fp32 roundings on a step of at most about lr."""
    want = p_before - lr * (m / (1.0 - 0.9 ** t)) / ((v / (1.0 - 0.999 ** t)).sqrt() + 1e-8)
    return (p_after - want).abs(), 1e-4 * lr + 2.0 ** -23 * p_before.abs()


def assert_adam(tr, p_before, before, g, lr, t, what):
    """After step t: the parameters moved as torch.optim.Adam's formula says from the kernel's own m_t, v_t; v_t follows
    0.999f v_{t-1} + 0.001f g_t^2 with g_t the kernel's own gradient (from m) to 4 x 2^-24 relative plus one fp32 denormal step
    (after the first step: plus what the recovery of g_t from two roundings of m costs, see below)."""
    assert int(tr.step_count) == t, (what, int(tr.step_count), t)
    now, p_after = moments(tr), parameters(tr)
    before = _zero_moments(now) if before is None else before
    for b in ('par', 'item'):
        err, bound = adam_step_error(p_before[b], p_after[b], now[b + '_m'], now[b + '_v'], lr, t)
        worst = float((err / bound).max())
        print(f'{what} step {t} {b}: Adam update, worst error / bound {worst:.3f} (largest error {float(err.max()):.3e})')
        record('trainer_adam', err.max(), 1e-4 * lr, what=what, name=b, step=t, ratio=worst)
        assert bool((err <= bound).all()), (what, b, t, worst, int((err > bound).sum()))
        v_want = B2 * before[b + '_v'] + W2 * g.flat[b] ** 2
        # From the second step on g_t itself is known only to U (|g_t| + 10 |m_t|) -- m_t's own rounding, divided by 0.1 -- and
        # 0.001 g_t^2 carries twice that, relative; at the first step m = 0.1f g is exact but for one rounding, inside the 4 U.
        g_abs = g.flat[b].abs()
        slack = 0.0 if t == 1 else W2 * 2.0 * g_abs * U * (g_abs + 10.0 * now[b + '_m'].abs())
        off = (now[b + '_v'] - v_want).abs() > 4 * U * v_want + DENORM + slack
        underflow = off & (v_want < 2.0 ** -126)
        print(f'{what} step {t} {b}: second-moment recurrence, {int(off.sum())} of {off.numel()} entries off, '
              f'{int(underflow.sum())} of them where v underflows')
        assert not bool((off & ~underflow).any()), (what, b, t, int((off & ~underflow).sum()),
                                                    float(((now[b + '_v'] - v_want).abs() / v_want.clamp_min(1e-300))[off & ~underflow].max()))


# ---------------------------------------------------------------------------
# input selection (CPU): how far the reference's own arithmetic sits from fp64 on a case's inputs
# ---------------------------------------------------------------------------
def float32_oracle_distance(model, steps, lr=5e-3):
    """The worst per-tensor max|g32 - g64| / max|g64| between the oracle in float32 (the reference's own arithmetic) and in
    float64, both at the same fp32 parameters, over the three steps of a float64 Adam trajectory from the model's parameters.
    `steps`: per step (resp, mask, eps_item, eps_ab, beta).  Returns (distance, tensor name, step)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # (float32 sums over 1e5 rows depend on how many threads split them: one thread, the longest chains)
    try:
        return _float32_oracle_distance(model, steps, lr)
    finally:
        torch.set_num_threads(threads)


def _float32_oracle_distance(model, steps, lr):
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    worst = (0.0, None, 0)
    for t, (resp, mask, eps_item, eps_ab, beta) in enumerate(steps, 1):
        at = {k: v.detach().float() for k, v in params.items()}
        _, g64 = oracle_at(at, model, resp, mask, eps_item, eps_ab, beta, torch.float64)
        _, g32 = oracle_at(at, model, resp, mask, eps_item, eps_ab, beta, torch.float32)
        for k in g64:
            top = float(g64[k].abs().max())
            if top > 0:
                worst = max(worst, (float((g32[k] - g64[k]).abs().max()) / top, k, t))
        for k, p in params.items():
            p.grad = g64[k]
        opt.step()
    return worst
