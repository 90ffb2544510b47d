"""What the tests of the un-amortized trainers (FusedVITrainer / FusedMLETrainer, include/vibo_hip_person_tables.h) share: the cases,
their inputs, the float64 references and the reading of Adam's moments.  Importable without a GPU.

Inputs: the models' default N(0, 1) initialisation is NOT used -- on it the reference's own float32 arithmetic sits up to 0.7
relative from float64 in a gradient tensor (saturated logits in the probability clamp band).  Instead
    VI   mu = 0.5 N(0,1), logvar = -3 + 0.3 N(0,1) for the person and the item tables
    MLE  0.5 N(0,1) for both tables
with coin-flip responses, 15 % missing.  A case is admitted only where the float32-to-float64 distance per tensor
(max|g32 - g64| / max|g64|), over the three steps of a float64 Adam trajectory, is at most a quarter of the gradient bound:
test_person_table_trainer_host.py asserts it for every case (the rule of trainer_gradient_common.py)."""
import collections

import torch

from oracle import vibo_oracle as O
from vibo_amd.torch_core.models import MLE_1PL, MLE_2PL, MLE_3PL, VI_1PL, VI_2PL, VI_3PL

VI_CLS = {1: VI_1PL, 2: VI_2PL, 3: VI_3PL}
MLE_CLS = {1: MLE_1PL, 2: MLE_2PL, 3: MLE_3PL}
BETAS = (0.7, 0.7, 1.0)
ADMIT = 2.5e-5            # a quarter of gpu_common.TOL_GRAD

# (IRT, A, P, I, B, seed); behind each the seed's float32-oracle distance, VI / MLE (worst tensor over the three steps, one CPU thread)
CASES = [(2, 1, 257, 100, 16, 1),             # 1.7e-7 / 1.5e-7
         (2, 8, 4099, 200, 130, 1),           # 3.7e-7 / 4.0e-7
         (3, 2, 1000, 95, 77, 1),             # 4.9e-7 / 5.3e-7
         (1, 3, 5, 64, 5, 1),                 # 1.6e-7 / 1.1e-7
         (2, 8, 3000, 1000, 2100, 1),         # 4.0e-7 / 3.4e-7
         (3, 5, 5000, 640, 4500, 1)]          # 1.1e-6 / 7.5e-7

Problem = collections.namedtuple('Problem', 'method irt A P I B params resp mask index eps_item eps_ab')


def ident(case):
    return '-'.join(str(x) for x in case)


def names(method):
    """state_dict names: person tables, then item tables."""
    if method == 'vi':
        return ['ability_mu_lookup.weight', 'ability_logvar_lookup.weight'], ['item_mu_lookup.weight', 'item_logvar_lookup.weight']
    return ['ability.weight'], ['item_feat.weight']


def make_problem(method, irt, A, P, I, B, seed):
    """Host tensors: the response matrix of all P persons, the parameters, and per step a minibatch index [B] (three minibatches
    that differ and overlap partly: windows of one permutation, half a minibatch apart, each shuffled) and the noise."""
    g = torch.Generator().manual_seed(seed)
    resp = (torch.rand(P, I, generator=g) < 0.5).float()
    mask = torch.rand(P, I, generator=g) >= 0.15
    D = O.item_feat_dim(irt, A)
    n = lambda *shape: torch.randn(*shape, generator=g)
    if method == 'vi':
        params = {'ability_mu_lookup.weight': 0.5 * n(P, A), 'ability_logvar_lookup.weight': -3.0 + 0.3 * n(P, A),
                  'item_mu_lookup.weight': 0.5 * n(I, D), 'item_logvar_lookup.weight': -3.0 + 0.3 * n(I, D)}
    else:
        params = {'ability.weight': 0.5 * n(P, A), 'item_feat.weight': 0.5 * n(I, D)}
    perm = torch.randperm(P, generator=g)
    index = []
    for t in range(3):
        window = torch.roll(perm, -t * max(1, B // 2))[:B]
        index.append(window[torch.randperm(B, generator=g)])
    eps_item = torch.randn(3, I, D, generator=g)
    eps_ab = [torch.randn(B, A, generator=g) for _ in range(3)]
    return Problem(method, irt, A, P, I, B, params, resp, mask, index, eps_item, eps_ab)


def build_model(p, device=None):
    cls = (VI_CLS if p.method == 'vi' else MLE_CLS)[p.irt]
    model = cls(p.A, p.P, p.I)
    model.load_state_dict(p.params)
    return model if device is None else model.to(device)


def reference(p, params, t, dtype=torch.float64):
    """(loss, {name: dense gradient}) of step t (0-based) at `params`, in `dtype`.  VI: oracle.vibo_oracle.vi_elbo_forward + autograd;
    MLE: the masked-BCE mean over all B x I cells (mle.py:193-196) written with O.irt_link / O.masked_bernoulli_ll."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    idx = p.index[t]
    resp, mask = p.resp[idx].to(dtype), p.mask[idx]
    if p.method == 'vi':
        loss = O.vi_elbo_forward(leaves, idx, resp, mask, p.eps_item[t].to(dtype), p.eps_ab[t].to(dtype), irt_model=p.irt,
                                 ability_dim=p.A, annealing_factor=BETAS[t])['loss']
    else:
        probs = O.irt_link(p.irt, leaves['ability.weight'][idx], leaves['item_feat.weight'])
        loss = -O.masked_bernoulli_ll(resp, mask, probs).sum() / float(p.B * p.I)
    ks = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in ks])
    return float(loss.detach()), {k: g.double() for k, g in zip(ks, grads)}


def float32_distance(p, lr=5e-3):
    """The worst per-tensor max|g32 - g64| / max|g64| over the three steps of a float64 torch.optim.Adam trajectory (dense, whole
    tables), both gradients at the same fp32 parameters; one thread.  -> (distance, tensor name, step)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        params = {k: v.double().clone().requires_grad_(True) for k, v in p.params.items()}
        opt = torch.optim.Adam(list(params.values()), lr=lr)
        worst = (0.0, None, 0)
        for t in range(3):
            at = {k: v.detach().float() for k, v in params.items()}
            _, g64 = reference(p, at, t, torch.float64)
            _, g32 = reference(p, at, t, torch.float32)
            for k in g64:
                worst = max(worst, (float((g32[k] - g64[k]).abs().max()) / float(g64[k].abs().max()), k, t + 1))
            for k, v in params.items():
                v.grad = g64[k]
            opt.step()
        return worst
    finally:
        torch.set_num_threads(threads)


class TableView:
    """A person-table trainer as trainer_gradient_common.moments / parameters / assert_adam read a trainer: par_* = the person tables
    (and their moments) one after the other, item_* as they are.  A snapshot of the tables; the moments are read when asked."""

    def __init__(self, tr):
        self.tr = tr
        self.item_mu, self.item_m, self.item_v = tr.item_mu, tr.item_m, tr.item_v
        self.item_lv = tr.item_lv if tr.item_lv is not None else tr.item_mu.new_empty(0)

    par_flat = property(lambda self: torch.cat([t.detach().reshape(-1) for t in self.tr.tables]))
    par_m = property(lambda self: self.tr.person_m.reshape(-1))
    par_v = property(lambda self: self.tr.person_v.reshape(-1))
    step_count = property(lambda self: self.tr.step_count)


def by_name(method, flat, P, A, I, D):
    """{'par': ..., 'item': ...} flat vectors -> {state_dict name: tensor}."""
    pn, it = names(method)
    out = {k: flat['par'][j * P * A:(j + 1) * P * A].reshape(P, A) for j, k in enumerate(pn)}
    out.update({k: flat['item'][j * I * D:(j + 1) * I * D].reshape(I, D) for j, k in enumerate(it)})
    return out
