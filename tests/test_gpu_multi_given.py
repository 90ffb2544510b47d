"""vibo_elbo_multi_forward_given on the GPU: S forward evaluations of the ELBO heads in one pass over the response rows for a
caller-supplied posterior (VIBO_POSTERIOR_GIVEN: --ability-merge mean with or without the conditional posterior, VI_*PL), shared
by the samples ([B, 2A]) or one per sample ([S, B, 2A]) -- against the fp64 table oracle and against S single launches, the
refusals of the C call, and log_marginal of the modules that now go through it."""
import ctypes
import os

import pytest
import torch

from conftest import GOLDEN_DIR, Golden
from golden_common import build_model
from gpu_common import TOL_ELBO, dev, random_problem, record, scattered_rows
from oracle import vibo_table_ref as T
from vibo_amd import _lib, ops
from vibo_amd.ops import ElboSpec
from vibo_amd.torch_core.models import VI_2PL, VIBO_2PL, VIBO_3PL, _normal_logpdf, _std_normal_logpdf

pytestmark = pytest.mark.gpu

# against S single launches (the VALU row-split kernel at these sizes): the bound of the plain multi-sample test
# (tests/test_gpu_parity.py::test_multi_sample_forward_equals_single_launches) -- same statements, sums of the same partial records
TOL_SINGLE = 2e-6


def given_problem(irt, A, B, I, S, n_flows, per_sample, seed):
    """Host tensors: rows, S item samples and noise blocks, the posterior mu = 0.5 randn | logvar = -1 + 0.5 randn, flows."""
    resp, mask, _, _, _ = random_problem(irt, A, B, I, 0.15, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    D = ElboSpec(irt_model=irt, ability_dim=A).item_dim
    items = torch.randn(S, I, D, generator=g)
    eps = torch.randn(S, B, A, generator=g)
    shape = (S, B, A) if per_sample else (B, A)
    post = torch.cat([0.5 * torch.randn(shape, generator=g), -1.0 + 0.5 * torch.randn(shape, generator=g)], dim=-1).contiguous()
    flow = None
    if n_flows:
        raw = torch.randn(n_flows, 2 * A + 1, generator=g) * 0.5
        flow = torch.stack([torch.cat([T.flow_uhat(f[:A], f[A:2 * A]), f[A:]]) for f in raw])      # (uhat | w | b) as the model packs them
    return resp, mask, items, eps, post, flow


def device_rows(resp, mask, rows):
    """-> (response, mask, code, row_index) on the device as the library reads them."""
    d = dev()
    ri = None
    if rows == 'gather':
        big_r, big_m, where = scattered_rows(resp, mask, 40)
        r_, m_ = big_r.to(d), big_m.to(d)
        ri = where.to(d)
    else:
        r_, m_ = resp.to(d), mask.bool().to(d)
    if rows in ('padded', 'codes'):
        r_, m_ = ops.pad_rows(r_, m_)
    if rows == 'codes':
        r_, m_ = ops.pack_cell_codes(r_, m_), None
    if rows == 'nomask':
        m_ = None
    return (*ops.prepare_rows(r_, m_), ri)


CASES = [
    # irt, A, B, I, S, flows, per-sample posterior, rows
    (2, 1, 13, 95, 7, 0, False, 'padded'),       # template width 2, ragged tail, 4 + 2 + 1 samples, one wave
    (2, 8, 33, 1000, 5, 0, True, 'fp32'),        # width 8, 2 + 2 + 1, four waves
    (3, 2, 21, 600, 4, 2, False, 'codes'),
    (1, 4, 9, 332, 3, 0, True, 'gather'),        # row_index into a 40-row matrix (the posterior and eps stay in minibatch order)
    (2, 3, 17, 1100, 6, 0, False, 'fp32'),       # two panels, 1024 + 76
    (2, 2, 10, 2500, 2, 4, True, 'fp32'),        # three panels, flows
]


@pytest.mark.parametrize('irt,A,B,I,S,n_flows,per_sample,rows', CASES)
def test_heads_equal_single_launches_and_the_oracle(irt, A, B, I, S, n_flows, per_sample, rows):
    assert B % 8 != 0
    spec = ElboSpec(irt_model=irt, ability_dim=A, n_flows=n_flows, given=True)
    resp, mask, items, eps, post, flow = given_problem(irt, A, B, I, S, n_flows, per_sample, seed=S * 100 + I)
    d = dev()
    r, m, code, ri = device_rows(resp, mask, rows)
    fl = flow.to(d).contiguous() if flow is not None else None
    items_d, eps_d, post_d = items.to(d), eps.to(d), post.to(d)
    sc = ops._hip_multi_forward(spec, r, m, code, ri, post_d, items_d, eps_d, fl, _lib.REG_SAMPLED, B)
    torch.cuda.synchronize()
    assert sc is not None and tuple(sc.shape) == (S, _lib.NUM_SCALARS)          # (None before this call existed)
    flows64 = [(f[:A].double(), f[A:2 * A].double(), f[2 * A:].double()) for f in flow] if n_flows else None
    assert ops.plan_kernel(spec, B, I, code, False) == _lib.KERNEL_NAMES[2]
    worst = 0.0
    for s in range(S):
        p_s = post[s] if per_sample else post
        a = sc[s, :7].cpu().double()
        ref = T.fused_elbo_ref(p_s.double(), items[s].double(), resp.double(), mask, eps[s].double(), irt_model=irt, ability_dim=A,
                               mode='sampled', flow_uhat_w_b=flows64, given_posterior=True, want_grad=False)
        want = torch.stack([ref['ll'], ref['reg'], ref['kl_ability'], ref['logq0'], ref['logp'], ref['ladj_sum'],
                            torch.tensor(float(B * I), dtype=torch.float64)])          # (GIVEN: every cell counts as observed)
        err = float(((a - want).abs() / want.abs().clamp_min(1.0)).max())
        record('multi_given:oracle', err, TOL_ELBO, sample=s)
        assert err < TOL_ELBO, (s, a, want)
        one = ops._hip_launch_elbo(spec, r, m, code, ri, post_d[s] if per_sample else post_d, items_d[s].contiguous(),
                                   eps_d[s].contiguous(), fl, _lib.REG_SAMPLED, False, B)
        b = one.scalars[:7].cpu().double()
        e1 = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        worst = max(worst, e1)
        record('multi_given:single', e1, TOL_SINGLE, sample=s, panels=(I + 1023) // 1024)
        assert e1 < TOL_SINGLE, (s, a, b)
    print('multi_given: max |multi - single| / max(1, |head|) = %.3g over %d samples' % (worst, S))


@pytest.mark.parametrize('rows', ['fp32', 'nomask'])
def test_shared_and_per_sample_posterior_agree_bitwise(rows):
    irt, A, B, I, S = 2, 3, 19, 200, 5
    spec = ElboSpec(irt_model=irt, ability_dim=A, given=True)
    resp, mask, items, eps, post, _ = given_problem(irt, A, B, I, S, 0, False, seed=77)
    d = dev()
    r, m, code, ri = device_rows(resp, mask, rows)
    args = (items.to(d), eps.to(d), None, _lib.REG_SAMPLED, B)
    shared = ops._hip_multi_forward(spec, r, m, code, ri, post.to(d), *args)
    repeated = ops._hip_multi_forward(spec, r, m, code, ri, post.to(d).unsqueeze(0).repeat(S, 1, 1).contiguous(), *args)
    torch.cuda.synchronize()
    assert shared is not None and repeated is not None and torch.equal(shared, repeated)


def test_bad_calls_are_refused_without_a_launch():
    lib = _lib.load()
    irt, A, B, I, S = 2, 2, 11, 100, 3
    resp, mask, items, eps, post, _ = given_problem(irt, A, B, I, S, 0, False, seed=5)
    d = dev()
    items_d, eps_d, post_d = items.to(d), eps.to(d), post.to(d)
    out = torch.full((S, _lib.NUM_SCALARS), 7.0, device=d)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=d)

    def call(spec, r, m, code, stride, fn='vibo_elbo_multi_forward_given', ability_dim=None):
        desc = ops._rows_desc(spec, B, r, m, code, _lib.REG_SAMPLED, False)
        if ability_dim is not None:
            desc.ability_dim = ability_dim
        args = [ctypes.byref(desc), S, ops._ptr(r), ops._ptr(m), None, ops._ptr(post_d)]
        if fn == 'vibo_elbo_multi_forward_given':
            args.append(ctypes.c_int64(stride))
        rc = getattr(lib, fn)(*args, ops._ptr(items_d), ops._ptr(eps_d), None, ops._ptr(out), ops._ptr(ws), ctypes.c_size_t(ws.numel()),
                              ops._stream(d))
        return rc, lib.vibo_last_error_string().decode()

    given = ElboSpec(irt_model=irt, ability_dim=A, given=True)
    r, m, code = ops.prepare_rows(resp.to(d), mask.bool().to(d))
    assert lib.vibo_multi_given_workspace_bytes(ctypes.byref(ops._rows_desc(given, B, r, m, code, _lib.REG_SAMPLED, False)), S) <= ws.numel()
    for stride in (1, B * 2 * A - 1, B * 2 * A + 4, -B * 2 * A, 2 * A):
        assert call(given, r, m, code, stride)[0] == -3
    r64, m64, code64 = ops.prepare_rows(resp.to(d), mask.long().to(d), keep_int64=True)
    assert code64 == _lib.MASK_I64 and call(given, r64, m64, code64, 0)[0] == -8
    assert ops._hip_multi_forward(given, r64, m64, code64, None, post_d, items_d, eps_d, None, _lib.REG_SAMPLED, B) is None
    assert call(given, r, m, code, 0, ability_dim=12)[0] == -8
    rc, msg = call(given, r, m, code, 0, fn='vibo_elbo_multi_forward')
    assert rc == -8 and 'vibo_elbo_multi_forward_given' in msg
    # ... and the new call takes GIVEN descriptors only
    assert call(ElboSpec(irt_model=irt, ability_dim=A), r, m, code, 0)[0] == -3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())          # nothing ran
    assert call(given, r, m, code, 0)[0] == 0
    torch.cuda.synchronize()
    assert bool((out[:, :7] != 7.0).any())


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------
def module_case(kind):
    d = dev()
    torch.manual_seed(31)
    B = 24
    if kind == 'mean':
        model, irt, A, I = VIBO_2PL(2, 100, ability_merge='mean'), 2, 2, 100
    elif kind == 'mean_cond':
        model, irt, A, I = VIBO_3PL(1, 95, ability_merge='mean', conditional_posterior=True), 3, 1, 95
    elif kind == 'mean_flows':
        model, irt, A, I = VIBO_2PL(3, 95, ability_merge='mean', n_norm_flows=2), 2, 3, 95
    else:
        model, irt, A, I = VI_2PL(2, B, 100), 2, 2, 100
    resp, mask, _, _, _ = random_problem(irt, A, B, I, 0.2, seed=I + A)
    return model.to(d), resp.to(d), mask.bool().to(d)


def loop_value(model, resp, mask, eps_item, eps_ab):
    """log_marginal's loop formula (models.py:445-504) from the heads of one single-launch forward per sample."""
    S, B = eps_item.shape[0], resp.shape[0]
    vi = isinstance(model, VI_2PL)
    r, m, code = ops.prepare_rows(*ops.pad_rows(resp, mask))
    with torch.no_grad():
        if vi:
            item_mu, item_lv = model.item_mu_lookup.weight, model.item_logvar_lookup.weight
            idx = torch.arange(B, device=resp.device)
            shared = torch.cat(model._posterior_rows(idx), dim=1)
        else:
            item_mu, item_lv = model.item_encoder()
        flows = 0 if vi else model.n_norm_flows
        fl = model.ability_norm_flows.packed() if flows else None
        log_w = []
        for s in range(S):
            feat = eps_item[s] * torch.exp(0.5 * item_lv) + item_mu
            lq = _normal_logpdf(feat, item_mu, item_lv).sum()
            item_k = feat
            if flows:
                item_k, item_ladj = model.item_norm_flows(feat)
                lq = lq - item_ladj.sum()
            post = shared if vi else model._mean_posterior(r, m, None, feat)
            one = ops._hip_launch_elbo(model.spec, r, m, code, None, post.contiguous(), item_k.contiguous(), eps_ab[s].contiguous(), fl,
                                       _lib.REG_SAMPLED, False, B)
            log_w.append(one.scalars[_lib.S_LL] - one.scalars[_lib.S_REG] + _std_normal_logpdf(item_k).sum() - lq)
        return float(torch.logsumexp(torch.stack(log_w), 0)) - float(torch.log(torch.tensor(float(S))))


@pytest.mark.parametrize('kind', ['mean', 'mean_cond', 'mean_flows', 'vi'])
def test_log_marginal_runs_no_single_launch_forward(kind):
    model, resp, mask = module_case(kind)
    d, S, B = dev(), 6, resp.shape[0]
    vi = kind == 'vi'
    idx = (torch.arange(B, device=d),) if vi else ()
    I, D = resp.shape[1], model.item_feat_dim
    # the noise of a seeded call, in the loop's order: item, then ability, per sample
    torch.manual_seed(12)
    eps_item, eps_ab = [], []
    for _ in range(S):
        eps_item.append(torch.randn(I, D, device=d))
        eps_ab.append(torch.randn(B, model.ability_dim, device=d))
    eps_item, eps_ab = torch.stack(eps_item), torch.stack(eps_ab)
    want = loop_value(model, resp, mask, eps_item, eps_ab)

    def no_single_launch(*a, **k):
        raise AssertionError('log_marginal ran a single-launch forward')
    saved = dict(ops._BACKEND)
    try:
        ops._BACKEND['elbo'] = no_single_launch
        if not vi:
            replayed = float(model.log_marginal(resp, mask, num_samples=S, eps_item=eps_item, eps_ability=eps_ab))
            assert abs(replayed - want) < 1e-5 * max(1.0, abs(want)), (replayed, want)
        torch.manual_seed(12)
        drawn = float(model.log_marginal(*idx, resp, mask, num_samples=S))
        assert abs(drawn - want) < 1e-5 * max(1.0, abs(want)), (drawn, want)          # the draw order is the loop's
        ops._BACKEND['elbo'] = saved['elbo']
        ops._BACKEND['multi'] = lambda *a: None
        torch.manual_seed(12)
        looped = float(model.log_marginal(*idx, resp, mask, num_samples=S))
        assert abs(drawn - looped) < 1e-5 * max(1.0, abs(looped)), (drawn, looped)
    finally:
        ops._BACKEND.update(saved)


@pytest.mark.parametrize('name', ['logmarg_2pl_a2_mean', 'logmarg_2pl_a2_cond_mean', 'logmarg_3pl_a1_mean_flows2'])
def test_new_log_marginal_goldens_through_module(name):
    g = Golden(os.path.join(GOLDEN_DIR, name + '.npz'))
    d = dev()
    model = build_model(g).to(d)
    calls = []
    saved = ops._BACKEND['multi']
    try:
        ops._BACKEND['multi'] = lambda *a: calls.append(1) or saved(*a)
        logp = model.log_marginal(g.response.to(d).unsqueeze(2), g.mask.to(d).bool().unsqueeze(2),
                                  num_samples=g.meta['num_samples'], eps_item=g.eps_item.to(d), eps_ability=g.eps_ability.to(d))
    finally:
        ops._BACKEND['multi'] = saved
    ref = float(g.out['logp'])
    assert len(calls) == 1 and abs(float(logp) - ref) < 1e-4 * max(1.0, abs(ref))
