"""vibo_elbo_multi_forward_cond on the GPU: log_marginal's S forward evaluations for the product of experts of the conditional
posterior in one call -- the experts' sums of up to 64 / 2A item samples per one-hot x table contraction over the cell codes
(cm_table_image_stack_kernel, cm_forward_kernel<1 | 2 | 4>), the per-person finish (cond_stack_finish_kernel) and the GIVEN
multi-sample pass on the posteriors that come out.

Posterior, entry by entry (posterior_out): patterns `single` and `few` of oracle/onehot_model.py with an unobserved last item
and one person who observes nothing, expert means in [1, 3], logvar in [-6, 0]; every mu / logvar against the fp64 product of
experts of the fp32 table of its sample within the counted bound of tests/test_gpu_onehot_contractions.py (_posterior_bounds,
entry 'encode': c_forward(k) + C_TAU + the finish `smu / lam`, `logf(1.0f / lam)`, + 2 with the prior term) -- imported from
there, no comparison uses a tensor's max-abs; `single` rows bit for bit against vibo_encode on table s.  Samples do not leak into
each other: alone, in a stack and in the reversed stack a sample's posterior has the same bits (2A = 6 and 10: samples straddle
the 16-column tiles).  Heads against the fp64 table oracle and against S single conditional launches; the refusals of the C
call; log_marginal of the modules that now go through it.

|multi - single launches|: the single launch finishes its posterior as s * (1 / lam), -ln 2 * log2 lam, this call as s / lam,
logf(1 / lam), so the heads differ by roundings no bound here derives.  Observed on an MI355X (profiles/r09_multi_cond_tolerance.txt),
worst case / max(1, max|head|) 1.14e-07: asserted at TOL_SINGLE = 3e-07."""
import ctypes
import os

import numpy as np
import pytest
import torch

import test_gpu_onehot_contractions as OH
from conftest import GOLDEN_DIR, Golden
from golden_common import build_model
from gpu_common import TOL_ELBO, dev, random_problem, record, scattered_rows
from oracle import vibo_table_ref as T
from vibo_amd import _lib, ops
from vibo_amd.ops import ElboSpec
from vibo_amd.torch_core.models import VIBO_2PL, VIBO_3PL, _normal_logpdf, _std_normal_logpdf

pytestmark = pytest.mark.gpu

# twice the worst |multi - single launches| / max(1, max|head|) of profiles/r09_multi_cond_tolerance.txt, rounded up to one digit
# (the kernels are deterministic; the factor covers another box's libm), never above TOL_ELBO
TOL_SINGLE = 3e-7          # (worst recorded: 1.14e-07)
assert TOL_SINGLE <= TOL_ELBO


def multi_cond(spec, r, m, code, ri, tables, items, eps, flow, B, want_post=True):
    """vibo_elbo_multi_forward_cond on device tensors -> (scalars [S, 8], posterior_out [S, B, 2A] or None)."""
    lib = _lib.load()
    d = dev()
    S, A = int(items.shape[0]), spec.ability_dim
    desc = ops._rows_desc(spec, B, r, m, code, _lib.REG_SAMPLED, False)
    ws_bytes = lib.vibo_multi_cond_workspace_bytes(ctypes.byref(desc), S)
    assert ws_bytes > 0, lib.vibo_last_error_string().decode()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d)
    out = torch.empty(S, _lib.NUM_SCALARS, device=d)
    post = torch.full((S, B, 2 * A), 7.0, device=d) if want_post else None
    ops._call('vibo_elbo_multi_forward_cond', ctypes.byref(desc), S, ops._ptr(r), ops._ptr(m), ops._ptr(ri), ops._ptr(tables),
              ops._ptr(items), ops._ptr(eps), ops._ptr(flow), ops._ptr(out), ops._ptr(post), ops._ptr(ws), ctypes.c_size_t(ws_bytes),
              ops._stream(d))
    torch.cuda.synchronize()
    return out, post


def lib_query(spec, r, m, code, B, S):
    desc = ops._rows_desc(spec, B, r, m, code, _lib.REG_SAMPLED, False)
    return _lib.load().vibo_multi_cond_workspace_bytes(ctypes.byref(desc), S)


# ---------------------------------------------------------------------------
# the posterior, entry by entry
# ---------------------------------------------------------------------------
# (ability_dim, samples): a full group of 64 // 2A samples and a remainder -- at ability_dim 2 a full 16-column tile and a
# remainder (5), and the full group of 16 as well (17)
SAMPLES = [(1, 33), (2, 5), (2, 17), (3, 11), (5, 7), (8, 5)]


def pattern_rows(pattern, I, B):
    """Cell codes [B, I] uint8: the first B persons of the pattern over I - 1 items, the last item observed by nobody, person 1
    observing nothing."""
    full = OH._cond_codes(I, pattern)[0]
    codes = full[np.arange(B) % full.shape[0]].copy()          # (64 items: 126 persons in the pattern)
    codes[1, :] = 2
    return codes


def stacked_tables(S, I, A, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([1.0 + 2.0 * torch.rand(S, 2, I, A, generator=g), -6.0 * torch.rand(S, 2, I, A, generator=g)], dim=3).contiguous()


def poe64(codes, table):
    """What OH._posterior_bounds reads: the fp64 product of experts' sums of one fp32 table [2, I, 2A]."""
    A = table.shape[2] // 2
    oh = OH.M.onehots(codes)
    t = table.numpy().astype(np.float64)
    mu, lv = t[..., :A], t[..., A:]
    tau = 1.0 / (np.exp(lv) + OH.EPS32)
    return dict(k=(codes != 2).sum(1), lam=oh[0] @ tau[0] + oh[1] @ tau[1], s=oh[0] @ (mu * tau)[0] + oh[1] @ (mu * tau)[1])


def rows_on_device(codes, rows):
    d = dev()
    if rows == 'codes':
        I = codes.shape[1]
        return ops.prepare_rows(OH._code_rows(codes, (I + 15) // 16 * 16), None)
    return ops.prepare_rows(torch.from_numpy((codes == 1).astype(np.float32)).to(d), torch.from_numpy(codes != 2).to(d))


@pytest.mark.parametrize('B,rows', [(13, 'fp32'), (65, 'codes'), (130, 'fp32')])
@pytest.mark.parametrize('I', [64, 200, 1000])
@pytest.mark.parametrize('A,S', SAMPLES)
def test_posterior_entry_by_entry(A, S, I, B, rows):
    d = dev()
    tables = stacked_tables(S, I, A, 1000 * A + I + B)
    g = torch.Generator().manual_seed(B)
    items, eps = (0.3 * torch.randn(S, I, A + 1, generator=g)).to(d), torch.randn(S, B, A, generator=g).to(d)
    tables_d = tables.to(d)
    ratios = []
    for pattern in ('single', 'few'):
        codes = pattern_rows(pattern, I, B)
        empty = (codes != 2).sum(1) == 0
        assert empty[1] and not (codes[:, I - 1] != 2).any()
        r, m, code = rows_on_device(codes, rows)
        for prior in (False, True):
            spec = ElboSpec(irt_model=2, ability_dim=A, conditional=True, drop_missing=not prior)
            if rows == 'codes':      # (from 3 dims the library leaves cell codes to the loop unless the stacked form is pinned)
                assert (lib_query(spec, r, m, code, B, S) > 0) == (A <= 2)
            with ops.desc_flags(_lib.FLAG_COND_MATRIX if rows == 'codes' else ops.DESC_FLAGS):
                _, post = multi_cond(spec, r, m, code, None, tables_d, items, eps, None, B)
            post = post.cpu()
            tag = f'multi_cond/{rows}/B{B}/I{I}' + ('/prior' if prior else '')
            for s in range(S):
                mu, lv = post[s, :, :A], post[s, :, A:]
                keep = np.ones(B, bool) if prior else ~empty
                if not prior:      # no expert at all: 0 / 0 and log(1 / 0), as vibo_encode and the reference
                    assert bool(torch.isnan(mu[empty]).all()) and bool(torch.isinf(lv[empty]).all())
                with np.errstate(all='ignore'):      # (the person without an expert: 0 / 0 in the reference too, not compared)
                    mu_ref, lv_ref, mu_b, lv_b = OH._posterior_bounds(poe64(codes, tables[s]), I, prior, 'encode', 1)
                    mu_err, lv_err = np.abs(mu.double().numpy() - mu_ref), np.abs(lv.double().numpy() - lv_ref)
                ratios.append(OH._hold('cond', tag, f'A{A}', pattern, f'mu[{s}]', mu_err[keep], mu_b[keep]))
                ratios.append(OH._hold('cond', tag, f'A{A}', pattern, f'logvar[{s}]', lv_err[keep], np.broadcast_to(lv_b, lv_ref.shape)[keep]))
                if pattern == 'single':      # one term summed with zeros: exact whatever the column group
                    with ops.desc_flags(_lib.FLAG_COND_MATRIX if rows == 'codes' else ops.DESC_FLAGS):
                        e_mu, e_lv = ops._hip_encode(spec, r, m, code, None, tables_d[s], B)
                    torch.cuda.synchronize()
                    k = torch.from_numpy(keep)
                    OH._same_bits('cond', tag, f'A{A}', pattern, f'mu[{s}] = vibo_encode', mu[k], e_mu.cpu()[k])
                    OH._same_bits('cond', tag, f'A{A}', pattern, f'logvar[{s}] = vibo_encode', lv[k], e_lv.cpu()[k])
                    if not prior:
                        assert bool(torch.isnan(e_mu.cpu()[empty]).all())
    assert max(ratios) <= 1.0, (A, I, B, rows, max(ratios))


@pytest.mark.parametrize('A', [3, 5])
@pytest.mark.parametrize('prior', [False, True])
def test_samples_do_not_leak_into_each_other(A, prior):
    """2A = 6 and 10: a sample's columns straddle the 16-column tiles.  posterior_out[s] of the stacked call, of the call with
    that sample alone and of the call with the samples in reversed order are the same bits."""
    S, I, B, d = dict(SAMPLES)[A], 200, 65, dev()
    codes = pattern_rows('few', I, B)
    r, m, code = rows_on_device(codes, 'fp32')
    tables = stacked_tables(S, I, A, 7 * A).to(d)
    g = torch.Generator().manual_seed(A)
    items, eps = (0.3 * torch.randn(S, I, A + 1, generator=g)).to(d), torch.randn(S, B, A, generator=g).to(d)
    spec = ElboSpec(irt_model=2, ability_dim=A, conditional=True, drop_missing=not prior)
    bits = lambda t: t.cpu().view(torch.int32)          # (the empty person's NaN compares as bits too)
    sc, post = multi_cond(spec, r, m, code, None, tables, items, eps, None, B)
    sc_r, post_r = multi_cond(spec, r, m, code, None, tables.flip(0).contiguous(), items.flip(0).contiguous(), eps.flip(0).contiguous(), None, B)
    assert torch.equal(bits(post_r.flip(0)), bits(post))
    for s in range(S):
        sc_1, post_1 = multi_cond(spec, r, m, code, None, tables[s:s + 1].contiguous(), items[s:s + 1].contiguous(), eps[s:s + 1].contiguous(),
                                  None, B)
        assert torch.equal(bits(post_1[0]), bits(post[s])), s


# ---------------------------------------------------------------------------
# the heads
# ---------------------------------------------------------------------------
def cond_problem(irt, A, B, I, S, n_flows, seed):
    """Host tensors: rows, S encoder tables / item samples / noise blocks, flows (uhat | w | b) as the model packs them."""
    resp, mask, _, _, _ = random_problem(irt, A, B, I, 0.15, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    D = ElboSpec(irt_model=irt, ability_dim=A).item_dim
    tables = (0.7 * torch.randn(S, 2, I, 2 * A, generator=g)).contiguous()
    items = torch.randn(S, I, D, generator=g)
    eps = torch.randn(S, B, A, generator=g)
    flow = None
    if n_flows:
        raw = torch.randn(n_flows, 2 * A + 1, generator=g) * 0.5
        flow = torch.stack([torch.cat([T.flow_uhat(f[:A], f[A:2 * A]), f[A:]]) for f in raw])
    return resp, mask, tables, items, eps, flow


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
    # irt, A, B, I, S, flows, rows
    (2, 1, 13, 95, 5, 0, 'padded'),         # 95 items in rows of 96, one contraction pass
    (2, 8, 33, 1000, 5, 0, 'fp32'),         # tight stride; 4 + 1 samples: COUNT form, then one tile
    (3, 2, 21, 600, 4, 2, 'codes'),         # the caller's cell codes, 3PL, flows
    (1, 4, 9, 332, 3, 0, 'gather'),         # row_index into a 40-row matrix: packed in minibatch order
    (2, 3, 17, 1100, 11, 0, 'fp32'),        # two panels of the GIVEN kernel; 10 + 1 samples
    (2, 5, 10, 200, 3, 2, 'nomask'),
    (2, 2, 12, 128, 6, 0, 'codes_gather'),  # cell codes through row_index in every pass
]


@pytest.mark.parametrize('irt,A,B,I,S,n_flows,rows', CASES)
def test_heads_equal_the_oracle_and_single_launches(irt, A, B, I, S, n_flows, rows):
    spec = ElboSpec(irt_model=irt, ability_dim=A, conditional=True, n_flows=n_flows)
    resp, mask, tables, items, eps, flow = cond_problem(irt, A, B, I, S, n_flows, seed=S * 100 + I)
    d = dev()
    if rows == 'nomask':      # every cell answered: the simulated rows hold -1 at their missing cells, which no kernel reads as an answer
        resp, mask = resp.clamp_min(0.0), torch.ones_like(mask)
    if rows == 'codes_gather':
        big_r, big_m, where = scattered_rows(resp, mask, 40)
        r, m, code = ops.prepare_rows(ops.pack_cell_codes(big_r.to(d), big_m.to(d)), None)
        ri = where.to(d)
    else:
        r, m, code, ri = device_rows(resp, mask, rows)
    fl = flow.to(d).contiguous() if flow is not None else None
    tables_d, items_d, eps_d = tables.to(d), items.to(d), eps.to(d)
    sc = ops._hip_multi_forward(spec, r, m, code, ri, tables_d, items_d, eps_d, fl, _lib.REG_SAMPLED, B)
    torch.cuda.synchronize()
    assert sc is not None and tuple(sc.shape) == (S, _lib.NUM_SCALARS)          # (None before this call existed)
    sc2, _ = multi_cond(spec, r, m, code, ri, tables_d, items_d, eps_d, fl, B)
    assert torch.equal(sc, sc2)                                                  # with or without posterior_out
    flows64 = [(f[:A].double(), f[A:2 * A].double(), f[2 * A:].double()) for f in flow] if n_flows else None
    worst = 0.0
    for s in range(S):
        a = sc[s, :7].cpu().double()
        ref = T.fused_elbo_ref(tables[s].double(), items[s].double(), resp.double(), mask, eps[s].double(), irt_model=irt, ability_dim=A,
                               conditional_posterior=True, mode='sampled', flow_uhat_w_b=flows64, want_grad=False)
        want = torch.stack([ref['ll'], ref['reg'], ref['kl_ability'], ref['logq0'], ref['logp'], ref['ladj_sum'],
                            torch.tensor(float(B * I), dtype=torch.float64)])          # (GIVEN conventions: NOBS = B I)
        err = float(((a - want).abs() / want.abs().clamp_min(1.0)).max())
        record('multi_cond:oracle', err, TOL_ELBO, sample=s)
        print('multi_cond: sample %d |multi - oracle| / max(1, |ref|) = %.3g' % (s, err))
        assert err < TOL_ELBO, (s, a, want)
        one = ops._hip_launch_elbo(spec, r, m, code, ri, tables_d[s], items_d[s].contiguous(), eps_d[s].contiguous(), fl,
                                   _lib.REG_SAMPLED, False, B)
        b = one.scalars[:6].cpu().double()                                             # (its NOBS counts the observed cells)
        e1 = float((a[:6] - b).abs().max()) / max(1.0, float(b.abs().max()))
        worst = max(worst, e1)
        record('multi_cond:single', e1, TOL_SINGLE, sample=s, panels=(I + 1023) // 1024)
        assert e1 < TOL_SINGLE, (s, a, b)
    print('multi_cond: max |multi - single| / max(1, |head|) = %.3g over %d samples' % (worst, S))


def test_bad_calls_are_refused_without_a_launch():
    lib = _lib.load()
    irt, A, B, I, S = 2, 2, 11, 100, 3
    resp, mask, tables, items, eps, _ = cond_problem(irt, A, B, I, S, 0, seed=5)
    d = dev()
    tables_d, items_d, eps_d = tables.to(d), items.to(d), eps.to(d)
    out = torch.full((S, _lib.NUM_SCALARS), 7.0, device=d)
    post = torch.full((S, B, 2 * A), 7.0, device=d)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=d)

    def call(spec, r, m, code, num_samples=S, ability_dim=None, null=None, fn='vibo_elbo_multi_forward_cond'):
        desc = ops._rows_desc(spec, B, r, m, code, _lib.REG_SAMPLED, False)
        if ability_dim is not None:
            desc.ability_dim = ability_dim
        p = dict(tables=ops._ptr(tables_d), item=ops._ptr(items_d), eps=ops._ptr(eps_d), out=ops._ptr(out), response=ops._ptr(r))
        if null:
            p[null] = None
        args = [ctypes.byref(desc), num_samples, p['response'], ops._ptr(m), None, p['tables'], p['item'], p['eps'], None, p['out']]
        if fn == 'vibo_elbo_multi_forward_cond':
            args.append(ops._ptr(post))
        rc = getattr(lib, fn)(*args, ops._ptr(ws), ctypes.c_size_t(ws.numel()), ops._stream(d))
        return rc, lib.vibo_last_error_string().decode()

    cond = ElboSpec(irt_model=irt, ability_dim=A, conditional=True)
    r, m, code = ops.prepare_rows(resp.to(d), mask.bool().to(d))
    desc = ops._rows_desc(cond, B, r, m, code, _lib.REG_SAMPLED, False)
    assert 0 < lib.vibo_multi_cond_workspace_bytes(ctypes.byref(desc), S) <= ws.numel()
    assert lib.vibo_multi_cond_workspace_bytes(ctypes.byref(desc), 0) == 0
    # a descriptor that is not conditional
    assert call(ElboSpec(irt_model=irt, ability_dim=A), r, m, code)[0] == -3
    assert call(ElboSpec(irt_model=irt, ability_dim=A, given=True), r, m, code)[0] == -3
    # outside the shapes: -8, and the query answers 0 so that callers keep looping
    r64, m64, code64 = ops.prepare_rows(resp.to(d), mask.long().to(d), keep_int64=True)
    assert code64 == _lib.MASK_I64 and call(cond, r64, m64, code64)[0] == -8
    assert lib.vibo_multi_cond_workspace_bytes(ctypes.byref(ops._rows_desc(cond, B, r64, m64, code64, _lib.REG_SAMPLED, False)), S) == 0
    assert ops._hip_multi_forward(cond, r64, m64, code64, None, tables_d, items_d, eps_d, None, _lib.REG_SAMPLED, B) is None
    assert call(cond, r, m, code, ability_dim=12)[0] == -8
    # cell codes from 3 dims: measured slower than the loop (profiles/r09_multi_cond.txt); VIBO_FLAG_COND_MATRIX pins the call
    cc = ops.prepare_rows(ops.pack_cell_codes(resp.to(d), mask.bool().to(d)), None)
    assert lib_query(cond, *cc, B, S) > 0          # (2 dims on cell codes: covered; it runs at the end)
    cond3 = ElboSpec(irt_model=irt, ability_dim=A, conditional=True)
    assert call(cond3, *cc, ability_dim=3)[0] == -8 and 'VIBO_FLAG_COND_MATRIX' in call(cond3, *cc, ability_dim=3)[1]
    with ops.desc_flags(_lib.FLAG_COND_MATRIX):
        d3 = ops._rows_desc(cond3, B, *cc, _lib.REG_SAMPLED, False)
    d3.ability_dim = 3
    assert lib.vibo_multi_cond_workspace_bytes(ctypes.byref(d3), S) > 0
    d3.flags = 0
    assert lib.vibo_multi_cond_workspace_bytes(ctypes.byref(d3), S) == 0
    assert call(cond, r, m, code, num_samples=0)[0] == -3
    for null in ('tables', 'item', 'eps', 'out', 'response'):
        assert call(cond, r, m, code, null=null)[0] == -5, null
    # rows that are not on the device: None, nothing raised
    assert ops._hip_multi_forward(cond, resp, mask.to(torch.uint8), _lib.MASK_U8, None, tables, items, eps, None, _lib.REG_SAMPLED, B) is None
    # vibo_elbo_multi_forward keeps refusing conditional descriptors
    assert call(cond, r, m, code, fn='vibo_elbo_multi_forward')[0] == -8
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((post == 7.0).all())          # nothing ran, after every refusal above
    for rows in ((r, m, code), cc):                                          # ... and the same buffers are written by a call that is taken
        out.fill_(7.0)
        post.fill_(7.0)
        assert call(cond, *rows)[0] == 0
        torch.cuda.synchronize()
        assert bool((out[:, :7] != 7.0).any()) and bool((post != 7.0).all())


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------
def module_case(kind):
    d = dev()
    torch.manual_seed(31)
    B = 24
    if kind == '3pl_a1_flows2':
        model, irt, A, I = VIBO_3PL(1, 95, ability_merge='product', conditional_posterior=True, n_norm_flows=2), 3, 1, 95
    else:
        model, irt, A, I = VIBO_2PL(5, 100, ability_merge='product', conditional_posterior=True, replace_missing_with_prior=False), 2, 5, 100
    resp, mask, _, _, _ = random_problem(irt, A, B, I, 0.2, seed=I + A)
    return model.to(d), resp.to(d), mask.bool().to(d)


def loop_value(model, resp, mask, eps_item, eps_ab):
    """log_marginal's loop formula (models.py:445-504) from the heads of one single conditional launch per sample."""
    S, B = eps_item.shape[0], resp.shape[0]
    r, m, code = ops.prepare_rows(*ops.pad_rows(resp, mask))
    with torch.no_grad():
        item_mu, item_lv = model.item_encoder()
        fl = model.ability_norm_flows.packed() if model.n_norm_flows else None
        log_w = []
        for s in range(S):
            feat = eps_item[s] * torch.exp(0.5 * item_lv) + item_mu
            lq = _normal_logpdf(feat, item_mu, item_lv).sum()
            item_k = feat
            if model.n_norm_flows:
                item_k, item_ladj = model.item_norm_flows(feat)
                lq = lq - item_ladj.sum()
            table = model.ability_encoder.expert_table(feat)
            one = ops._hip_launch_elbo(model.spec, r, m, code, None, table.contiguous(), item_k.contiguous(), eps_ab[s].contiguous(), fl,
                                       _lib.REG_SAMPLED, False, B)
            log_w.append(one.scalars[_lib.S_LL] - one.scalars[_lib.S_REG] + _std_normal_logpdf(item_k).sum() - lq)
        return float(torch.logsumexp(torch.stack(log_w), 0)) - float(torch.log(torch.tensor(float(S))))


@pytest.mark.parametrize('kind', ['3pl_a1_flows2', '2pl_a5_drop'])
def test_log_marginal_runs_no_single_launch_forward(kind):
    model, resp, mask = module_case(kind)
    d, S, B = dev(), 6, resp.shape[0]
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
        replayed = float(model.log_marginal(resp, mask, num_samples=S, eps_item=eps_item, eps_ability=eps_ab))
        assert abs(replayed - want) < 1e-5 * max(1.0, abs(want)), (replayed, want)
        torch.manual_seed(12)
        drawn = float(model.log_marginal(resp, mask, num_samples=S))
        assert abs(drawn - want) < 1e-5 * max(1.0, abs(want)), (drawn, want)          # the draw order is the loop's
        ops._BACKEND['elbo'] = saved['elbo']
        ops._BACKEND['multi'] = lambda *a: None
        torch.manual_seed(12)
        looped = float(model.log_marginal(resp, mask, num_samples=S))
        assert abs(drawn - looped) < 1e-5 * max(1.0, abs(looped)), (drawn, looped)
    finally:
        ops._BACKEND.update(saved)


def test_conditional_golden_through_one_multi_sample_call():
    g = Golden(os.path.join(GOLDEN_DIR, 'logmarg_3pl_a1_cond_flows2.npz'))
    d = dev()
    model = build_model(g).to(d)
    calls, singles = [], []
    saved = dict(ops._BACKEND)
    try:
        ops._BACKEND['multi'] = lambda *a: calls.append(1) or saved['multi'](*a)
        ops._BACKEND['elbo'] = lambda *a, **k: singles.append(1) or saved['elbo'](*a, **k)
        logp = model.log_marginal(g.response.to(d).unsqueeze(2), g.mask.to(d).bool().unsqueeze(2),
                                  num_samples=g.meta['num_samples'], eps_item=g.eps_item.to(d), eps_ability=g.eps_ability.to(d))
    finally:
        ops._BACKEND.update(saved)
    ref = float(g.out['logp'])
    assert len(calls) == 1 and singles == [] and abs(float(logp) - ref) < 1e-4 * max(1.0, abs(ref))


def test_declined_shapes_are_turned_back_before_anything_is_prepared():
    """Cell codes at 5 dims: the workspace query answers 0, so log_marginal asks it (ops.multi_forward_declined) before it draws or
    stacks anything and runs the plain loop -- no 'multi' call is prepared -- with the loop's number; with the stacked call pinned
    (VIBO_FLAG_COND_MATRIX) the same seeded call goes through it and agrees."""
    model, resp, mask = module_case('2pl_a5_drop')
    cc = ops.pack_cell_codes(resp, mask)
    r, m, code = ops.prepare_rows(cc, None)
    S, B = 6, resp.shape[0]
    assert ops.multi_forward_declined(model.spec, r, m, code, S, B)
    assert not ops.multi_forward_declined(model.spec, *ops.prepare_rows(resp, mask), S, B)
    stacked = []
    inner = model.ability_encoder.expert_table
    model.ability_encoder.expert_table = lambda feat=None: stacked.append(1) or inner(feat)
    torch.manual_seed(12)
    looped = float(model.log_marginal(cc, None, num_samples=S))
    assert len(stacked) == S                      # one table per sample, in the loop: none computed for a stack first
    with ops.desc_flags(_lib.FLAG_COND_MATRIX):
        assert not ops.multi_forward_declined(model.spec, r, m, code, S, B)
        torch.manual_seed(12)
        pinned = float(model.log_marginal(cc, None, num_samples=S))
    assert abs(pinned - looped) < 1e-5 * max(1.0, abs(looped)), (pinned, looped)
