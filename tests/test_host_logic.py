"""Host logic of the drop-in modules on CPU: state_dict compatibility with the
reference, loss / gradient composition around the fused op, the reference call
pattern ``model.elbo(*model(response, mask))`` -- with the native entry points
replaced by the CPU analytic restatement (oracle/cpu_backend.py).  The same
assertions run against the real HIP kernel in tests/test_gpu_parity.py."""
import pytest
import torch

import os

from conftest import GOLDEN_DIR, Golden, rel_err
from golden_common import build_model, check_against_golden, run_reference_pattern
from oracle import cpu_backend
from oracle import vibo_oracle as O
from oracle import vibo_table_ref as T
from vibo_amd import ops
from vibo_amd.torch_core.models import DeferredResponseMu


@pytest.fixture()
def cpu_ops():
    restore = cpu_backend.install(ops)
    yield
    restore()


def test_state_dict_keys_match_reference(golden):
    model = build_model(golden)
    assert list(model.state_dict().keys()) == list(golden.sd.keys())


def test_reference_call_pattern_matches_golden(cpu_ops, golden):
    model = build_model(golden)
    outs, loss = run_reference_pattern(model, golden)
    assert isinstance(outs[2], DeferredResponseMu)
    check_against_golden(model, golden, outs, loss)


def test_mask_dtypes_equivalent(cpu_ops, golden):
    model = build_model(golden)
    _, l_i64 = run_reference_pattern(model, golden, torch.int64)
    _, l_bool = run_reference_pattern(model, golden, torch.bool)
    _, l_u8 = run_reference_pattern(model, golden, torch.uint8)
    assert float(l_i64.detach()) == float(l_bool.detach()) == float(l_u8.detach())


def test_cell_codes_rows_match_golden(cpu_ops, golden):
    """Format P host plumbing (ops.CellCodes -> prepare_rows -> VIBO_MASK_CODES): the goldens fed as one byte per cell."""
    model = build_model(golden)
    mask = golden.mask != 0
    I = golden.response.shape[1]
    padded = torch.full((golden.response.shape[0], (I + 3) // 4 * 4), 2, dtype=torch.uint8)
    padded[:, :I] = torch.where(mask, (golden.response == 1).to(torch.uint8), torch.full_like(mask, 2, dtype=torch.uint8))
    codes = ops.CellCodes(padded[:, :I])
    r2, m2 = codes.unpack()
    assert torch.equal(m2, mask) and torch.equal(r2[m2], golden.response[m2])
    assert torch.equal(codes.rows(torch.tensor([1, 0])).codes, codes.codes[[1, 0]])
    with pytest.raises(ValueError):
        ops.prepare_rows(codes, mask)
    with pytest.raises(ValueError):
        ops.CellCodes(padded[:, :I].float())
    m = golden.meta
    outs = model(codes, None, eps_item=golden.eps_item, eps_ability=golden.eps_ability)
    if m['n_norm_flows'] > 0:
        (r, k, rmu, ak, a0, amu, alv, aladj, ik, i0, imu, ilv, iladj) = outs
        loss = model.elbo(r, k, rmu, a0, amu, alv, i0, imu, ilv, annealing_factor=m['annealing_factor'],
                          use_kl_divergence=False, ability_k=ak, item_feat_k=ik,
                          ability_logabsdetjac=aladj, item_logabsdetjac=iladj)
    else:
        loss = model.elbo(*outs, annealing_factor=m['annealing_factor'], use_kl_divergence=m['use_kl_divergence'])
    check_against_golden(model, golden, outs, loss)


def test_decode_and_deferred_response_mu(cpu_ops, golden):
    model = build_model(golden)
    outs, _ = run_reference_pattern(model, golden)
    rmu = outs[2].materialize()
    assert rmu.shape == (golden.meta['num_person'], golden.meta['num_item'], 1)
    assert (rmu.squeeze(2) - golden.out['response_mu']).abs().max() < 1e-5


def test_table_ref_matches_autograd_oracle(golden):
    """The analytic backward the kernel implements == autograd through the naive oracle."""
    cfg = golden.cfg
    if cfg['n_norm_flows'] > 0:
        mode = 'sampled'
    else:
        mode = 'kl' if cfg['use_kl_divergence'] else 'sampled'
    sd = {k: v.double() for k, v in golden.sd.items()}
    A = cfg['ability_dim']
    item_mu, item_lv = sd['item_encoder.mu_lookup.weight'], sd['item_encoder.logvar_lookup.weight']
    item_feat = golden.eps_item.double() * torch.exp(0.5 * item_lv) + item_mu
    flows = None
    item_k = item_feat
    if cfg['n_norm_flows'] > 0:
        flows = [(T.flow_uhat(sd[f'ability_norm_flows.flows.{k}.u'], sd[f'ability_norm_flows.flows.{k}.w']),
                  sd[f'ability_norm_flows.flows.{k}.w'], sd[f'ability_norm_flows.flows.{k}.b'])
                 for k in range(cfg['n_norm_flows'])]
        item_k, _ = O.planar_flows(sd, 'item_norm_flows', item_feat, cfg['n_norm_flows'])
    mean = golden.meta.get('ability_merge', 'product') == 'mean'
    if mean:      # the kernel takes the per-person posterior as given (VIBO_POSTERIOR_GIVEN): table = [B, 2A]
        table = torch.cat(O.ability_posterior(sd, golden.response.double(), golden.mask, item_feat, ability_dim=A,
                                              conditional_posterior=cfg['conditional_posterior'],
                                              replace_missing_with_prior=True), dim=1)
        table = table.detach().requires_grad_(True)
    else:
        table = T.encoder_table(sd, item_feat, cfg['conditional_posterior']).detach().requires_grad_(True)
    item_leaf = item_k.detach().requires_grad_(True)
    out = T.fused_elbo_ref(table.detach(), item_leaf.detach(), golden.response.double(), golden.mask,
                           golden.eps_ability.double(), irt_model=cfg['irt_model'], ability_dim=A,
                           conditional_posterior=cfg['conditional_posterior'] and not mean,
                           replace_missing_with_prior=cfg['replace_missing_with_prior'], mode=mode,
                           flow_uhat_w_b=flows, exact_saturation=False, given_posterior=mean)

    # autograd version of the same heads from the op-by-op oracle pieces
    B, I = golden.response.shape
    resp, mask = golden.response.double(), golden.mask
    x = (resp == 1).long()
    k = (mask != 0).double().unsqueeze(2)
    if mean:
        m = s = None
    elif cfg['conditional_posterior']:
        idx = torch.arange(I).unsqueeze(0).expand(B, I)
        m, s = table[x, idx, :A], table[x, idx, A:]
    else:
        m, s = table[x][..., :A], table[x][..., A:]
    if mean:
        amu, alv = table[:, :A], table[:, A:]
    elif cfg['replace_missing_with_prior']:
        amu, alv = O.product_of_experts((m * k).permute(1, 0, 2), (s * k).permute(1, 0, 2))
    else:
        amu, alv = O.product_of_experts(m.permute(1, 0, 2), s.permute(1, 0, 2), weight=k.permute(1, 0, 2))
    theta0 = golden.eps_ability.double() * torch.exp(0.5 * alv) + amu
    theta, ladj = theta0, torch.zeros(B, dtype=torch.float64)
    if flows:
        for (uhat, w, b) in flows:
            t = torch.tanh(theta @ w + b)
            ladj = ladj + torch.log(torch.abs(1 + (1 - t * t) * torch.dot(w, uhat)) + 1e-8)
            theta = theta + uhat.unsqueeze(0) * t.unsqueeze(1)
    probs = O.irt_link(cfg['irt_model'], theta, item_leaf)
    ll = O.masked_bernoulli_ll(resp, mask, probs).sum()
    if mode == 'kl':
        reg = O.kl_std_normal(amu, alv).sum()
    else:
        reg = O.normal_logpdf(theta0, amu, alv).sum() - ladj.sum() - O.std_normal_logpdf(theta).sum()
    if mean and cfg['irt_model'] == 3 and float(out['logit'].abs().max()) > 12.0:
        # 3PL clamps p itself at fp32 eps (utils.py:46-49 through torch's Bernoulli): inside that band the fp64 autograd
        # oracle (clamp at fp64 eps) is not the same function; the saturation golden covers the band
        pytest.skip('saturated 3PL logits: analytic-vs-autograd identity does not apply')
    assert rel_err(out['ll'], ll.detach()) < 1e-9
    assert rel_err(out['reg'], reg.detach()) < 1e-9
    g_t0, g_i0 = torch.autograd.grad(ll, [table, item_leaf], retain_graph=True)
    g_t1, = torch.autograd.grad(reg, [table], retain_graph=True)
    assert rel_err(out['g_table'][0], g_t0) < 1e-8
    assert rel_err(out['g_table'][1], g_t1) < 1e-8
    assert rel_err(out['g_item'], g_i0) < 1e-8


@pytest.mark.parametrize('name', ['logmarg_2pl_a2', 'logmarg_3pl_a1_cond_flows2'])
def test_log_marginal_matches_reference_golden(name, cpu_ops):
    """model.log_marginal (models.py:445-504) under the reference's recorded noise sequence; host logic on the CPU
    stand-in backend (one forward per sample)."""
    g = Golden(os.path.join(GOLDEN_DIR, name + '.npz'))
    model = build_model(g)
    logp = model.log_marginal(g.response.unsqueeze(2), g.mask.long().unsqueeze(2), num_samples=g.meta['num_samples'],
                              eps_item=g.eps_item, eps_ability=g.eps_ability)
    ref = float(g.out['logp'])
    assert abs(float(logp) - ref) < 1e-4 * max(1.0, abs(ref))


def test_elbo_accepts_a_materialised_response_mu_and_reruns_with_the_row_index(cpu_ops=None):
    """(a) a caller that builds response_mu through decode() before elbo() (the reference's predictive code does) gets the
    fused step's loss; (b) elbo(use_kl_divergence=False) after a KL-mode forward on gathered rows re-runs the step on the
    same rows with the same item noise."""
    from oracle import cpu_backend
    from vibo_amd import ops
    from vibo_amd.torch_core.models import VIBO_2PL
    restore = cpu_backend.install(ops)
    try:
        torch.manual_seed(3)
        B, I, A = 40, 24, 2
        model = VIBO_2PL(A, I, ability_merge='product')
        resp = (torch.rand(B, I) < 0.5).float()
        mask = torch.rand(B, I) > 0.2
        rows = torch.tensor([5, 1, 17, 30, 2, 9, 11, 39])
        outs = model(resp, mask, row_index=rows)
        loss_a = model.elbo(*outs)
        rmu = model.decode(outs[3], outs[6])
        loss_b = model.elbo(outs[0], outs[1], rmu, *outs[3:])
        assert torch.equal(loss_a, loss_b)
        # KL-mode forward, sampled-mode elbo with gradients on: the step is redone on the SAME rows and item noise
        loss_c = model.elbo(*outs, use_kl_divergence=False)
        eps_i = model._last_ctx.eps_item
        outs2 = model(resp[rows], mask[rows], eps_item=eps_i, eps_ability=model._last_ctx.eps_ability)
        loss_d = model.elbo(*outs2, use_kl_divergence=False)
        assert abs(float(loss_c) - float(loss_d)) <= 1e-4 * abs(float(loss_d))
    finally:
        restore()


# ---------------------------------------------------------------------------
# the resident-matrix record of ops.py (ops.ResidentMatrix, ops._lookup_counts) on CPU tensors: every count goes through
# ops._BACKEND['counts'], so the launches are counted by wrapping that entry around the CPU oracle's
# ---------------------------------------------------------------------------
@pytest.fixture()
def count_calls(cpu_ops):
    calls = []
    inner = ops._BACKEND['counts']
    ops._BACKEND['counts'] = lambda *a: (calls.append(a[3]), inner(*a))[1]
    yield calls
    ops._BACKEND['counts'] = inner


def _matrix(P=12, I=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, I, generator=g) < 0.5).float(), torch.rand(P, I, generator=g) > 0.2


class _FakeStream:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def record_event(self):
        self.log.append(('record', self.name))
        return 'event of ' + self.name

    def wait_event(self, event):
        self.log.append(('wait', self.name, event))


def _elbo_lookup(resp, mask, row_index=None, B=None, capturing=False, stream=_FakeStream([], 'a stream')):
    """ops._lookup_counts as the ELBO launch calls it (ops._resident_row_counts behind its early-outs)."""
    r, m, code = ops.prepare_rows(resp, mask)
    B = (r.shape[0] if row_index is None else int(row_index.numel())) if B is None else B
    return ops._lookup_counts(r, None if isinstance(resp, ops.CellCodes) else m, (r, m, code), row_index, B,
                              for_elbo=True, capturing=lambda: capturing, stream=stream)


def _expected_counts(resp, mask):
    return (((resp == 1) & mask).sum(1).to(torch.int32) << 16) | mask.sum(1).to(torch.int32)


def test_resident_record_never_confuses_a_dead_mask_with_no_mask(count_calls):
    """ADVICE round 6, finding 2: a record made with a mask whose tensor has since been freed must not match mask=None (the
    masked counts would serve an unmasked call), nor a record made without a mask a call with one."""
    import gc
    resp, mask = _matrix()
    ops.row_counts(resp, mask)
    rec = resp._vibo_row_counts
    assert rec.has_mask and rec.counts is not None and rec.is_(resp, mask)
    del mask
    gc.collect()
    assert rec.mask.ref() is None and not rec.is_(resp, None)
    assert torch.equal(ops.row_counts(resp, None), _expected_counts(resp, torch.ones_like(resp, dtype=torch.bool)))
    assert len(count_calls) == 2
    rec = resp._vibo_row_counts
    assert not rec.has_mask and rec.is_(resp, None) and not rec.is_(resp, _matrix(seed=1)[1])
    assert _elbo_lookup(resp, _matrix(seed=1)[1]) is None and len(count_calls) == 2      # recorded without a mask, looked up with one: a first sighting


@pytest.mark.parametrize('edit', ['response', 'mask'])
def test_resident_record_misses_after_an_in_place_edit(count_calls, edit):
    resp, mask = _matrix()
    assert _elbo_lookup(resp, mask) is None and _elbo_lookup(resp, mask) is not None and len(count_calls) == 1
    if edit == 'response':
        resp[3, :] = 1.0
    else:
        mask[3, :] = False
    assert not resp._vibo_row_counts.is_(resp, mask)
    assert _elbo_lookup(resp, mask) is None and len(count_calls) == 1          # a first sighting again: the kernel counts
    got = _elbo_lookup(resp, mask)                                               # the next one counts the matrix as it is now
    assert len(count_calls) == 2 and torch.equal(got, _expected_counts(resp, mask))


def test_elbo_lookup_policy_eager_and_capturing(count_calls):
    """First sighting: recorded only.  Second: one whole-matrix count.  From then on: served.  While capturing (ADVICE round 6,
    finding 1): never with row_index=None -- the captured input is the matrix, a replay has to count what is there then --, with a
    row_index yes, and nothing is counted."""
    resp, mask = _matrix()
    rows = torch.tensor([5, 1, 7])
    assert _elbo_lookup(resp, mask, capturing=True) is None and count_calls == []
    assert _elbo_lookup(resp, mask, rows, capturing=True) is None and count_calls == []      # capturing, no counts yet: nothing is counted
    cnt = _elbo_lookup(resp, mask)
    assert count_calls == [None] and torch.equal(cnt, _expected_counts(resp, mask))
    assert _elbo_lookup(resp, mask) is cnt and _elbo_lookup(resp, mask, rows) is cnt and count_calls == [None]
    assert _elbo_lookup(resp, mask, capturing=True) is None
    assert _elbo_lookup(resp, mask, rows, capturing=True) is cnt and count_calls == [None]


def test_elbo_lookup_counts_nothing_it_would_throw_away(count_calls):
    """ADVICE round 6, finding 3: row_index=None on fewer persons than the matrix has rows uses no whole-matrix counts."""
    resp, mask = _matrix()
    for _ in range(3):
        assert _elbo_lookup(resp, mask, B=5) is None
    assert count_calls == [] and not hasattr(resp, '_vibo_row_counts')


def test_counts_are_ordered_behind_their_stream(count_calls):
    """ADVICE round 6, finding 3: the counts remember their stream and an event; a consumer on another stream waits on it, the same
    stream gets no extra call, a capturing stream (which cannot wait on an eager event) none either."""
    resp, mask = _matrix()
    log = []
    main, side = _FakeStream(log, 'main'), _FakeStream(log, 'side')
    _elbo_lookup(resp, mask, stream=main)
    assert log == []
    _elbo_lookup(resp, mask, stream=main)
    assert log == [('record', 'main')]
    _elbo_lookup(resp, mask, stream=main)
    assert log == [('record', 'main')]
    _elbo_lookup(resp, mask, stream=side)
    assert log == [('record', 'main'), ('wait', 'side', 'event of main')]
    _elbo_lookup(resp, mask, torch.tensor([1, 2]), stream=side, capturing=True)
    assert len(log) == 2 and len(count_calls) == 1


def test_row_counts_launches_per_resident_matrix(count_calls):
    """The sequence of test_gpu_mean_merge.py::test_row_counts_are_cached_per_resident_matrix: the same launch counts."""
    g = torch.Generator().manual_seed(1)
    resp, mask = O.simulate_responses(2, 300, 100, 1, generator=g, missing_frac=0.2)
    mask = mask.bool()
    rows = torch.tensor([5, 7, 299])
    a = ops.row_counts(resp, mask, rows)               # first gathered minibatch of this matrix: those rows only
    a2 = ops.row_counts(resp, mask, rows)              # the matrix came back: counted as a whole, once
    b = ops.row_counts(resp, mask)
    c = ops.row_counts(resp, mask, rows)
    assert len(count_calls) == 2 and torch.equal(a, b[rows]) and torch.equal(a, c) and torch.equal(a, a2)
    mask[5, :] = False                                 # in-place change: counted again
    d_ = ops.row_counts(resp, mask, rows)
    assert len(count_calls) == 3 and int(d_[0]) == 0 and torch.equal(d_[1:], a[1:])
    codes = ops.CellCodes(torch.where(mask, resp.to(torch.uint8), torch.full((), 2, dtype=torch.uint8)))
    e = ops.row_counts(codes, None)
    f = ops.row_counts(codes, None, rows)
    assert len(count_calls) == 4 and torch.equal(e[rows], f) and torch.equal(e, ops.row_counts(resp, mask))
    assert len(count_calls) == 4 and _elbo_lookup(codes, None) is e


@pytest.mark.parametrize('mask_dtype', [torch.bool, torch.int64])
def test_row_counts_and_the_elbo_lookup_recognise_the_same_matrix(count_calls, mask_dtype):
    """row_counts() is called with the caller's tensors, the ELBO launch with prepare_rows()'s: one record serves both."""
    resp, mask = _matrix()
    mask = mask.to(mask_dtype)
    cnt = ops.row_counts(resp, mask)
    assert _elbo_lookup(resp, mask) is cnt and len(count_calls) == 1
    resp2, mask2 = _matrix(seed=2)
    mask2 = mask2.to(mask_dtype)
    _elbo_lookup(resp2, mask2)
    cnt2 = _elbo_lookup(resp2, mask2)
    assert ops.row_counts(resp2, mask2) is cnt2 and torch.equal(ops.row_counts(resp2, mask2, torch.tensor([3])), cnt2[[3]])
    assert len(count_calls) == 2


def test_prepare_mask_narrows_once_per_live_mask():
    import weakref
    for dtype in (torch.bool, torch.int64):
        mask = _matrix()[1].to(dtype)
        a, code = ops.prepare_mask(mask)
        assert code == ops._lib.MASK_U8 and a.dtype == torch.uint8 and ops.prepare_mask(mask)[0] is a
        assert torch.equal(a != 0, mask != 0) and a.stride() == mask.stride()
        mask[0, 0] = 1 - mask[0, 0] if dtype == torch.int64 else ~mask[0, 0]
        b = ops.prepare_mask(mask)[0]
        assert torch.equal(b != 0, mask != 0) and ops.prepare_mask(mask)[0] is b
        if dtype == torch.int64:
            assert b is not a and b.data_ptr() != a.data_ptr()          # a fresh copy after the in-place edit
        else:
            assert b.data_ptr() == mask.data_ptr()                      # read in place
        narrowed, caller = weakref.ref(b), weakref.ref(mask)
        del a, b, mask
        assert narrowed() is None and caller() is None                  # freed with the mask, without the garbage collector
    padded = ops.pad_rows(*_matrix(I=7))[1]                             # strided rows are aliased as they are
    p8 = ops.prepare_mask(padded)[0]
    assert p8.stride() == (8, 1) and p8.data_ptr() == padded.data_ptr() and torch.equal(p8 != 0, padded)


@pytest.mark.parametrize('mask_dtype', [torch.bool, torch.int64])
def test_an_edit_through_the_narrowed_mask_is_a_miss(count_calls, mask_dtype):
    """prepare_rows() hands out the narrowed mask, and that is the tensor a caller of the ELBO launch holds: an in-place edit made
    through it must miss like one made through the caller's own tensor (a bool mask's narrowed form shares its version counter; the
    copy of an int64 mask stops standing for that mask once it has been edited itself)."""
    resp, mask = _matrix()
    mask = mask.to(mask_dtype)
    r, m8, code = ops.prepare_rows(resp, mask)
    look = lambda: ops._lookup_counts(r, m8, (r, m8, code), None, r.shape[0], for_elbo=True, capturing=lambda: False, stream=None)
    assert look() is None and look() is not None and len(count_calls) == 1
    m8[0, :] = 0
    assert not r._vibo_row_counts.is_(r, m8)
    assert look() is None and len(count_calls) == 1
    got = look()
    assert len(count_calls) == 2 and int(got[0]) == 0 and torch.equal(got, _expected_counts(resp, m8 != 0))
    if mask_dtype == torch.int64:
        assert ops.prepare_mask(mask)[0] is not m8          # the edited copy no longer stands for the caller's mask


def test_counts_recorded_into_a_graph_are_not_served_to_the_elbo_launch(count_calls):
    resp, mask = _matrix()
    side = _FakeStream([], 'capturing')
    cnt = ops._lookup_counts(resp, mask, lambda: ops.prepare_rows(resp, mask, keep_int64=True), None, resp.shape[0], for_elbo=False,
                             capturing=lambda: True, stream=side)
    assert cnt is not None and resp._vibo_row_counts.in_graph and side.log == []
    assert _elbo_lookup(resp, mask) is None and _elbo_lookup(resp, mask, torch.tensor([1])) is None and len(count_calls) == 1
    assert ops.row_counts(resp, mask) is cnt


def test_bookkeeping_on_callers_tensors_is_not_saved_with_them(count_calls, tmp_path):
    import copy
    resp, mask = _matrix()
    ops.row_counts(resp, mask)
    ops.prepare_rows(resp, mask.long())
    for k, t in enumerate((resp, mask, ops.prepare_mask(mask)[0])):
        torch.save(t, tmp_path / f'{k}.pt')
        back = torch.load(tmp_path / f'{k}.pt', weights_only=False)
        assert torch.equal(back, t) and not any(vars(back).values()) and not any(vars(copy.deepcopy(t)).values())


def test_chunkable_rows_is_the_one_padding_idiom():
    """ops.chunkable_rows: compact rows whose width is no multiple of 4 come back as padded copies (row stride a multiple of 4, zeros
    behind column I, a row index gathered first and returned as None); everything the kernels can chunk already comes back as it is."""
    g = torch.Generator().manual_seed(31)
    P, I = 13, 95
    resp = (torch.rand(P, I, generator=g) < 0.5).float()
    mask = torch.rand(P, I, generator=g) < 0.8
    idx = torch.tensor([5, 0, 5, 12, 3, 3])

    def check_padded(r, want):
        assert tuple(r.shape) == tuple(want.shape) and torch.equal(r, want) and r.stride(0) % 4 == 0 and r.stride(1) == 1
        whole = r.as_strided((r.shape[0], r.stride(0)), (r.stride(0), 1))
        assert r.stride(0) >= 96 and not whole[:, I:].any()

    for m in (mask, None):
        r2, m2 = ops.chunkable_rows(resp, m)
        check_padded(r2, resp)
        assert (m2 is None) if m is None else (check_padded(m2, ops.prepare_mask(mask)[0]) is None)
        # a row index that permutes and repeats rows: gathered before the padding, gone afterwards
        r3, m3, i3 = ops.chunkable_rows(resp, m, idx)
        check_padded(r3, resp[idx])
        assert i3 is None and ((m3 is None) if m is None else (check_padded(m3, ops.prepare_mask(mask)[0][idx]) is None))
        r4, m4, i4 = ops.chunkable_rows(resp, m, None)
        check_padded(r4, resp)
        assert i4 is None and (m4 is None) == (m is None)
    # [B, I, 1] input as the reference's loaders yield it
    r5, m5 = ops.chunkable_rows(resp.unsqueeze(2), mask.unsqueeze(2))
    check_padded(r5, resp)
    check_padded(m5, ops.prepare_mask(mask)[0])
    # nothing to do: 96-item rows and 95-item views of padded rows are the same storage, mask and row index pass through
    wide_r, wide_m = torch.cat([resp, resp[:, :1]], 1), torch.cat([mask, mask[:, :1]], 1)
    for r, m in ((wide_r, wide_m), (r2, m2), ops.pad_rows(resp, mask)):
        ra, ma, ia = ops.chunkable_rows(r, m, idx)
        assert ra.data_ptr() == r.data_ptr() and ra.stride() == r.stride() and ma is m and ia is idx
        rb, mb = ops.chunkable_rows(r, m)
        assert rb.data_ptr() == r.data_ptr() and mb is m
    codes = ops.CellCodes(torch.zeros(P, 96, dtype=torch.uint8)[:, :I])
    c3 = ops.chunkable_rows(codes, None, idx)
    assert ops.chunkable_rows(codes, None)[0] is codes and c3[0] is codes and c3[1] is None and c3[2] is idx
