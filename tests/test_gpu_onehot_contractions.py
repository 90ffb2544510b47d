"""The one-hot x table contractions of csrc/vibo_cmean.hip (three bf16 pieces on v_mfma_f32_16x16x32_bf16), number by number.

Every other test of these kernels compares a tensor's largest error with a fraction of its max-abs, on N(0, 1) inputs: a lost
third piece (2^-17 of a value, always toward zero) or a piece added into the wrong column group sits under all of them.  Here the
one-hot operand makes the arithmetic checkable exactly: **a person who observes one cell gets that cell's table row back bit for
bit**, sums of up to 16 grid values are exact, and everything else is held, output by output, to a bound that
oracle/onehot_model.py derives from the inputs alone (c 2^-24 sum|terms| with c counted from the kernels' additions, plus an
absolute term for bf16 subnormal pieces; tests/test_onehot_model.py holds the CPU model of the scheme to the same bound and shows
that a model without the third piece leaves it).  No comparison here uses a tensor's max-abs.

Part A -- vibo_code_table_sum_forward / _backward (cm_forward_kernel<4>, cm_backward_wide_kernel) through ops.CodeTableSumFn on
the test's own feature / gradient bits: patterns single / few / isolated, value classes hostile / binades / tiny / grid
(onehot_model.make_pattern / make_values), 63 / 64 / 200 / 1000 items with 2 I persons, tight rows (stride 1000: the 4-byte
aligned path) and rows padded to 16 and to 64 bytes.  `tiny` x single is held to the bound's absolute term (one bf16 subnormal
piece may be flushed), every other single and every grid case is asserted with torch.equal.

Part B -- the conditional posterior through vibo_encode and vibo_elbo_fwd_bwd at ability_dim 1, 2, 4, 5, 8, --drop-missing unless
stated, expert means in [1, 3], logvar in [-6, 0].  The last item is observed by nobody.  Every form of the first pass is pinned
through ops.DESC_FLAGS under the matrix row-split kernel and asserted with vibo_plan_cond_passes (_elbo_forms): cm_forward_kernel<1>
on packed, tight and gathered cell codes (ones column up to 7 dims, COUNT at 8), cm_forward_fp32_kernel (5+ dims), the VALU
cond_pre pass on fp32 rows and on codes, VIBO_FLAG_NO_EMIT_CODES, and the XM == 3 gather inside the matrix kernel (1 dim); the
table-gradient pass follows as the packed form (1 dim), cm_backward_kernel<1> (2, 4), <2> (5, 8) or the VALU cond_post pass.
  * single: ability_mu / ability_logvar are bit-identical across the forms of one entry point (every form writes
    1.0f / (expf(lv) + kPoeEps) and sums one of them with zeros).  vibo_encode's forms: cm_forward_kernel<1> and cond_pre -- its
    wave-per-person fallback (encode_kernel, __expf) takes no row this file builds.  The two entry points finish the posterior
    differently (vibo_encode: s / lam, logf(1 / lam); the matrix kernel: s * (1 / lam), -ln 2 * v_log_f32(lam)) and are each held
    to their own counted bound below, not to each other.
  * single and few against the fp64 product of experts of the fp32 table, person by person (_posterior_bounds):
    |d logvar| <= c u + (the logarithm's 1 ulp), |d mu| <= c u sum|mu tau| / lam, c = c_forward(k) + the roundings of tau (expf 1 ulp =
    2 u, the add, the divide: C_TAU = 4; mu tau: 5) + the finish; the missing-prior cases add the prior term's 2.  S_NOBS is exact.
  * table gradient, KL head, every form: coefficients S1 = mu_p / lam_p, S2 = -(mu_p^2 - (1 - 1 / lam_p) / 2) / lam_p recomputed in
    fp64 from the device's own ability_mu / ability_logvar; every entry within _kl_head_bounds (the issue's
    c u sum_p (|S1 mu| + |S2|) tau^2 e^lv with c counted there); the unobserved item's rows exactly zero.
  * table gradient, both heads, single: the matrix form against the VALU form from the same first pass, entry by entry.

VIBO_TOL_RECORD=path appends one JSON line per comparison (part, form, class / dim, pattern, observable, worst error / bound);
tools/onehot_record_table.py turns the file into profiles/onehot_contraction_record.txt."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gpu_common import dev, launch_elbo, record
from oracle import onehot_model as M
from vibo_amd import _lib, ops
from vibo_amd.ops import ElboSpec

pytestmark = pytest.mark.gpu

U = M.U
LN2 = float(np.log(2.0))
SECOND_ORDER = 1.0 + 2.0 ** -10          # every counted bound is first order in u; this covers the products of two such terms
EPS32 = float(np.float32(1e-8))          # kPoeEps as the kernels hold it


def _hold(part, form, cls, pattern, observable, err, bound):
    """Record the worst err / bound of one observable (a bound of exactly zero admits no error) and return it."""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    assert np.all(np.isfinite(err)), (part, form, cls, pattern, observable)
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    if zero.any() and float(err[zero].max()) > 0:
        ratio = float('inf')
    record('onehot_contraction', err.max() if err.size else 0.0, part=part, form=form, **{'class': cls}, pattern=pattern,
           observable=observable, ratio=ratio)
    print(f'{part} {form:28s} {cls:8s} {pattern:8s} {observable:10s} worst error / bound = {ratio:.3f}')
    return ratio


def _same_bits(part, form, cls, pattern, observable, got, want):
    """torch.equal, recorded as ratio 0 (or inf with the number of differing entries)."""
    same = torch.equal(got, want)
    record('onehot_contraction', 0.0 if same else float((got.double() - want.double()).abs().max()), part=part, form=form,
           **{'class': cls}, pattern=pattern, observable=observable, ratio=0.0 if same else float('inf'), exact=True)
    print(f'{part} {form:28s} {cls:8s} {pattern:8s} {observable:10s} bit for bit: {same}')
    assert same, (part, form, cls, pattern, observable, int((got != want).sum()))


@functools.lru_cache(maxsize=None)
def _pattern(kind, I):
    return M.make_pattern(kind, 2 * I + (1 if kind == 'isolated' else 0), I, 100 + I)


def _code_rows(codes, stride):
    """The codes as device rows of `stride` bytes (padding cells missing), as CellCodes."""
    B, I = codes.shape
    buf = torch.full((B, stride), 2, dtype=torch.uint8, device=dev())
    buf[:, :I] = torch.from_numpy(codes).to(dev())
    return ops.CellCodes(buf[:, :I])


# ---------------------------------------------------------------------------
# Part A
# ---------------------------------------------------------------------------
LAYOUTS = [(63, 64), (64, 64), (200, 200), (1000, 1000), (1000, 1008), (1000, 1024)]      # (items, row stride in bytes)


def _table_sums(cc, X, G):
    """-> (S [B, 64], dX [2, I, 64]) of vibo_code_table_sum_forward / _backward on the fp32 bits of X and G (host tensors)."""
    feat = X.to(dev()).requires_grad_(True)
    S = ops.CodeTableSumFn.apply(feat, cc)
    (dX,) = torch.autograd.grad(S, feat, G.to(dev()))
    torch.cuda.synchronize()
    return S.detach().cpu(), dX.cpu()


@pytest.mark.parametrize('cls', M.CLASSES)
@pytest.mark.parametrize('I,stride', LAYOUTS, ids=[f'I{i}-stride{s}' for i, s in LAYOUTS])
def test_code_table_sums_cell_by_cell(I, stride, cls):
    form = f'<4>/wide I={I} stride={stride}'
    X = torch.from_numpy(M.make_values(cls, (2, I, 64), 7 * I + len(cls)))
    G = torch.from_numpy(M.make_values(cls, (2 * I, 64), 11 * I + len(cls)))
    ratios = []
    for pattern in ('single', 'few'):
        codes = _pattern(pattern, I)
        S, dX = _table_sums(_code_rows(codes, stride), X, G)
        if pattern == 'single' and cls != 'tiny':
            p, i = np.nonzero(codes != 2)
            c = codes[p, i].astype(np.int64)
            _same_bits('A', form, cls, pattern, 'out_sum', S[p], X[c, i])
            _same_bits('A', form, cls, pattern, 'grad_feat', dX[c, i], G[p])
            continue
        S_ref, T, k = M.exact_sum(codes, X.numpy())
        D_ref, TD, kd = M.exact_grad(codes, G.numpy())
        if cls == 'grid':
            _same_bits('A', form, cls, pattern, 'out_sum', S.double(), torch.from_numpy(S_ref))
            _same_bits('A', form, cls, pattern, 'grad_feat', dX.double(), torch.from_numpy(D_ref))
            continue
        ratios.append(_hold('A', form, cls, pattern, 'out_sum', np.abs(S.double().numpy() - S_ref), M.sum_bound(T, k)))
        ratios.append(_hold('A', form, cls, pattern, 'grad_feat', np.abs(dX.double().numpy() - D_ref), M.grad_bound(TD, kd)))
    assert max(ratios, default=0.0) <= 1.0, (form, cls, ratios)


@pytest.mark.parametrize('I,stride', [(63, 64), (1000, 1000)], ids=['I63', 'I1000'])
def test_an_unobserved_item_and_empty_persons_leak_nowhere(I, stride):
    """`isolated`: the last item carries 2^100 in both codes and is observed by nobody; the last three persons observe nothing and
    carry 2^100 as their upstream gradient.  Against the same launch with 1.0 in those places no other output changes by a bit,
    the empty persons' sums and the unobserved item's gradient rows are exactly +0."""
    form = f'<4>/wide I={I} stride={stride}'
    codes = _pattern('isolated', I)
    cc = _code_rows(codes, stride)
    X = torch.from_numpy(M.make_values('hostile', (2, I, 64), I))
    G = torch.from_numpy(M.make_values('hostile', (codes.shape[0], 64), I + 1))
    outs = []
    for big in (1.0, 2.0 ** 100):
        X[:, I - 1, :] = big
        G[-3:, :] = big
        outs.append(_table_sums(cc, X, G))
    (S1, D1), (S2, D2) = outs
    _same_bits('A', form, 'hostile', 'isolated', 'out_sum', S2, S1)
    _same_bits('A', form, 'hostile', 'isolated', 'grad_feat', D2, D1)
    zero = torch.zeros(3, 64, dtype=torch.int32)
    assert torch.equal(S2[-3:].view(torch.int32), zero), 'a person without observed cells must get exactly +0'
    assert bool((D2[:, I - 1] == 0).all()), 'an unobserved item must get exactly zero'
    p, i = np.nonzero(codes != 2)
    _same_bits('A', form, 'hostile', 'isolated', 'rows', S2[p], X[codes[p, i].astype(np.int64), i])


# ---------------------------------------------------------------------------
# Part B
# ---------------------------------------------------------------------------
KM, CM, CV = _lib.FLAG_KERNEL_MATRIX, _lib.FLAG_COND_MATRIX, _lib.FLAG_COND_VALU
C_TAU, C_MUTAU = 4, 5           # tau = 1.0f / (expf(lv) + kPoeEps): expf 1 ulp = 2 u, the add, the divide; mu * tau: one more


@functools.lru_cache(maxsize=None)
def _cond_codes(I, pattern):
    """Codes over I - 1 items plus the unobserved last one, and their float64 indicators [2, B, I] (shared by the dims)."""
    inner = _pattern(pattern, I - 1)
    codes = np.concatenate([inner, np.full((inner.shape[0], 1), 2, np.uint8)], axis=1)
    return codes, M.onehots(codes)


def _cond_problem(A, I, pattern):
    """Host side of one case: codes over I - 1 items (+ the unobserved last one), the table, 2PL items, noise, and the fp64 product
    of experts of the fp32 table with its sums of absolute terms."""
    codes, oh = _cond_codes(I, pattern)
    B = codes.shape[0]
    g = torch.Generator().manual_seed(1000 * A + I)
    table = torch.cat([1.0 + 2.0 * torch.rand(2, I, A, generator=g), -6.0 * torch.rand(2, I, A, generator=g)], dim=2).contiguous()
    item = (0.3 * torch.randn(I, A + 1, generator=g)).contiguous()
    eps = torch.randn(B, A, generator=g)
    t = table.numpy().astype(np.float64)
    mu, lv = t[..., :A], t[..., A:]
    tau = 1.0 / (np.exp(lv) + EPS32)
    return dict(codes=codes, resp=torch.from_numpy((codes == 1).astype(np.float32)), mask=torch.from_numpy(codes != 2), table=table,
                item=item, eps=eps, mu=mu, lv=lv, tau=tau, oh=oh, k=(codes != 2).sum(1),
                lam=oh[0] @ tau[0] + oh[1] @ tau[1], s=oh[0] @ (mu * tau)[0] + oh[1] @ (mu * tau)[1])


def _ulp32(x):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 23)


def _posterior_bounds(P, I, prior, entry, panels):
    """-> (mu_ref, lv_ref, mu_bound, lv_bound) [B, A].  The sums: c_forward(k) (the VALU and in-kernel forms add k nonzero terms in
    some tree: at most k - 1 roundings, below it), + panels - 1 for `lam += st[...]` over the VALU first pass's panels.  The finish:
      vibo_encode   `smu / lam`, `logf(1.0f / lam)`: 1 and 1 + (logf: 1 ulp of the result)
      matrix kernel `inv_lam = 1.0f / lam; amu = smu * inv_lam`: 2;  `-kLn2 * fast_log2(lam)`: v_log_f32 1 ulp of log2 lam, the
                    constant's and the product's rounding: 2 u |logvar|
    missing prior: `lam += (I - nobs) * prior_w` with prior_w = 1.0f for the exact 1 / (1 + 1e-8): one rounding and 2^-26.6, 2."""
    k = P['k'][:, None].astype(np.float64)
    lam = P['lam'] + ((I - k) / (1.0 + EPS32) if prior else 0.0)
    mu_ref, lv_ref = P['s'] / lam, -np.log(lam)
    c_lam = M.c_forward(k) + C_TAU + (panels - 1) + (2 if prior else 0)
    c_s = M.c_forward(k) + C_MUTAU + (panels - 1)
    if entry == 'encode':
        mu_b = (c_s * P['s'] / lam + (c_lam + 1) * np.abs(mu_ref)) * U
        lv_b = (c_lam + 1) * U
        lv_b = lv_b + _ulp32(np.abs(lv_ref) + lv_b)
    else:
        mu_b = (c_s * P['s'] / lam + (c_lam + 2) * np.abs(mu_ref)) * U
        lv_b = c_lam * U + 2 * U * np.abs(lv_ref) + LN2 * _ulp32(np.abs(lv_ref) / LN2 * SECOND_ORDER + c_lam * U)
    return mu_ref, lv_ref, mu_b * SECOND_ORDER, lv_b * SECOND_ORDER


def _kl_head_bounds(P, amu, alv):
    """KL head of grad_table from the device's own posterior (amu, alv float64 [B, A]) -> (mean columns, logvar columns, their bounds),
    each [2, I, A].  The kernel's coefficients (backward_slot): S1 = amu * inv_lam, S2 = -(amu * amu + glv) * inv_lam with
    glv = -0.5f * (1.0f - inv_lam).  Counted, in u:
      E    the test's own lam = exp(-alv) against the kernel's: alv = -kLn2 * v_log_f32(lam) carries 2 |alv| + ln 2 ulp32(log2 lam) / u
      S1   E + 2 (inv_lam, the product)
      S2   E + 6 (inv_lam twice, amu * amu, 1 - inv_lam, the sum, the product) of |amu^2| + |(1 - 1 / lam) / 2|, which is at most
           3 |S2| because the expert means are at least 1 (amu^2 - 1 / 2 >= amu^2 / 2): 3 (E + 6) of |S2|
      the sums over the observers: c_cond_backward(k) = 7 k + 6 (the VALU pass: k fma and an fp64 finalize, below it)
      the chain, cm_cond_finalize_body / cond_post_kernel: `s1 * tau`: 1 + C_TAU = 5;
           `-(s1 * mu + s2) * tau * tau * es`: the product, the sum, 2 (1 + C_TAU), es = expf: 1 + 2 -- 15."""
    lam = np.exp(-alv)
    E = 2.0 * np.abs(alv) + LN2 * _ulp32(np.abs(alv) / LN2 * SECOND_ORDER) / U
    S1 = amu / lam
    S2 = -(amu * amu - 0.5 * (1.0 - 1.0 / lam)) / lam
    oh, mu, tau = P['oh'], P['mu'], P['tau']
    chain = tau * tau * np.exp(P['lv'])
    k = oh.sum(1)[..., None]                                               # observers [2, I, 1]

    def scat(v):                                                           # [B, A] -> [2, I, A]
        return np.stack([oh[0].T @ v, oh[1].T @ v])
    g_mu = scat(S1) * tau
    g_lv = -(scat(S1) * mu + scat(S2)) * chain
    c_sum = M.c_cond_backward(k)
    b_mu = (scat((E + 2) * np.abs(S1)) + (c_sum + 5) * scat(np.abs(S1))) * tau * U
    b_lv = (scat((E + 2) * np.abs(S1)) * mu + scat(3 * (E + 6) * np.abs(S2)) + (c_sum + 15) * (scat(np.abs(S1)) * mu + scat(np.abs(S2)))) * chain * U
    return g_mu, g_lv, b_mu * SECOND_ORDER, b_lv * SECOND_ORDER


def _plan_bits(spec, B, I, code, want_grad, flags):
    stride = ((I + 63) // 64 * 64 if I >= 256 else (I + 15) // 16 * 16) if code == _lib.MASK_CODES else (I + 3) // 4 * 4
    with ops.desc_flags(flags):
        d = ops._make_desc(spec, B, I, code, _lib.REG_KL, want_grad, stride, stride)
    return _lib.load().vibo_plan_cond_passes(ctypes.byref(d))


def _elbo_forms(A, I):
    """(name, rows, vibo_desc.flags, vibo_plan_cond_passes) of every first-pass form at this dim: bit 0 the experts' sums on the
    matrix pipe, bit 1 the table-gradient scatter, bit 2 no separate first pass (the matrix kernel's XM == 3 gather)."""
    first = 'cm_forward<1>/' + ('COUNT' if A == 8 else 'ones')
    forms = [(first, 'codes', KM | CM, 3), (first + '/tight', 'tight', KM | CM, 3), (first + '/row_index', 'gather', KM | CM, 3)]
    if A >= 5:
        forms.append(('cm_forward_fp32', 'fp32', KM | CM, 3))
    else:
        forms.append(('cond_pre/fp32 + matrix tail', 'fp32', KM | CM | _lib.FLAG_COND_THREE_PASS, 2))
    if A == 1 and I <= 1024:
        forms.append(('XM3 gather', 'fp32', KM | CM, 6))
    forms += [('cond_pre/fp32', 'fp32', KM | CV, 0), ('cond_pre/codes', 'codes', KM | CV, 0),
              ('cond_pre/no-emit', 'fp32', KM | _lib.FLAG_NO_EMIT_CODES, 0)]
    return forms


def _gathered(codes):
    """The minibatch at random places of a matrix with seven decoy rows -> (big codes, index)."""
    B, I = codes.shape
    rng = np.random.default_rng(B)
    big = rng.integers(0, 3, (B + 7, I)).astype(np.uint8)
    index = rng.permutation(B + 7)[:B]
    big[index] = codes
    return big, torch.from_numpy(index)


def _run_elbo(P, spec, rows, flags, bits):
    codes = P['codes']
    B, I = codes.shape
    code = _lib.MASK_U8 if rows == 'fp32' else _lib.MASK_CODES
    assert _plan_bits(spec, B, I, code, True, flags) == bits, ('vibo_plan_cond_passes', rows, flags, bits)
    with ops.desc_flags(flags):
        if rows == 'tight':
            cc = _code_rows(codes, (I + 3) // 4 * 4).codes
            d = dev()
            raw = ops._hip_launch_elbo(spec, cc, cc, _lib.MASK_CODES, None, P['table'].to(d), P['item'].to(d), P['eps'].to(d), None,
                                       _lib.REG_KL, True, B)
            torch.cuda.synchronize()
        elif rows == 'gather':
            big, index = _gathered(codes)
            raw = launch_elbo(spec, torch.from_numpy((big == 1).astype(np.float32)), torch.from_numpy(big != 2), P['table'], P['item'],
                              P['eps'], row_index=index, codes=True, kernel=_lib.KERNEL_NAMES[1])
        else:
            raw = launch_elbo(spec, P['resp'], P['mask'], P['table'], P['item'], P['eps'], pad=rows == 'fp32', codes=rows == 'codes',
                              kernel=_lib.KERNEL_NAMES[1])
    assert torch.isfinite(raw.flat).all()
    return raw


def _encode_forms():
    return [('cm_forward<1>', 'codes', CM, 1), ('cm_forward<1>/tight', 'tight', CM, 1), ('cm_forward<1>/row_index', 'gather', CM, 1),
            ('cond_pre/codes', 'codes', CV, 0), ('cond_pre/fp32', 'fp32', CV, 0)]


def _run_encode(P, spec, rows, flags, bit0):
    codes = P['codes']
    B, I = codes.shape
    d = dev()
    index = None
    # (vibo_encode's own choice is encode_on_matrix_pipe; under these pins it agrees with bit 0 of the forward-only ELBO plan)
    assert _plan_bits(spec, B, I, _lib.MASK_U8 if rows == 'fp32' else _lib.MASK_CODES, False, flags) & 1 == bit0
    if rows == 'fp32':
        r, m, code = ops.prepare_rows(*ops.pad_rows(P['resp'].to(d), P['mask'].to(d)))
    elif rows == 'tight':
        r, m, code = ops.prepare_rows(_code_rows(codes, (I + 3) // 4 * 4), None)
    else:
        big, index = _gathered(codes) if rows == 'gather' else (codes, None)
        r, m, code = ops.prepare_rows(ops.pack_cell_codes(torch.from_numpy((big == 1).astype(np.float32)).to(d),
                                                          torch.from_numpy(big != 2).to(d)), None)
    with ops.desc_flags(flags):
        mu, lv = ops._hip_encode(spec, r, m, code, index.to(d) if index is not None else None, P['table'].to(d), B)
    torch.cuda.synchronize()
    return mu.cpu(), lv.cpu()


DIMS = (1, 2, 4, 5, 8)
COND_ITEMS = (63, 64, 200, 1000, 1500)


@pytest.mark.parametrize('pattern', ['single', 'few'])
@pytest.mark.parametrize('I', COND_ITEMS)
@pytest.mark.parametrize('A', DIMS)
def test_conditional_posterior_and_kl_head_on_every_form(A, I, pattern):
    P = _cond_problem(A, I, pattern)
    spec = ElboSpec(irt_model=2, ability_dim=A, conditional=True, drop_missing=True)
    panels = (I + 1023) // 1024
    ratios, first = [], {}
    for entry, forms in (('encode', _encode_forms()), ('elbo', _elbo_forms(A, I))):
        for name, rows, flags, bits in forms:
            if entry == 'encode':
                mu, lv = _run_encode(P, spec, rows, flags, bits)
            else:
                raw = _run_elbo(P, spec, rows, flags, bits)
                mu, lv = raw.ability_mu.cpu(), raw.ability_logvar.cpu()
                assert float(raw.scalars.cpu()[_lib.S_NOBS]) == float(P['k'].sum()), 'S_NOBS is a sum of small integers: exact'
            tag = f'{entry}:{name}'
            if pattern == 'single':
                if entry in first:
                    _same_bits('B', tag, f'A{A}', pattern, 'mu', mu, first[entry][0])
                    _same_bits('B', tag, f'A{A}', pattern, 'logvar', lv, first[entry][1])
                else:
                    first[entry] = (mu, lv)
            mu_ref, lv_ref, mu_b, lv_b = _posterior_bounds(P, I, False, entry, panels if name.startswith('cond_pre') else 1)
            ratios.append(_hold('B', tag, f'A{A}', pattern, 'mu', np.abs(mu.double().numpy() - mu_ref), mu_b))
            ratios.append(_hold('B', tag, f'A{A}', pattern, 'logvar', np.abs(lv.double().numpy() - lv_ref), lv_b))
            if entry == 'elbo':
                g_mu, g_lv, b_mu, b_lv = _kl_head_bounds(P, mu.double().numpy(), lv.double().numpy())
                gt = raw.grad_table(1).cpu()
                assert bool((gt[:, I - 1] == 0).all()), 'no observer: exactly zero'
                gt = gt.double().numpy()
                ratios.append(_hold('B', tag, f'A{A}', pattern, 'dKL/dmu', np.abs(gt[..., :A] - g_mu), b_mu))
                ratios.append(_hold('B', tag, f'A{A}', pattern, 'dKL/dlv', np.abs(gt[..., A:] - g_lv), b_lv))
    assert max(ratios) <= 1.0, (A, I, pattern, max(ratios))


@pytest.mark.parametrize('A', DIMS)
def test_conditional_posterior_with_prior_experts(A):
    """--drop-missing off: a thousand N(0, 1) prior experts beside the few observed ones; the prior term is in the bound."""
    I, pattern = 1000, 'few'
    P = _cond_problem(A, I, pattern)
    spec = ElboSpec(irt_model=2, ability_dim=A, conditional=True, drop_missing=False)
    ratios = []
    for entry, forms in (('encode', _encode_forms()[:1] + _encode_forms()[3:4]), ('elbo', [f for f in _elbo_forms(A, I) if f[1] != 'gather'])):
        for name, rows, flags, bits in forms:
            if entry == 'encode':
                mu, lv = _run_encode(P, spec, rows, flags, bits)
            else:
                raw = _run_elbo(P, spec, rows, flags, bits)
                mu, lv = raw.ability_mu.cpu(), raw.ability_logvar.cpu()
            mu_ref, lv_ref, mu_b, lv_b = _posterior_bounds(P, I, True, entry, 1)
            ratios.append(_hold('B', f'{entry}:{name}', f'A{A}', 'few+prior', 'mu', np.abs(mu.double().numpy() - mu_ref), mu_b))
            ratios.append(_hold('B', f'{entry}:{name}', f'A{A}', 'few+prior', 'logvar', np.abs(lv.double().numpy() - lv_ref), lv_b))
    assert max(ratios) <= 1.0, (A, max(ratios))


@pytest.mark.parametrize('I', [63, 200, 1000])
@pytest.mark.parametrize('A', DIMS)
def test_table_gradient_matrix_form_against_valu_form(A, I):
    """single, fp32 rows, one panel, both heads: VIBO_FLAG_COND_MATRIX (+ VIBO_FLAG_COND_THREE_PASS at 1 dim) against
    VIBO_FLAG_COND_VALU.  Up to 4 dims both run the VALU first pass, from 5 the posterior is bit-identical between
    cm_forward_fp32_kernel and cond_pre (asserted): the row-split kernel hands both tails the same coefficients, and with one
    observer per (code, item) each tail's sum is that observer's coefficient exactly.  Both then evaluate `s1 * tau` (one rounding
    each: 2 u of the entry) and `-(s1 * mu + s2) * tau * tau * es` (the inner product unless contracted to an fma: u |S1 mu|, the sum
    and three products: 4 u of the entry, per tail), with the same tau and es."""
    P = _cond_problem(A, I, 'single')
    spec = ElboSpec(irt_model=2, ability_dim=A, conditional=True, drop_missing=True)
    m = _run_elbo(P, spec, 'fp32', KM | CM | (_lib.FLAG_COND_THREE_PASS if A == 1 else 0), 3 if A >= 5 else 2)
    v = _run_elbo(P, spec, 'fp32', KM | CV, 0)
    assert torch.equal(m.ability_mu, v.ability_mu) and torch.equal(m.ability_logvar, v.ability_logvar)
    tag, ratios = 'matrix tail vs VALU tail', []
    growth = P['mu'] * P['tau'] * np.exp(P['lv'])                         # |S1 mu| tau^2 e^lv = |S1 tau| mu tau e^lv
    for head in range(2):
        gm, gv = m.grad_table(head).cpu().double().numpy(), v.grad_table(head).cpu().double().numpy()
        ratios.append(_hold('B', tag, f'A{A}', 'single', f'head{head}/mu', np.abs(gm[..., :A] - gv[..., :A]),
                            2 * U * np.abs(gv[..., :A]) * SECOND_ORDER))
        ratios.append(_hold('B', tag, f'A{A}', 'single', f'head{head}/logvar', np.abs(gm[..., A:] - gv[..., A:]),
                            U * (2 * np.abs(gv[..., :A]) * growth + 8 * np.abs(gv[..., A:])) * SECOND_ORDER))
    assert max(ratios) <= 1.0, (A, I, ratios)
