"""The matrix row-split kernel's split-f16 contractions, cell by cell, on inputs built to be the split's worst case.

Every other kernel-vs-oracle test compares aggregates (a tensor's largest error over its max-abs, one log-likelihood sum) on
N(0, 1) inputs.  Here every number is compared on its own, in fp64 on the host, against a bound that
oracle/split_model.py derives from the split's arithmetic and the inputs alone (cell_bound / grad_bounds; the CPU model
of the scheme is held to the same bound in tests/test_split_model.py, where dropping any one term of it is shown to break it).

Single cells are observed through the C ABI as it is:
  * every item is observed by exactly ONE person p(i) (the other cells are missing but still run through the MFMAs), so
    grad_item's difficulty column is x - sigmoid(logit) of one cell -- the logit error is that difference over sigmoid'(l),
    taken where |l| <= 3 -- and its discrimination columns are -g theta of one cell;
  * with the caller-supplied posterior (ElboSpec(given=True)) and eps = 0 the sample IS the mean the test passes in: theta's
    bit patterns are the test's, and grad_table(0)[:, :A] is d LL/d theta person by person.  Under the unconditional posterior
    (the headline instantiation) theta is what the kernel returns (raw.ability, pinned to the oracle elsewhere and once more
    here); the difficulties are set from the oracle's theta and the reference is built from the kernel's.
Input classes: split_model.make_case.  One dense launch per class (all cells observed) covers the sums over batches.  The
VALU kernel (true fp32) runs the same inputs against the plain fp32 bound: if IT fails, the test or the reference is wrong.

3PL (class clamp3): cancelling logits whose p = guess + (1 - guess) sigmoid(l) sits within 1e-6 of a probability clamp value, on both
sides; compared with the reference's exact saturation on every cell at least 4 fp32 ulp of p away from the clamp (at most 2 % may be
left out).  Forward only (want_grad = 0, another instantiation of the kernel): one person who observes every item, S_LL against
the sum of the exact log-likelihoods.

NOT pinned by this file: the KERNEL's third difficulty piece b2.  It is worth at most 6 x 2^-24 |b|; a logit seen through
x - sigmoid(l) carries 6 x 2^-24 / sigmoid'(l) of fp32 evaluation noise, and in cancelling cells the products' own 28 x 2^-24 hide
it.  A build with b2 zeroed passes every case here, the 'bias' class included; only the CPU model (tests/test_split_model.py)
shows that term.  Builds without theta_lo * a_hi, or with g_hi alone in the d LL/d theta transpose, fail most cases.

VIBO_TOL_RECORD=path appends, per observable, the worst error / bound, the largest error, the fp64 model's worst ratio on the same
cells and the bound's size against the plain fp32 bound as a JSON line; tools/split_record_table.py turns such a file into
profiles/split_worst_case_record.txt.  The assertions hold either way."""
import numpy as np
import pytest
import torch

from gpu_common import launch_elbo, record, recording
from oracle import split_model as M
from oracle import vibo_table_ref as T
from vibo_amd import _lib, ops
from vibo_amd.ops import ElboSpec

pytestmark = pytest.mark.gpu

KERNELS = {'matrix': _lib.FLAG_KERNEL_MATRIX, 'valu': _lib.FLAG_KERNEL_VALU}

# cls, A, B, I, posterior, rows, kwargs of make_case
PLAN = [
    ('cancel', 2, 33, 200, 'given', 'direct', {}), ('cancel', 5, 95, 640, 'given', 'gather', {}), ('cancel', 8, 64, 1000, 'given', 'codes', {}),
    ('cancel', 8, 2049, 1024, 'given', 'direct', {}), ('cancel', 8, 33, 1028, 'given', 'direct', {}), ('cancel', 5, 32, 2500, 'given', 'codes', {}),
    ('cancel', 8, 64, 1000, 'uncond', 'direct', dict(shift=3)), ('cancel', 2, 95, 200, 'uncond', 'codes', {}),
    ('cancel', 2, 64, 640, 'given', 'direct', dict(all_signs=True)), ('cancel', 2, 32, 1024, 'given', 'codes', dict(all_signs=True, shift=5)),
    ('clamp3', 2, 33, 200, 'given', 'direct', {}), ('clamp3', 8, 64, 1000, 'given', 'codes', {}), ('clamp3', 5, 95, 640, 'given', 'gather', {}),
    ('clamp3', 8, 33, 1024, 'given', 'direct', dict(shift=9)), ('clamp3', 8, 64, 1000, 'uncond', 'direct', {}), ('clamp3', 2, 95, 640, 'uncond', 'codes', {}),
    ('hostile', 2, 64, 640, 'given', 'direct', {}), ('hostile', 8, 33, 1024, 'given', 'codes', dict(shift=7)), ('hostile', 8, 33, 1024, 'uncond', 'gather', {}),
    ('bias', 1, 32, 200, 'given', 'direct', {}), ('bias', 8, 95, 1000, 'given', 'gather', {}), ('bias', 8, 95, 1000, 'uncond', 'direct', {}),
    ('onepl', 4, 64, 640, 'given', 'direct', {}), ('onepl', 8, 33, 1000, 'given', 'codes', {}), ('onepl', 4, 64, 640, 'uncond', 'direct', {}),
    ('mixed_a', 8, 64, 1000, 'given', 'direct', dict(outliers=(6,))), ('mixed_a', 8, 64, 1000, 'given', 'codes', dict(outliers=(10,))),
    ('mixed_a', 5, 95, 640, 'given', 'direct', dict(outliers=(14,), same_tile=True)),
    ('mixed_a', 8, 64, 1024, 'given', 'direct', dict(outliers=(20, 14, 10, 6))),
    ('mixed_a', 8, 64, 1000, 'uncond', 'direct', dict(outliers=(10,))), ('mixed_a', 8, 64, 1000, 'uncond', 'direct', dict(outliers=(20,))),
    ('mixed_b', 8, 64, 1000, 'given', 'direct', dict(outliers=(14,))), ('mixed_b', 2, 33, 200, 'given', 'direct', dict(outliers=(16,), same_tile=True)),
    ('mixed_b', 8, 64, 1000, 'given', 'codes', dict(outliers=(20,))), ('mixed_b', 5, 95, 640, 'given', 'direct', dict(outliers=(29,))),
    ('mixed_b', 8, 64, 1000, 'uncond', 'direct', dict(outliers=(20,))), ('mixed_b', 8, 64, 1000, 'uncond', 'direct', dict(outliers=(29,))),
]
FORWARD = [('cancel', 8, 640), ('cancel', 2, 200), ('hostile', 8, 1024), ('bias', 8, 1000), ('onepl', 4, 640), ('clamp3', 8, 1000)]
DENSE = [('cancel', {}), ('hostile', {}), ('bias', {}), ('onepl', {}), ('mixed_a', dict(outliers=(10,))), ('mixed_b', dict(outliers=(20,)))]


def _id(c):
    return f'{c[0]}-A{c[1]}-B{c[2]}-I{c[3]}-{c[4]}-{c[5]}' + ''.join(f'-2^{k}' for k in c[6].get('outliers', ())) + \
        ('-same-tile' if c[6].get('same_tile') else '') + ('-all-signs' if c[6].get('all_signs') else '')


def _record(cls, kernel, observable, err, bound, **extra):
    """Worst err / bound of one observable; a bound of exactly zero admits no error.  -> the ratio (the caller asserts it)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.all(np.isfinite(err)), (cls, kernel, observable)
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    if zero.any() and float(err[zero].max()) > 0:
        ratio = float('inf')
    record('split_worst_case', err.max(), **{'class': cls}, kernel=kernel, observable=observable, ratio=ratio, **extra)
    print(f'{cls:8s} {kernel:6s} {observable:8s} worst error / bound = {ratio:.3f}  (largest error {float(err.max()):.3e})')
    return ratio


def _launch(case, posterior, rows, table, kernel, want_grad=True):
    B, I = case['resp'].shape
    A = case['theta'].shape[1]
    spec = ElboSpec(irt_model=case['irt'], ability_dim=A, given=posterior == 'given')
    resp, mask = torch.from_numpy(case['resp']), torch.from_numpy(case['obs'])
    index = None
    if rows == 'gather':
        P = B + 7
        index = torch.randperm(P, generator=torch.Generator().manual_seed(B))[:B]
        resp_all, mask_all = torch.zeros(P, I), torch.zeros(P, I, dtype=torch.bool)
        resp_all[index], mask_all[index] = resp, mask
        resp, mask = resp_all, mask_all
    # the pin must really put the call on the kernel under test: any other kernel is true fp32 and would pass the split bound idly
    raw = launch_elbo(spec, resp, mask, table, torch.from_numpy(M.item_tensor(case)), torch.zeros(B, A), row_index=index, pad=True,
                      codes=rows == 'codes', want_grad=want_grad, kernel=_lib.KERNEL_NAMES[1 if kernel == 'matrix' else 2])
    assert torch.isfinite(raw.scalars).all() and (not want_grad or torch.isfinite(raw.flat).all())
    return spec, raw


def _build(cls, A, B, I, posterior, seed, kw, dense=False):
    """-> (case, table).  given: table = [theta | logvar 0]; uncond: a seeded encoder table, theta from the fp64 oracle's product
    of experts on the case's own responses (which do not depend on theta: split_model.make_case)."""
    if posterior == 'given':
        case = M.make_case(cls, A, B, I, seed, **kw)
        if dense:
            case['obs'][:] = True
            case['obs'][:, case['outliers']] = False
        return case, torch.from_numpy(np.concatenate([case['theta'], np.zeros((B, A), np.float32)], axis=1))
    assert not dense
    g = torch.Generator().manual_seed(seed)
    table = (torch.randn(2, 2 * A, generator=g) * 0.7)
    table[:, :A] *= 3.0                                  # posterior means of a few units: products that can cancel
    c0 = M.make_case(cls, A, B, I, seed, **kw)
    ref = T.fused_elbo_ref(table.double(), torch.zeros(I, M.item_tensor(c0).shape[1], dtype=torch.float64),      # (only theta is wanted)
                           torch.from_numpy(c0['resp']).double(), torch.from_numpy(c0['obs']), torch.zeros(B, A, dtype=torch.float64),
                           irt_model=c0['irt'], ability_dim=A, want_grad=False)
    case = M.make_case(cls, A, B, I, seed, theta=ref['ability'].float().numpy(), **kw)
    assert np.array_equal(case['resp'], c0['resp']) and np.array_equal(case['obs'], c0['obs'])
    case['theta_oracle'] = ref['ability'].numpy()
    return case, table


def _check(case, spec, raw, posterior, kernel, dense=False):
    cls, irt = case['cls'], case['irt']
    B, I = case['resp'].shape
    A = case['theta'].shape[1]
    theta = raw.ability.cpu().numpy()                    # the fp32 sample the kernel used
    if posterior == 'given':
        assert np.array_equal(theta, case['theta'])     # eps = 0, logvar = 0: the sample is the mean, bit for bit
    else:
        assert np.abs(theta - case['theta_oracle']).max() < 2e-5 * max(1.0, np.abs(case['theta_oracle']).max())
    fp32 = kernel == 'valu'
    ref = M.reference(case, theta)
    e_l = M.per_panel(M.cell_bound, theta, case['a'], case['b'], irt, fp32=fp32)
    c_eval = M.C_SIGMA3 if irt == 3 else M.C_SIGMA
    bnd_b, bnd_a, bnd_t = M.grad_bounds(theta, case['a'], case['b'], ref['g'], case['obs'], e_l, irt, fp32=fp32,
                                        dgdl=ref['dgdl'] if irt == 3 else None, c_eval=c_eval)
    # 3PL: entries fed by a cell within 4 fp32 ulp of p of a clamp value are not asserted; at most 2 % of the observed cells
    excl = ref['excluded']
    assert excl.sum() <= 0.02 * case['obs'].sum(), (int(excl.sum()), int(case['obs'].sum()))
    items, persons = ~excl.any(0), ~excl.any(1)
    if dense:
        items[case['outliers']] = False                 # (unobserved in the dense launches: _build)
    gi = raw.grad_item((I, spec.item_dim)).cpu().numpy().astype(np.float64)
    gb = gi[:, 0 if irt == 1 else A]
    tag = cls + ('/dense' if dense else '')
    ratios = [_record(tag, kernel, 'dLL/db', np.abs(gb - ref['g_b'])[items], bnd_b[items])]
    if not dense and irt != 3:
        # logit of the one observed cell of each item, where sigmoid'(l) >= 0.045 and the clamp is far
        idx = np.arange(I)
        l = ref['logit'][case['p_obs'], idx]
        sel = np.abs(l) <= 3.0
        assert sel.mean() > (0.0 if cls == 'bias' else 0.8)
        sp = (M.sigmoid(l) * (1 - M.sigmoid(l)))[sel]
        el = e_l[case['p_obs'], idx][sel]
        extra = {}
        if not fp32 and I <= M.PANEL and recording():
            # for the record: the fp64 model of the scheme on the same cells, and the bound's size against the plain fp32 bound
            model = np.abs(M.logit_model(theta, case['a'], case['b'], irt) - ref['logit'])[case['p_obs'], idx][sel]
            vs32 = (el / M.cell_bound(theta, case['a'], case['b'], irt, fp32=True)[case['p_obs'], idx][sel])
            extra = dict(model_ratio=float((model / el).max()), bound_over_fp32_median=float(np.median(vs32)), bound_over_fp32_max=float(vs32.max()))
        ratios.append(_record(tag, kernel, 'logit', np.abs(gb - ref['g_b'])[sel] / sp, el + el ** 2 / sp + M.C_SIGMA * M.U / sp, **extra))
    if irt != 1:
        ratios.append(_record(tag, kernel, 'dLL/da', np.abs(gi[:, :A] - ref['g_a'])[items], bnd_a[items]))
    if posterior == 'given':
        gt = raw.grad_table(0).cpu().numpy().astype(np.float64)[:, :A]
        ratios.append(_record(tag, kernel, 'dLL/dth', np.abs(gt - ref['g_theta'])[persons], bnd_t[persons]))
    assert max(ratios) <= 1.0, (tag, kernel, ratios)


@pytest.mark.parametrize('kernel', list(KERNELS))
@pytest.mark.parametrize('n', range(len(PLAN)), ids=[_id(c) for c in PLAN])
def test_one_observer_per_item(n, kernel):
    cls, A, B, I, posterior, rows, kw = PLAN[n]
    assert I <= M.PANEL or cls in ('cancel', 'hostile', 'bias', 'onepl')      # mixed magnitudes: one panel (the scales are per panel)
    case, table = _build(cls, A, B, I, posterior, 1000 + n, kw)
    with ops.desc_flags(KERNELS[kernel]):
        spec, raw = _launch(case, posterior, rows, table, kernel)
    _check(case, spec, raw, posterior, kernel)


@pytest.mark.parametrize('kernel', list(KERNELS))
@pytest.mark.parametrize('cls,kw', DENSE, ids=[d[0] for d in DENSE])
def test_dense_launch_with_summed_bounds(cls, kw, kernel):
    """B = 96 (three batches of the matrix kernel), every cell observed: each gradient entry is a sum over 96 or 640 cells and is
    held to the sum of their bounds plus the fp32 accumulation term.  The outlier item of the mixed classes stays in the launch (it
    sets the scales) but is observed by nobody, so that its own huge terms do not swamp the persons' sums.  (No 3PL clamp class
    here: with every cell observed a third of them saturate and fall under the 4-ulp exclusion.)"""
    case, table = _build(cls, 8, 96, 640, 'given', 2000 + len(cls), kw, dense=True)
    with ops.desc_flags(KERNELS[kernel]):
        spec, raw = _launch(case, 'given', 'direct', table, kernel)
    _check(case, spec, raw, 'given', kernel, dense=True)


@pytest.mark.parametrize('kernel', list(KERNELS))
@pytest.mark.parametrize('cls,A,I', FORWARD, ids=[f'{c[0]}-A{c[1]}-I{c[2]}' for c in FORWARD])
def test_forward_only_through_s_ll(cls, A, I, kernel):
    """want_grad = 0 is an instantiation of its own (no g split, no transposed image).  ONE person who observes every item -- no
    unobserved cell, whose -1 the kernel's sum would carry -- and S_LL against the sum of the exact per-cell log-likelihoods:
    sum |g| E_logit + E^2 plus the fp32 evaluation (split_model.ll_bound).  3PL: |d ll/d l| <= 1 in place of |g| (the value is
    continuous across the clamp; the gradient is not).  This is an aggregate again -- the cells' errors cancel and the measured ratio
    is ~0.01 -- but one the split still shows in: a build without theta_lo * a_hi fails half of these cases."""
    case, table = _build(cls, A, 1, I, 'given', 3000 + I + A, {})
    with ops.desc_flags(KERNELS[kernel]):
        spec, raw = _launch(case, 'given', 'direct', table, kernel, want_grad=False)
    theta = raw.ability.cpu().numpy()
    assert np.array_equal(theta, case['theta'])
    ref = M.reference(case, theta)
    e_l = M.per_panel(M.cell_bound, theta, case['a'], case['b'], case['irt'], fp32=kernel == 'valu')
    slope = np.ones_like(ref['g']) if case['irt'] == 3 else ref['g']
    bound = M.ll_bound(ref['ll'], slope, case['obs'], e_l, fp32=kernel == 'valu')
    s_ll = float(raw.scalars.cpu()[_lib.S_LL].double())
    assert _record(cls + '/forward', kernel, 'S_LL', np.array([abs(s_ll - float(ref['ll'].sum()))]), np.array([bound])) <= 1.0
