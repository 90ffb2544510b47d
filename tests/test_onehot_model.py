"""CPU checks of oracle/onehot_model.py: the three-piece split is exact where it says so, the patterns are what they claim, the
float32 model of the contractions stays inside sum_bound / grad_bound on every output, and the model with one piece missing
leaves them -- on at least half of the outputs of every (class, k) the GPU tests rely on.  `pytest -s` prints the shares that
the model's docstring quotes."""
import numpy as np
import pytest

from oracle import onehot_model as M

I_CPU, SEED = 200, 11


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _all_mantissas(exponents):
    m = np.arange(1 << 23, dtype=np.uint32)
    return np.concatenate([((np.uint32(e + 127) << np.uint32(23)) | m).view(np.float32) for e in exponents])


def _check_exact(x):
    hi, mid, lo = M.split3(x)
    h = np.float32(0.5) * x
    assert np.array_equal(_bits((hi + mid) + lo), _bits(h))             # fp32 adds: every partial sum is a prefix of h's bits
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), h.astype(np.float64))
    for p in (hi, mid, lo):                                              # bf16 numbers
        assert not (_bits(p) & np.uint32(0xffff)).any()
    # non-overlapping: a piece is below the ulp of the piece before it (8 significant bits: ulp = 2^-7 of its leading bit)
    def ulp8(p):
        return np.where(p == 0, np.inf, 2.0 ** (np.floor(np.log2(np.abs(p.astype(np.float64)) + (p == 0))) - 7))
    assert (np.abs(mid.astype(np.float64)) < ulp8(hi)).all() and (np.abs(lo.astype(np.float64)) < ulp8(mid)).all()
    # truncation: the pieces share the value's sign
    assert ((np.sign(mid) == 0) | (np.sign(mid) == np.sign(hi))).all() and ((np.sign(lo) == 0) | (np.sign(lo) == np.sign(hi))).all()
    return hi, mid, lo


def test_split3_is_exact_on_every_mantissa_of_five_binades():
    for e in (-102, -1, 0, 1, 100):                                     # the lowest all-normal binade, around 1.0, the values class's top
        x = _all_mantissas([e])
        hi, mid, lo = _check_exact(x)
        _check_exact(-x[::4097])
        for p in (hi, mid, lo):                                          # every nonzero piece is a NORMAL bf16 number from 2^-102 on
            assert (np.abs(p[p != 0]) >= 2.0 ** -126).all()


def test_split3_zero_and_the_exponent_range():
    z = np.array([0.0, -0.0], np.float32)
    for p in M.split3(z):
        assert np.array_equal(np.abs(p), np.zeros(2, np.float32))
    assert np.array_equal(_bits(M.split3(z)[0]), _bits(z))               # hi keeps the zero's sign
    rng = np.random.default_rng(3)
    # all pieces normal: |x| in [2^-102, 2^127]  (0.5 x: no overflow anywhere in fp32's range)
    e = np.repeat(np.arange(-102, 128), 64)
    x = M._assemble(rng.integers(0, 2, e.size), e, M._hostile_mantissas(rng, e.size))
    assert np.abs(x).min() >= M.ALL_NORMAL_MIN
    for p in _check_exact(x):
        assert (np.abs(p[p != 0]) >= 2.0 ** -126).all()
    # below: a residual under 2^-126 is an fp32 subnormal, whose top 16 bits are a fixed 2^-133 grid and no longer 8 significant
    # bits -- such pieces are bf16 subnormals.  Kept, they leave less than 2^-133 of 0.5 x behind; flushed, less than 2^-126:
    # either way less than FTZ_ABS of a term
    e = np.repeat(np.arange(-125, -102), 64)
    x = M._assemble(rng.integers(0, 2, e.size), e, M._hostile_mantissas(rng, e.size))
    hi, mid, lo = M.split3(x)
    half = 0.5 * x.astype(np.float64)
    assert (np.abs(half - sum(p.astype(np.float64) for p in (hi, mid, lo))) < 2.0 ** -133).all()
    kept = sum(M.flush_bf16_subnormals(p).astype(np.float64) for p in (hi, mid, lo))
    lost = np.abs(half - kept)
    assert (2.0 * lost < M.FTZ_ABS).all() and lost.max() > 0
    # subnormal x: 0.5 x itself rounds by at most 2^-150, far below the same term
    x = (np.arange(1, 4096, dtype=np.uint32) * np.uint32(2047)).view(np.float32)
    assert x.max() < 2.0 ** -126
    hi, mid, lo = M.split3(x)
    kept = sum(M.flush_bf16_subnormals(p).astype(np.float64) for p in (hi, mid, lo))
    assert (2.0 * np.abs(0.5 * x.astype(np.float64) - kept) < M.FTZ_ABS).all()


def test_rounding_the_pieces_to_nearest_is_exact_too_but_overlaps():
    rng = np.random.default_rng(5)
    x = M._assemble(rng.integers(0, 2, 4096), rng.integers(-50, 50, 4096), M._hostile_mantissas(rng, 4096))
    hi, mid, lo = M.split3(x, nearest=True)
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), 0.5 * x.astype(np.float64))
    assert (np.sign(mid) == -np.sign(hi)).any()                          # (what the truncating split never does)


@pytest.mark.parametrize('I', [63, 64, 200, 1000])
def test_patterns(I):
    B = 2 * I
    s = M.make_pattern('single', B, I, SEED)
    assert ((s != 2).sum(1) == 1).all() and ((s == 0).sum(0) == 1).all() and ((s == 1).sum(0) == 1).all()
    assert not np.array_equal(np.argmax(s != 2, axis=1)[:I], np.arange(I))          # person order and item order are unrelated
    f = M.make_pattern('few', B, I, SEED)
    k = (f != 2).sum(1)
    assert set(k.tolist()) == set(M.KS) and all((k == kk).sum() == B // 4 or abs((k == kk).sum() - B / 4) <= 1 for kk in M.KS)
    for c in (0, 1):
        n = (f == c).sum(0)
        assert n.min() >= 1 and n.max() <= 16
    # the cells of the 16-cell persons fall on all four K-steps j and all four lane groups g of a 64-item step
    wide = f[k == 16] != 2
    pos = np.arange(I) % 64
    for g in range(4):
        for j in range(4):
            slot = ((pos >> 4) == g) & (((pos >> 2) & 3) == j)
            if I >= 64:
                assert wide[:, slot].any(1).mean() >= 0.75, (g, j)      # (15 drawn slots + the first cell's own)
    iso = M.make_pattern('isolated', B + 1, I, SEED)
    assert (iso[:, I - 1] == 2).all() and ((iso[-3:] != 2).sum() == 0) and ((iso[:-3] != 2).sum(1) == 1).all()
    assert ((iso[:, :I - 1] == 0).sum(0) == 1).all() and ((iso[:, :I - 1] == 1).sum(0) == 1).all()


def test_value_classes():
    h = M.make_values('hostile', (2, 64, 64), 1)
    low = _bits(h) & np.uint32(0xff)
    assert (low == 0xff).mean() > 0.6 and ((_bits(h) & np.uint32(0x7fffff)) == 0x7fffff).any() and (low == 0x55).any() and (low == 0xaa).any()
    assert (h[..., 0::2] > 0).all() and (h[..., 1::2] < 0).all()
    b = M.make_values('binades', (2, 64, 64), 1)
    e = np.floor(np.log2(np.abs(b.astype(np.float64))))
    assert e.min() == -100 and e.max() == 100 and (np.ptp(e[0, :, 0]) > 150) and (b > 0).any() and (b < 0).any()
    t = M.make_values('tiny', (2, 64, 64), 1)
    assert (np.abs(t) >= 2.0 ** -110).all() and (np.abs(t) < 2.0 ** -109).all()
    g = M.make_values('grid', (2, 64, 64), 1).astype(np.float64)
    m = g / 2.0 ** ((np.arange(64) * 7) % 41 - 20)
    assert np.array_equal(m, np.round(m)) and np.abs(m).max() < 2 ** 20 and np.abs(m).max() > 2 ** 19


def _share_outside(err, bound, sel):
    return float((err[sel] > bound[sel]).mean())


@pytest.fixture(scope='module')
def few():
    codes = M.make_pattern('few', 2 * I_CPU, I_CPU, SEED)
    return codes, (codes != 2).sum(1)


def test_forward_model_and_bound(few):
    codes, k = few
    worst_in, worst_out = {None: 0.0, 'nearest': 0.0, 'ftz': 0.0}, 0.0
    for cls in M.CLASSES:
        X = M.make_values(cls, (2, I_CPU, 8), SEED + len(cls))
        S, T, kk = M.exact_sum(codes, X)
        bound = M.sum_bound(T, kk)
        for mode in (None, 'nearest', 'ftz'):
            err = np.abs(M.model_sum(codes, X, mode).astype(np.float64) - S)
            assert (err <= bound).all(), (cls, mode, float((err / bound).max()))       # 100 % of the outputs
            worst_in[mode] = max(worst_in[mode], float((err / bound).max()))
        if cls == 'grid':
            assert np.array_equal(M.model_sum(codes, X).astype(np.float64), S)
        err_mid = np.abs(M.model_sum(codes, X, 'mid').astype(np.float64) - S)
        assert (err_mid > bound).mean() > 0.95, cls                 # (a value whose middle byte happens to be zero has no mid)
        err_lo = np.abs(M.model_sum(codes, X, 'lo').astype(np.float64) - S)
        for kv in M.KS:
            share = _share_outside(err_lo, bound, k == kv)
            print(f'forward  {cls:8s} k = {kv:2d}: without lo {100 * share:5.1f} % of the outputs outside the bound')
            if (cls, kv) in M.DROP_LO_PLAN:
                assert share >= 0.5, (cls, kv, share)
                worst_out = max(worst_out, float((err_lo / bound)[k == kv].max()))
    print('forward: worst error / bound of the intact model %.3f, with pieces rounded to nearest %.3f, with bf16 subnormals flushed %.3f; '
          'without lo the worst output is at %.1f x its bound' % (worst_in[None], worst_in['nearest'], worst_in['ftz'], worst_out))
    # one observed cell: the value itself
    single = M.make_pattern('single', 2 * I_CPU, I_CPU, SEED)
    X = M.make_values('binades', (2, I_CPU, 8), 2)
    S = M.model_sum(single, X)
    p, i = np.nonzero(single != 2)
    assert np.array_equal(_bits(S[p]), _bits(X[single[p, i], i]))


@pytest.mark.parametrize('packed', [False, True], ids=['three-mfmas', 'packed'])
def test_backward_model_and_bound(few, packed):
    codes, _ = few
    N = 4 if packed else 8
    nsl = 2 if packed else 1
    worst_in = 0.0
    for cls in M.CLASSES:
        G = M.make_values(cls, (2 * I_CPU, N), SEED + 7 + len(cls))
        D, T, kk = M.exact_grad(codes, G)
        bound = M.grad_bound(T, kk, cond=packed)
        err = np.abs(M.model_grad(codes, G, None, packed, nsl).astype(np.float64) - D)
        assert (err <= bound).all(), (cls, float((err / bound).max()))
        worst_in = max(worst_in, float((err / bound).max()))
        if cls == 'grid':
            assert np.array_equal(M.model_grad(codes, G, None, packed, nsl).astype(np.float64), D)
        assert (np.abs(M.model_grad(codes, G, 'mid', packed, nsl).astype(np.float64) - D) > bound).mean() > 0.95, cls
        err_lo = np.abs(M.model_grad(codes, G, 'lo', packed, nsl).astype(np.float64) - D)
        kb = np.broadcast_to(kk[..., None], err_lo.shape)
        for lo_k, hi_k in M.OBSERVER_BUCKETS:
            sel = (kb >= lo_k) & (kb <= hi_k)
            if not sel.any():
                continue
            share = _share_outside(err_lo, bound, sel)
            print(f'backward {"packed" if packed else "3 mfma":7s} {cls:8s} observers {lo_k:2d}..{hi_k:2d}: without lo {100 * share:5.1f} % outside the bound')
            if cls in ('hostile', 'binades'):
                assert share >= 0.5, (cls, lo_k, share)
        if packed:
            for mode in ('neighbour', 'two-groups'):
                e2 = np.abs(M.model_grad(codes, G, mode, True, nsl).astype(np.float64) - D)
                share = float((e2 > bound).mean())
                print(f'backward packed  {cls:8s} {mode}: {100 * share:5.1f} % outside the bound')
                if cls in ('hostile', 'binades'):
                    assert share >= 0.5, (cls, mode, share)
    print(f'backward: intact model worst error / bound {worst_in:.3f}')


def test_person_ranges_match_the_library():
    # (cm_ranges of csrc/vibo_cmean.hip, worked by hand)
    assert M.person_ranges(2000, 16) == (32, 64) and M.person_ranges(126, 1) == (2, 64) and M.person_ranges(4099, 16) == (65, 64)
    assert M.person_ranges(1_000_000, 16) == (128, 7872)
