"""The MLP decoder kernel (csrc/vibo_decoder.hip, decoder_kernel), term by term and at every operand scale.

tests/test_gpu_decoder.py compares whole gradient tensors on Gaussian inputs of one scale to 2e-4 of their maximum; here EVERY entry of
every record is held to a bound of its own, counted in oracle/decoder_model.py from the kernel's statements and the inputs alone (the
fp64 value of the hi/lo scheme is held to the same bounds in tests/test_decoder_model.py, where each mutation of it leaves one).  All
launches go through vibo_decoder_fwd_bwd with a descriptor of the test's own (decoder_cells_common.launch), so person_chunks is the
test's choice and the person loop takes a second pair, a later pair and an odd tail at B <= 10.

Mask layouts (decoder_model.masks):
  term    one observed item per (person, 16-item wave group): dV_part[4 ib + w][p][:] is that term's dz1 (all 64 entries), dL[p, i] its
          dl; unobserved dL entries and every record entry without an observed term are exact zeros; prob holds every term's forward.
  single  one observed term per (person chunk, wave): dW2_part[wave] is one outer product through the transposition image (4 096
          entries), the dvec_part rows are dz2, d_o h2, dz1 l and d_o of that term, dU_part / dguess_part / ll_part single-term too.  The
          observer sits in the first pair, a later pair (r = 0 and r = 1) and the last pair (the odd tail where the chunk is odd), on
          every i16 lane of every wave (class `unit`: 16 seeds) and in the ragged last item block.  Because row 0 of dvec_part IS the
          kernel's dz2, the backward half (dV, dU, dW2, dw1) is also held on that value: its split residual evaluated, nothing propagated
          ('x|dz2' in the record) -- a bound of a few u, where a dropped cross term is 2^-11.
  dense   30 % missing: every record against the summed bounds plus the counted chains; empty chunks write exact zeros.
Per case: shapes I in {1, 15, 16, 17, 63, 64, 65, 130} x B in {1, 2, 3, 7, 8, 9, 10} (cycled against each other over the classes) x
person_chunks in {1, 2, ceil(B / 2)} and 4 at B = 10; the six modes (U alone, w1 alone, resid alone, guess alone, the logits alone, all
together) cycled over the shapes; the forward-only instantiation of the same case (prob and ll_part inside their bounds); the same launch
with row strides of I + 3, NaN responses under mask bytes 1 in the padding: bit for bit the same records -- which is also the second
launch that has to repeat the first.

Exact probes of split8: with no U and V = 1 (even hidden units) | 1 + 2^-11 (odd ones), h1 is (1, 0) | (1, 2^-11) in pieces exactly, so in
the `single` layout dW2_part[wave][n][k] = hi + lo of dz2[n] for even k and hi + lo + 2^-11 hi for odd k, while dvec_part row 0 is dz2[n]
itself: the DEVICE's two pieces and its split residual, element by element, have to be the model's (rtz16, then round-to-nearest f16 of
the rest, subnormals kept) at scales from both pieces normal down to dz2 on the subnormal grid.  The weight images have no such probe (no output isolates W_hi + W_lo): they are held through the bounds only.

A second probe (h_lo = 2^-20, |dz2| < 2^-20) measures how the MFMA adds a product of two subnormal pieces: not exactly -- the pipe aligns
by exponent fields and keeps 24 bits below the largest --, within one step of that window, which is what E_acc on nominal sizes allows.

VIBO_TOL_RECORD=path appends the worst error / bound per part, class and observable and the contraction bounds over the plain fp32 bound
(gpu_common.record, kind 'decoder_cells'); tools/split_record_table.py decoder_cells turns the file into
profiles/decoder_cells_record.txt.  The assertions hold either way."""
import time

import numpy as np
import pytest
import torch

import decoder_cells_common as C
from gpu_common import record
from oracle import decoder_model as D
from vibo_amd import decoder as DEC

pytestmark = pytest.mark.gpu

I_SET = (1, 15, 16, 17, 63, 64, 65, 130)
B_SET = (1, 2, 3, 7, 8, 9, 10)
MODE_LIST = tuple(C.MODES)
WHERES = ('first', 'later', 'last', 'last0')


@pytest.fixture(scope='module', autouse=True)
def _file_total():
    t0 = time.time()
    yield
    record('decoder_cells', time.time() - t0, part='time', **{'class': '-'}, observable='seconds of the whole file', ratio=0.0)


def chunk_choices(B):
    return sorted({1, min(2, B), (B + 1) // 2} | ({4} if B == 10 else set()))


def sweep(offset):
    """(B, I, person_chunks, mode) over every I, with B and the mode cycled by `offset`."""
    for j, I in enumerate(I_SET):
        B = B_SET[(j + offset) % len(B_SET)]
        for n, chunks in enumerate(chunk_choices(B)):
            yield B, I, chunks, MODE_LIST[(j + n + offset) % len(MODE_LIST)]


def test_the_sweeps_meet_every_shape_mode_and_loop_edge():
    seen = [s for o in range(len(D.CLASSES)) for s in sweep(o)]
    assert {s[1] for s in seen} == set(I_SET) and {s[0] for s in seen} == set(B_SET) and {s[3] for s in seen} == set(MODE_LIST)
    assert (10, 4) in {(s[0], s[2]) for s in seen}
    assert all(set(chunk_choices(B)) == {s[2] for s in seen if s[0] == B} for B in B_SET)
    lay = D.layout(10, 64, 4)
    assert lay.empty == [3]                                          # an empty chunk
    assert len(D.layout(10, 64, 1).pairs(0)) == 5 and D.layout(9, 64, 1).pairs(0)[-1] == (8, None)      # later pairs, an odd tail behind full pairs
    for o in range(len(D.CLASSES)):                                  # every class meets a chunk of more than one pair and an odd tail
        lays = [D.layout(B, I, c) for B, I, c, _ in sweep(o)]
        assert any(len(l.pairs(0)) >= 2 for l in lays) and any(l.pairs(c)[-1][1] is None for l in lays for c in range(l.chunks) if l.pairs(c))


def _one(cls, kind, B, I, chunks, mode, seed, where='first'):
    """One case: the gradient launch, the padded-stride launch (bit for bit), the forward-only launch.  -> (ratios, X, E, case)."""
    lay = D.layout(B, I, chunks)
    case = D.with_mask(D.make_case(cls, B, I, seed=100 * B + I, **C.MODES[mode]), D.masks(kind, lay, seed=seed, where=where))
    model = C.model_of(case, chunks)
    got = C.launch(case, chunks)
    r = C.ratios_of(got, case, model, kind)
    r['same bits under padded strides'] = 0.0 if C.same_bits(got, C.launch(case, chunks, pad=3)) else np.inf
    if r.get('dW2|dz2', 0.0) > 1.0:
        print('dW2|dz2 outside its bound:', (B, I, chunks, mode, seed), C.explain_dw2_given(got, case, model))
    fwd = C.launch(case, chunks, want_grad=False)
    r.update({'forward-only ' + k: v for k, v in D.ratios(fwd, model[1], model[2], model[0], names=('prob', 'll')).items()})
    if kind != 'dense' and 'dL' in got:
        r['unobserved dL exactly zero'] = 0.0 if np.all(got['dL'][np.asarray(case['mask']) == 0] == 0) else np.inf
    return r, model, case


def _run_sweep(cls, kind, seeds=(0,)):
    worst, failed, grade = {}, [], {}
    n_obs = n_excl = 0
    for seed in seeds:
        for B, I, chunks, mode in sweep(D.CLASSES.index(cls) + seed):
            r, (X, _, _, E, _), case = _one(cls, kind, B, I, chunks, mode, seed, WHERES[(seed + chunks) % 4])
            C.worse(worst, r)
            for k, (med, mx) in D.fp32_grade(case, X, E).items():
                grade[k] = (max(grade.get(k, (0, 0))[0], med), max(grade.get(k, (0, 0))[1], mx))
            n_obs, n_excl = n_obs + int(X['obs'].sum()), n_excl + int(X['excluded'].sum())
            if max(r.values()) > 1.0:
                failed.append((B, I, chunks, mode, seed, {k: v for k, v in r.items() if v > 1.0}))
    C.report(kind, cls, worst, grade)
    assert n_excl <= 0.02 * n_obs, (n_excl, n_obs)                   # 3PL cells within 4 ulp of a clamp value are asserted by nobody: at most 2 %
    assert not failed, failed


@pytest.mark.parametrize('cls', D.CLASSES)
def test_term_layout_every_term_against_its_own_bound(cls):
    _run_sweep(cls, 'term')


@pytest.mark.parametrize('cls', D.CLASSES)
def test_single_layout_one_outer_product_per_wave(cls):
    _run_sweep(cls, 'single', seeds=range(2))


def test_single_layout_observer_on_every_lane_of_every_wave():
    """Class unit at I = 130 (three item blocks, the last one ragged), B = 7 in one chunk: 16 seeds move the observer through every
    i16 lane of every wave; `where` moves it through the first pair, a later pair (r = 0, r = 1) and the odd tail."""
    worst, failed, lanes = {}, [], set()
    B, I, chunks = 7, 130, 1
    lay = D.layout(B, I, chunks)
    base = D.make_case('unit', B, I, seed=5, has_w1=True, resid=1.0, has_guess=True)
    X = None
    for seed in range(16):
        case = D.with_mask(base, D.masks('single', lay, seed=seed, where=WHERES[(seed // 2) % 4]))
        model = C.model_of(case, chunks)
        r = C.ratios_of(C.launch(case, chunks), case, model, 'single')
        C.worse(worst, r)
        lanes |= {(int(i) // 16, int(i) % 16, int(p)) for p, i in np.argwhere(case['mask'])}
        if max(r.values()) > 1.0:
            failed.append((seed, {k: v for k, v in r.items() if v > 1.0}))
    assert {(w, l) for w, l, _ in lanes} >= {(w, l) for w in range(8) for l in range(16)} and {p for _, _, p in lanes} >= {0, 1, 2, 3, 6}
    C.report('single-lanes', 'unit', worst)
    assert not failed, failed


@pytest.mark.parametrize('cls', D.CLASSES)
def test_dense_layout_summed_bounds_and_chains(cls):
    _run_sweep(cls, 'dense')


def test_empty_chunk_writes_exact_zeros():
    case = D.with_mask(D.make_case('unit', 10, 70, seed=3, has_w1=True, resid=1.0, has_guess=True), D.masks('dense', D.layout(10, 70, 4), seed=1))
    got = C.launch(case, 4)
    lay = D.layout(10, 70, 4)
    assert lay.empty == [3]
    waves = [lay.wave_id(3, ib, w) for ib in range(2) for w in range(4)]
    for k in ('ll_part', 'dW2_part', 'dvec_part'):
        assert np.all(got[k][waves] == 0), k
    assert np.all(got['dU_part'][3] == 0) and np.all(got['dguess_part'][3] == 0)
    assert all(np.isfinite(v).all() for v in got.values())           # every entry of every buffer was written


@pytest.mark.parametrize('hidden', [16, 32, 48])
def test_narrow_hidden_widths_through_the_padding(hidden):
    """decoder._pad_hidden's zero padding: the padded units' record entries are exactly zero, the rest inside the bounds."""
    B, I, chunks = 9, 65, 2
    case = D.make_case('unit', B, I, seed=hidden, has_w1=True, resid=1.0, has_guess=True, hidden=hidden)
    narrow = [None if case[k] is None else torch.from_numpy(case[k][..., :hidden]) for k in ('U', 'V')] + \
        [torch.from_numpy(case['W2'][:hidden, :hidden])] + [torch.from_numpy(case[k][:hidden]) for k in ('b2', 'w3', 'w1')]
    padded = DEC._pad_hidden(*narrow)
    for k, t in zip(('U', 'V', 'W2', 'b2', 'w3', 'w1'), padded):
        assert np.array_equal(t.numpy(), case[k]), k                 # the case IS what _pad_hidden hands the kernel
    worst = {}
    for kind in ('term', 'dense'):
        c = D.with_mask(case, D.masks(kind, D.layout(B, I, chunks), seed=hidden))
        got = C.launch(c, chunks)
        C.worse(worst, C.ratios_of(got, c, C.model_of(c, chunks), kind))
        h = hidden
        assert np.all(got['dW2_part'][:, h:, :] == 0) and np.all(got['dW2_part'][:, :, h:] == 0)
        assert np.all(got['dvec_part'][:, :3, h:] == 0) and np.all(got['dV_part'][:, :, h:] == 0) and np.all(got['dU_part'][:, :, h:] == 0)
    C.report(f'hidden-{hidden}', 'unit', worst)
    assert max(worst.values()) <= 1.0, worst


def _hi_flushed(x):
    """The alternative the probe has to tell apart: v_cvt_pkrtz flushing a subnormal hi to zero (lo then takes the whole value, rounded)."""
    hi = D.M.rtz16(x)
    hi = np.where(np.abs(hi) < 2.0 ** -14, 0.0, hi)
    return hi, D.rn16(x - hi)


PROBES = [('both-pieces-normal', 4.0, 2.0), ('unit', 0.25, 1.0), ('lo-at-the-subnormal-boundary', 2.0 ** -2, 0.3),
          ('hi-at-the-subnormal-boundary', 2.0 ** -13, 1.0), ('small_g', 2.0 ** -16, 1.0)]


@pytest.mark.parametrize('name,w3_scale,spread', PROBES, ids=[p[0] for p in PROBES])
def test_split8_pieces_are_the_models_element_by_element(name, w3_scale, spread):
    """No U, V = 1 in the even hidden units and 1 + 2^-11 in the odd ones: h1 = (1, 0) resp. (1, 2^-11) in pieces, exactly.  In the
    `single` layout dvec_part row 0 is dz2[n] itself and dW2_part[wave][n][k] = hi + lo of dz2[n] for even k, hi + lo + 2^-11 hi for odd k
    (every partial sum fits 24 bits): the DEVICE's two pieces of every dz2[n], element by element, against split_act -- and, for the
    record, against a conversion that flushes a subnormal hi.  Decides whether v_cvt_pkrtz, v_fma_mix and the MFMA's operands keep f16
    subnormals."""
    B, I, chunks = 7, 130, 1
    lay = D.layout(B, I, chunks)
    rng = np.random.default_rng(int(w3_scale * 2 ** 20))
    n_all = n_model = n_flushed = sub_lo = sub_hi = 0
    worst_dev = worst_model = 0.0
    for seed in range(4):
        case = D.make_case('unit', B, I, seed=seed, has_U=False)
        case['V'][:, 0::2], case['V'][:, 1::2] = 1.0, 1.0 + 2.0 ** -11
        case['w3'] = (rng.choice([-1.0, 1.0], D.H) * w3_scale * np.exp2(rng.uniform(-spread, spread, D.H))).astype(np.float32)
        case['W2'], case['b2'] = (case['W2'] * 0.02).astype(np.float32), (case['b2'] * 0.2).astype(np.float32)      # |o| stays small at any w3
        case = D.with_mask(case, D.masks('single', lay, seed=seed, where=WHERES[seed % 4]))
        got = C.launch(case, chunks)
        for p, i in np.argwhere(case['mask']):
            wid = lay.wave_id(0, i // 64, (i % 64) // 16)
            x = got['dvec_part'][wid, 0].astype(np.float64)           # dz2[n], the kernel's own
            dw = got['dW2_part'][wid].astype(np.float64)              # [n, k]
            assert np.all(x != 0) and np.all(dw[:, 0::2] == dw[:, :1]) and np.all(dw[:, 1::2] == dw[:, 1:2])
            dev_hi = (dw[:, 1] - dw[:, 0]) * 2.0 ** 11
            dev_lo = dw[:, 0] - dev_hi
            hi, lo = D.split_act(x)
            fh, fl = _hi_flushed(x)
            n_all += x.size
            n_model += int(((dev_hi == hi) & (dev_lo == lo)).sum())
            n_flushed += int(((dev_hi == fh) & (dev_lo == fl)).sum())
            worst_dev = max(worst_dev, float(np.abs(dw[:, 0] - x).max()))
            worst_model = max(worst_model, float(np.abs(hi + lo - x).max()))
            sub_lo += int(((np.abs(lo) < 2.0 ** -14) & (lo != 0)).sum())
            sub_hi += int(((np.abs(hi) < 2.0 ** -14) & (hi != 0)).sum())
    print(name, dict(entries=n_all, equal_to_model=n_model, equal_to_flushing_model=n_flushed, device_residual=worst_dev, model_residual=worst_model,
                     subnormal_lo=sub_lo, subnormal_hi=sub_hi))
    record('decoder_cells', worst_dev, part='split8-probe', **{'class': name}, observable='device residual', ratio=worst_dev / max(worst_model, 1e-300),
           entries=n_all, equal_to_model=n_model, equal_to_flushing_model=n_flushed, model_residual=worst_model, subnormal_lo=sub_lo, subnormal_hi=sub_hi)
    if name in ('hi-at-the-subnormal-boundary', 'small_g'):
        assert sub_hi > 0
    if name != 'both-pieces-normal':
        assert sub_lo > 0
    assert n_model == n_all, (n_model, n_flushed, n_all)


def test_mfma_aligns_subnormal_operands_by_their_exponent_field():
    """The same probe with h1 = (1, 2^-20) in pieces (a subnormal h_lo) and |dz2| < 2^-20, so that dz_hi = m 2^-24 with m <= 15 is
    subnormal too and hi + lo + 2^-20 hi still fits 24 bits: were every product of two pieces added exactly, dW2_part[n][odd k] -
    dW2_part[n][even k] would be m 2^-44.  The matrix pipe aligns by exponent fields (a subnormal counts as 2^-14) and keeps 24 bits below
    the largest, 2^-14 x 1 here: the small product comes back rounded to that window's step, 2^-38.  Held to one step -- what
    decoder_model's E_acc on nominal sizes allows --, the figures are printed and recorded."""
    B, I, chunks = 7, 130, 1
    lay = D.layout(B, I, chunks)
    rng = np.random.default_rng(20)
    step, n_all, n_exact, worst = 2.0 ** -38, 0, 0, 0.0
    for seed in range(2):
        case = D.make_case('unit', B, I, seed=seed, has_U=False)
        case['V'][:, 0::2], case['V'][:, 1::2] = 1.0, 1.0 + 2.0 ** -20
        case['w3'] = (rng.choice([-1.0, 1.0], D.H) * 2.0 ** -21 * np.exp2(rng.uniform(-1, 1, D.H))).astype(np.float32)
        case['W2'], case['b2'] = (case['W2'] * 0.02).astype(np.float32), (case['b2'] * 0.2).astype(np.float32)
        case = D.with_mask(case, D.masks('single', lay, seed=seed, where=WHERES[seed % 4]))
        got = C.launch(case, chunks)
        for p, i in np.argwhere(case['mask']):
            wid = lay.wave_id(0, i // 64, (i % 64) // 16)
            x = got['dvec_part'][wid, 0].astype(np.float64)
            dw = got['dW2_part'][wid].astype(np.float64)
            hi, lo = D.split_act(x)
            assert np.all(np.abs(x) < 2.0 ** -20) and np.all(dw[:, 0] == hi + lo)          # the even columns: both products against 1, exact
            dev = np.abs((dw[:, 1] - dw[:, 0]) - hi * 2.0 ** -20)
            n_all, n_exact, worst = n_all + x.size, n_exact + int((dev == 0).sum()), max(worst, float(dev.max()) / step)
    print(dict(entries=n_all, exact=n_exact, worst_in_steps_of_2_to_minus_38=worst))
    record('decoder_cells', worst, 1.0, part='mfma-subnormal-probe', **{'class': 'unit'}, observable='dz_hi x h_lo, both subnormal: error in steps of 2^-38',
           ratio=worst, entries=n_all, exact=n_exact)
    assert worst <= 1.0, worst


@pytest.mark.parametrize('cls', D.CLASSES)
def test_multi_sample_launch_returns_the_single_launchs_bits(cls):
    """One case per class through decoder._launch_multi(person_chunks=...): each sample's ll_part row equals the forward-only single launch's."""
    B, I, chunks = 9, 65, 2
    mode = MODE_LIST[D.CLASSES.index(cls) % len(MODE_LIST)]
    case = D.with_mask(D.make_case(cls, B, I, seed=17, **C.MODES[mode]), D.masks('dense', D.layout(B, I, chunks), seed=2))
    single = C.launch(case, chunks, want_grad=False)['ll_part']
    multi = C.launch_multi(case, chunks, S=2)
    assert multi.shape == (2, single.size)
    assert np.array_equal(multi[0].view(np.int32), single.view(np.int32)) and np.array_equal(multi[1].view(np.int32), single.view(np.int32))
