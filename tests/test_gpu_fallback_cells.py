"""The three fallback ELBO kernels -- tiled (csrc/vibo_elbo_kernel.hpp), wave-per-row (csrc/vibo_row_kernel.hip) and wave-per-person
(csrc/vibo_general.hip) -- output by output, and over more than one trip through their persistent loops.

tests/test_gpu_parity.py and four goldens compare aggregates on N(0, 1) inputs, and no launch there gives a workgroup of the tiled
kernel a second tile, a wave of the wave-per-row kernel a row for its second register set, or a wave of the wave-per-person kernel a
second row.  Here EVERY entry of every output is held to a bound of its own, counted in oracle/fallback_model.py from the kernel's
statements and the inputs alone; the float32 emulations of those statements are held to the same bounds on the same cases in
tests/test_fallback_model.py, where each mutation of the trip structure leaves one.  No kernel pin (ops.DESC_FLAGS == 0): every launch
asserts the kernel the planner names for a descriptor with the rows' own strides (ops.plan_kernel assumes strides padded to four
cells, which tight ragged rows do not have), and hands the name to launch_elbo wherever ops.plan_kernel can answer.  The C ABI
exposes no grid, so trips are taken from the geometry functions, which tests/test_fallback_model.py holds against the planner's
source.  theta is what the kernel returns; the cell reference is built from it.

 (a) edges, one trip (fallback_model.EDGES): tiled at 1 ... 1023 items on tight rows (the scalar phase A; every waves boundary, the
     16-item block tail, every tail_words case) and at I % 4 == 0 under int64 masks (the vector phase A), ability_dim 1 ... 8, B = 1, 63,
     64, 65, 130, gathered rows, --drop-missing, forward only; wave-per-row at 192 ... 1024 items on both sides of each CH limit;
     wave-per-person at ability_dim 9, 12, 16 and, through tight rows of 1027 items,
     3 and 8, u8 / int64 / no mask, each side of the 40 / 80 / 150 KiB thresholds of its LDS item slab.  Entries whose reference is an
     exact zero have a zero bound.  A matrix handed over one float past a 16-byte boundary: every output bit for bit that of the
     aligned launch.  NaN responses under mask value 1 between a row's end and its stride change no output bit.
 (b) more than one trip (fallback_model.TRIPS): B from the geometry so that every workgroup / wave takes at least two trips and some a
     third; one observer per item, placed in the first trip, a later one and the ragged end.  Every output against its bound; every
     posterior entry bit for bit that of the same rows launched in single-trip slices; tiled and wave-per-row: a second launch of the
     same call returns the same bits.  Dense launches (30 % missing, fallback_model.DENSE) against the summed bounds with the counted
     chain.
Found by this file and fixed in csrc/vibo_elbo_kernel.hpp: the tiled kernel returned a sample recomputed in its epilogue, which the
compiler rounded differently from the one in the tile's share that the cells used (d LL / d a up to 24 x its bound where mean and noise
cancel); it now returns the share's.  The forward-only instantiations still round mu and theta differently from the gradient ones
(<= 1 ulp): each launch is held to its own bounds, not to the other's bits.
The wave-per-person kernel's cases cross ability_dim 9 / 12 / 16 and 3 / 8 with the plain and the conditional posterior, planar flows
1, 2 and 8 (theta_K, the log-determinants, S_LADJ and the flow gradients per entry), 1PL / 2PL / 3PL, u8 / int64 / no mask,
--drop-missing and REG_KL / REG_SAMPLED; encode_kernel is held on the same rows through ops.encode_posterior.

VIBO_TOL_RECORD=path appends the worst error / bound per observable (gpu_common.record, kind 'fallback_cells');
tools/split_record_table.py fallback_cells turns the file into profiles/fallback_cells_record.txt."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_common import dev, launch_elbo, record
from oracle import fallback_model as Fm
from oracle import narrow_model as N
from oracle import split_model as M
from test_gpu_narrow_cells import _outputs
from vibo_amd import _lib, ops
from vibo_amd.ops import ElboSpec

pytestmark = pytest.mark.gpu


def _num_cu():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def _planned(spec, B, resp, mask, code, want_grad, reg_mode):
    """The kernel vibo_plan_kernel names for the descriptor of THESE rows (their own strides): ops._rows_desc on the prepared rows, the
    call ops._hip_launch_elbo itself makes for the launch (launch_elbo prepares the rows the same way, ops.prepare_rows)."""
    d = ops._rows_desc(spec, B, resp, mask, code, reg_mode, want_grad)
    return _lib.KERNEL_NAMES[_lib.load().vibo_plan_kernel(ctypes.byref(d))]


def _device_rows(c, case, pad_nan=False):
    """-> (resp, mask, row_index) on the device as the case asks: tight rows; 'gather': scattered over a matrix with 7 decoy rows;
    'view': the matrix one float past a 16-byte boundary.  pad_nan: rows of stride I + 4 whose padding holds NaN under mask 1."""
    d = dev()
    resp, obs = torch.from_numpy(case['resp']), torch.from_numpy(np.asarray(case['obs'], bool))
    B, I = resp.shape
    index = None
    if c['rows'] == 'gather':
        P = B + 7
        index = torch.randperm(P, generator=torch.Generator().manual_seed(B + I))[:B]
        resp_all = (torch.rand(P, I, generator=torch.Generator().manual_seed(I)) < 0.5).float()
        obs_all = torch.ones(P, I, dtype=torch.bool)
        resp_all[index], obs_all[index] = resp, obs
        resp, obs, index = resp_all, obs_all, index.to(d)
    mdt = {'u8': torch.bool, 'i64': torch.int64}.get(c['mask'])
    resp, mask = resp.to(d), (obs.to(d).to(mdt) if mdt is not None else None)
    if pad_nan:
        n = resp.shape[0]
        rbuf = torch.full((n, I + 4), float('nan'), device=d)
        rbuf[:, :I] = resp
        resp = rbuf[:, :I]
        if mask is not None:
            mbuf = torch.ones(n, I + 4, dtype=mask.dtype, device=d)
            mbuf[:, :I] = mask
            mask = mbuf[:, :I]
    if c['rows'] == 'view':
        buf = torch.zeros(resp.numel() + 8, device=d)
        assert buf.data_ptr() % 16 == 0
        buf[1:1 + resp.numel()] = resp.reshape(-1)
        resp = buf[1:1 + resp.numel()].view(resp.shape)
        assert resp.data_ptr() % 16 == 4
    return resp, mask, index


def _launch(c, case, table, eps, want_grad=None, rows=None):
    assert ops.DESC_FLAGS == 0
    want_grad = c['grad'] if want_grad is None else want_grad
    A, I = case['a'].shape[1], case['resp'].shape[1]
    spec = ElboSpec(irt_model=case['irt'], ability_dim=A, drop_missing=c['drop'], conditional=c['cond'], n_flows=c['flows'])
    reg_mode = _lib.REG_KL if c['reg'] == 'kl' else _lib.REG_SAMPLED
    resp, mask, index = _device_rows(c, case) if rows is None else rows
    r2, m2, code = ops.prepare_rows(resp, mask, keep_int64=True)
    assert r2.data_ptr() == resp.data_ptr()              # (no repacking of the responses: a view or padding under test has to survive)
    B = int(index.numel()) if index is not None else resp.shape[0]
    assert _planned(spec, B, r2, m2, code, want_grad, reg_mode) == c['kernel'], (Fm.case_id(c), _planned(spec, B, r2, m2, code, want_grad, reg_mode))
    chunkable = I % 4 == 0 and I >= 4                    # (what ops.plan_kernel assumes of the strides holds for these rows)
    raw = launch_elbo(spec, resp, mask, torch.from_numpy(table), torch.from_numpy(M.item_tensor(case)), torch.from_numpy(eps),
                      mask_dtype=mask.dtype if mask is not None else torch.bool, keep_int64=True, row_index=index, want_grad=want_grad,
                      reg_mode=reg_mode, flow=torch.from_numpy(case['flow']) if c['flows'] else None,
                      kernel=c['kernel'] if chunkable else None)
    return spec, raw


def _all_outputs(spec, raw, case, c, want_grad):
    """test_gpu_narrow_cells._outputs plus, with flows, theta_K, the log-determinants, S_LADJ and both flow-gradient heads."""
    I, A = case['resp'].shape[1], c['A']
    got = _outputs(spec, raw, I, want_grad=want_grad)
    if c['flows']:
        flat = raw.flat.cpu().numpy()
        got.update(ability_k=raw.ability_k.cpu().numpy(), ladj=raw.ability_ladj.cpu().numpy(), S_LADJ=flat[_lib.S_LADJ])
        if want_grad:
            o = _lib.NUM_SCALARS + 2 * raw.n_table + raw.n_item
            gf = flat[o:o + 2 * raw.n_flow].reshape(2, c['flows'], 2 * A + 1)
            got['grad_flow'] = [gf[0], gf[1]]
    return got


def _same_bits(a, b, want_grad):
    flat = (a.flat, b.flat) if want_grad else (a.scalars, b.scalars)
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in
               (flat, (a.ability_mu, b.ability_mu), (a.ability_logvar, b.ability_logvar), (a.ability, b.ability)))


def _report(part, c, r, trips=None):
    for k, v in sorted(r.items()):
        record('fallback_cells', v, part=part, kernel=c['kernel'], case=Fm.case_id(c), observable=k, ratio=v, trips=trips)
    print(part, Fm.case_id(c), trips, {k: round(v, 3) for k, v in r.items()})


def _held(c, case, table, eps, cu, want_grad=None, rows=None):
    want_grad = c['grad'] if want_grad is None else want_grad
    spec, raw = _launch(c, case, table, eps, want_grad, rows=rows)
    got = _all_outputs(spec, raw, case, c, want_grad)
    assert np.abs(got['theta'] - case['theta_oracle']).max() < 2e-5 * max(1.0, np.abs(case['theta_oracle']).max()), 'theta'
    # the cell reference is built from the sample the cells ran on: theta, with flows theta_K
    exp = Fm.expected_of(dict(c, grad=want_grad), case, table, eps, got.get('ability_k', got['theta']), cu)
    if want_grad:                                        # an item nobody observes: every output it feeds is an exact zero
        dead = ~np.asarray(case['obs'], bool).any(0)
        assert not got['g_item'][dead].any(), ('unobserved items', np.flatnonzero(dead))
        if c['cond']:
            assert not any(g[:, dead].any() for g in got['g_table']), 'table gradient of unobserved items'
    return raw, got, exp, Fm.ratios(exp, got, case['irt'], c['A'])


def _regime(c, case, exp):
    """The generators' shares on the reference built from the kernel's own sample: at most 2 % of the observed cells left out, |l| <= 3
    on 0.8 of them (bias: 0.7, the shared generator gives 0.75 by construction; clamp3 places its cells at the clamp)."""
    n_obs = int(np.asarray(case['obs']).sum())
    assert int(exp['excluded'].sum()) <= max(1, 0.02 * n_obs), ('excluded', int(exp['excluded'].sum()), n_obs)
    n_l3, n = exp['logit_share']
    if n >= 16 and c['cls'] != 'clamp3' and c['mask'] != 'none':
        assert n_l3 >= (0.7 if c['cls'] == 'bias' else 0.8) * n, ('|l| <= 3', n_l3, n)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) edges, one trip
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', Fm.EDGES, ids=Fm.case_id)
def test_every_entry_at_the_edges(c):
    cu = _num_cu()
    case, table, eps = Fm.problem(c, cu)
    assert Fm.plan_of(c, Fm.persons(c, cu), cu)['trips'][1] == 1
    raw, got, exp, r = _held(c, case, table, eps, cu)
    _report('edges', c, r)
    _regime(c, case, exp)
    assert max(r.values()) <= 1.0, r
    for i in Fm.unobserved_of(c):
        assert not case['obs'][:, i].any()
    if c['grad']:
        # forward only is another instantiation (the compiler contracts its posterior differently: not the same bits): its own bounds
        _, gf, _, rf = _held(c, case, table, eps, cu, want_grad=False)
        assert max(rf.values()) <= 1.0, rf


ALIGNED = Fm._case('tiled', 'cancel', 3, 148, 65, mask='i64')


def test_a_matrix_one_float_past_a_16_byte_boundary_gives_the_same_bits():
    """vec_ok is false for the view (the scalar phase A), the codes in LDS and the grid are the same: every output bit for bit."""
    cu = _num_cu()
    case, table, eps = Fm.problem(ALIGNED, cu)
    _, base = _launch(ALIGNED, case, table, eps)
    _, view = _launch(dict(ALIGNED, rows='view'), case, table, eps)
    assert _same_bits(view, base, True)


PADDED = [Fm._case('tiled', 'cancel', 3, 148, 65, mask='i64'), Fm._case('tiled', 'threepl', 2, 3, 65, rows='gather'),
          Fm._case('wave-per-row', 'cancel', 2, 260, 9, mask='i64', rows='gather'), Fm._case('wave-per-person', 'cancel', 12, 65, 9, mask='i64')]


@pytest.mark.parametrize('c', PADDED, ids=Fm.case_id)
def test_padding_cells_are_never_interpreted(c):
    case, table, eps = Fm.problem(c, _num_cu())
    for want_grad in (True, False):
        _, base = _launch(c, case, table, eps, want_grad)
        _, out = _launch(c, case, table, eps, want_grad, rows=_device_rows(c, case, pad_nan=True))
        assert torch.isfinite(out.flat).all() if want_grad else torch.isfinite(out.scalars).all(), 'finite'
        if c['kernel'] == 'wave-per-person':                     # (atomics: the sums are not bitwise reproducible, the posterior is)
            assert torch.equal(out.ability, base.ability) and torch.equal(out.ability_mu, base.ability_mu)
            assert torch.equal(out.ability_logvar, base.ability_logvar) and torch.equal(out.scalars[_lib.S_NOBS], base.scalars[_lib.S_NOBS])
            # ... and every entry of the padded launch stays inside its own bound: a padding cell in a gradient would leave it
            _, _, _, r = _held(c, case, table, eps, _num_cu(), want_grad, rows=_device_rows(c, case, pad_nan=True))
            assert max(r.values()) <= 1.0, r
        else:
            assert _same_bits(out, base, want_grad), Fm.case_id(c)


ENCODE = [c for c in Fm.EDGES if not c['flows'] and (c['kernel'] == 'wave-per-person' or (c['kernel'] == 'tiled' and c['mask'] == 'u8'))]


def _encode_takes_the_wave_per_person_kernel(c, resp, mask, code):
    """vibo_encode's rule on the rows as ops.encode_posterior prepares them: encode_scratch_bytes == 0 (ability_dim > 8, fewer than 4
    items, an int64 mask, rows not chunkable in 4 cells) or rows_vec_ok false (strides or base pointers off 16 / 4 bytes)."""
    I, i4 = c['I'], (c['I'] + 3) & ~3
    if c['A'] > 8 or I < 4 or code == _lib.MASK_I64:
        return True
    chunkable = I % 4 == 0 or (resp.stride(0) >= i4 and (code != _lib.MASK_U8 or mask.stride(0) >= i4))
    vec = chunkable and resp.stride(0) % 4 == 0 and resp.data_ptr() % 16 == 0 and \
        (code != _lib.MASK_U8 or (mask.stride(0) % 4 == 0 and mask.data_ptr() % 4 == 0))
    return not vec


@pytest.mark.parametrize('c', ENCODE, ids=Fm.case_id)
def test_encode_kernel_entry_by_entry(c):
    """The same rows through ops.encode_posterior.  vibo_encode hands them to the wave-per-person encode_kernel (vibo_helpers.hip)
    where ability_dim exceeds 8 or the rows cannot be read in 16-byte chunks (tight rows of I % 4 != 0 or fewer than 4 items under a
    byte mask; it narrows int64 masks to bytes first): vibo_capi.hip, vibo_encode, `need > 0 && rows_vec_ok(...)` takes encode_fast,
    everything else encode_kernel, with need = encode_scratch_bytes (vibo_planner.hip: 0 above ability_dim 8 and outside
    row_split_shape).  The C ABI exposes neither figure (vibo_workspace_bytes is the maximum over the ELBO plan), so the rule is
    restated in _encode_takes_the_wave_per_person_kernel and asserted per case; a change of the rule in the library has to change it.  mu and
    logvar per entry against encode_kernel's own bound (__expf at (2 |s| + 2) u), and within the summed bounds of the ELBO launch's
    posterior on the same rows."""
    cu = _num_cu()
    case, table, eps = Fm.problem(c, cu)
    spec, raw = _launch(c, case, table, eps, want_grad=False)
    resp, mask, index = _device_rows(c, case)
    assert _encode_takes_the_wave_per_person_kernel(c, *ops.prepare_rows(resp, mask))
    mu, logvar = ops.encode_posterior(spec, torch.from_numpy(table).to(dev()), resp, mask, row_index=index)
    torch.cuda.synchronize()
    got = dict(mu=mu.cpu().numpy().astype(np.float64), logvar=logvar.cpu().numpy().astype(np.float64))
    enc = Fm.expected_encode(case, table, drop_missing=c['drop'])
    elbo = Fm.expected_of(dict(c, grad=False), case, table, eps, raw.ability.cpu().numpy(), cu)
    worst = {}
    for k, t in (('mu', raw.ability_mu), ('logvar', raw.ability_logvar)):
        # (a person without answers has mu = 0 exactly: a zero bound admits no error)
        ratio = lambda err, bnd: float(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0)).max())
        worst['encode ' + k] = ratio(np.abs(got[k] - enc[k][0]), enc[k][1])
        worst['encode - elbo ' + k] = ratio(np.abs(got[k] - t.cpu().numpy().astype(np.float64)), enc[k][1] + elbo[k][1])
    _report('encode', c, worst)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------------
# (b) more than one trip
# ---------------------------------------------------------------------------------------------------------------------------
def _single_trip_rows(c, cu):
    """Persons one launch takes in a single trip of every workgroup / wave."""
    if c['kernel'] == 'tiled':
        return Fm.TILE * cu * Fm.tiled_plan(1 << 30, c['I'], c['A'], cu)['per_cu']
    if c['kernel'] == 'wave-per-row':
        return 4 * 2 * cu
    return 4 * cu * Fm.general_plan(1 << 30, c['I'], Fm.item_dim(c), c['grad'], cu)['per_cu']


def _slices_bit_identical(c, case, table, eps, full, cu):
    B, step = case['resp'].shape[0], _single_trip_rows(c, cu)
    for lo in range(0, B, step):
        sl = slice(lo, min(B, lo + step))
        assert Fm.plan_of(c, sl.stop - sl.start, cu)['trips'][1] == 1
        part = dict(case, resp=case['resp'][sl], obs=case['obs'][sl])          # (table, items and flows are the launch's own)
        _, raw = _launch(c, part, table, eps[sl])
        for k, t in (('mu', raw.ability_mu), ('logvar', raw.ability_logvar), ('theta', raw.ability)) + \
                ((('ability_k', raw.ability_k), ('ladj', raw.ability_ladj)) if c['flows'] else ()):
            if not np.array_equal(t.cpu().numpy(), full[k][sl]):
                return False
    return True


@pytest.mark.parametrize('c', Fm.TRIPS, ids=Fm.case_id)
def test_more_than_one_trip(c):
    cu = _num_cu()
    B = Fm.persons(c, cu)
    trips = Fm.plan_of(c, B, cu)['trips']
    assert trips[0] >= 2 and trips[1] >= 3, trips            # precondition: every workgroup / wave takes two trips, some a third
    if c['kernel'] == 'wave-per-person':
        assert Fm.lds_regimes_met(cu)                        # (k = 4 with the LDS item slab, k = 1 with it, and no slab at all)
    worst, failed = {}, []
    for shift in Fm.shifts(c, B):
        case, table, eps = Fm.problem(c, cu, shift=shift)
        assert case['p_obs'].min() == shift and case['p_obs'].max() == shift + c['I'] - 1
        raw, got, exp, r = _held(c, case, table, eps, cu)
        _regime(c, case, exp)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        same = _slices_bit_identical(c, case, table, eps, got, cu)
        again = True
        if c['kernel'] != 'wave-per-person':
            _, second = _launch(c, case, table, eps)
            again = _same_bits(second, raw, c['grad'])
        if max(r.values()) > 1.0 or not same or not again:
            failed.append((shift, {k: v for k, v in r.items() if v > 1.0}, same, again))
    _report('trips', c, worst, trips)
    assert not failed, failed


@pytest.mark.parametrize('c', Fm.DENSE, ids=Fm.case_id)
def test_dense_launch_over_several_trips_with_the_counted_chain(c):
    cu = _num_cu()
    B = Fm.persons(c, cu)
    trips = Fm.plan_of(c, B, cu)['trips']
    assert trips[0] >= 2 and trips[1] >= 3, trips
    case, table, eps = Fm.problem(c, cu, missing=0.3)
    raw, got, exp, r = _held(c, case, table, eps, cu)
    r.pop('logit', None)
    _report('dense', c, r, trips)
    assert int(exp['excluded'].sum()) <= 0.02 * int(np.asarray(case['obs']).sum()), ('excluded', int(exp['excluded'].sum()))
    assert max(r.values()) <= 1.0, r
