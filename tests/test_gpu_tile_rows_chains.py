"""The (person, dim) chains of the one-barrier batch loop (tile rows at 8 waves; csrc/vibo_msplit_kernel.hpp, `OB`) where the other
tile-row suites do not go: the chains' LDS addresses, the `r * A + ed` noise index and the `ones` plane of the logit operand are formed
once per launch from the wave's own slot, the slot's twelve running sums and five kept state values live in registers and reach LDS
once behind the loop, and the launch constants the chains test (who supplies the noise, which outputs exist, the regulariser's form)
sit in one scalar mask.

So: every ability_dim between the suites' 1 and 8; the sampled regulariser and dropped missing cells (the other values of the constants
in the mask); launches whose workgroups hold no batch, one batch and two batches side by side (the flush of the register sums); and the
drawing step replayed from a captured graph (the once-per-launch setup under replay).  The reference is the launch on the source rows
-- the two-barrier loop, which keeps the sums and the state in LDS and which the fp64-oracle suites hold -- compared with torch.equal."""
import contextlib
import functools

import pytest
import torch

from gpu_common import dev
from tile_rows_gpu_common import SEED, STREAM, assert_same_outputs, both, build, grid_of, host_rows, problem, strided
from vibo_amd import _lib, ops

pytestmark = pytest.mark.gpu

I = 1000


def persons(a, b, tail=0):
    """32 (a G + b) + tail rows: a G + b batches over the launch's G workgroups."""
    return 32 * (a * grid_of(I) + b) + tail


@functools.lru_cache(maxsize=1)
def all_rows():
    """Host rows of the largest shape (and one more), made once; every case takes P rows from row `first` on (host_rows: row 0 all
    missing, row 1 all observed, one item column all missing)."""
    return host_rows(persons(2, 1, 7) + 1, I, seed=23)


@functools.lru_cache(maxsize=4)
def device_case(P, first=0):
    resp, mask = all_rows()
    resp, mask = resp[first:first + P], mask[first:first + P]
    r, m = strided(resp, (I + 3) & ~3, 1.0), strided(mask.to(torch.uint8), (I + 3) & ~3, 1)
    return r, m, build(r, m, _lib.MASK_U8, P), int(mask.sum())


# ---------------------------------------------------------------------------
# every ability_dim between 1 and 8
# ---------------------------------------------------------------------------
MODELS = [(2, A) for A in (2, 3, 4, 5, 6, 7)] + [(1, 3), (3, 3)]


@pytest.mark.parametrize('shape', ['2G+1 batches, tail 7', 'one partial batch'])
@pytest.mark.parametrize('irt,A', MODELS, ids=[f'{irt}pl-a{A}' for irt, A in MODELS])
def test_every_ability_dim(irt, A, shape):
    """Gradients with given noise, forward only, the drawing step: rows against image, and the image twice."""
    P = persons(2, 1, 7) if shape.startswith('2G') else 39
    r, m, image, n_obs = device_case(P)
    spec, table, item = problem(irt, A, I)
    for want_grad, draw in ((True, False), (False, False), (True, True)):
        ref, got = both(spec, r, m, _lib.MASK_U8, image, table, item, want_grad=want_grad, draw=draw)
        assert_same_outputs(ref, got, n_obs, want_grad=want_grad, draw=draw)
        _, again = both(spec, r, m, _lib.MASK_U8, image, table, item, want_grad=want_grad, draw=draw)
        assert_same_outputs(got, again, n_obs, want_grad=want_grad, draw=draw)


# ---------------------------------------------------------------------------
# the other values of the launch constants
# ---------------------------------------------------------------------------
@contextlib.contextmanager
def pinned(r, m, image, tiles):
    """both()'s monkeypatch block for one launch: the matrix kernel pinned, the image (or the source rows) through the resident-matrix
    record; yields the list the launch's mask format is logged to."""
    sent, real_call = [], ops._call

    def logging_call(name, *args):
        if name.startswith('vibo_elbo_fwd_bwd'):
            sent.append(args[0]._obj.mask_dtype)
        return real_call(name, *args)
    with pytest.MonkeyPatch.context() as mp, ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        mp.setattr(ops, '_call', logging_call)
        mp.setattr(ops, 'SIGN_ROWS', False)
        mp.setattr(ops, 'TILE_ROWS_MIN_PERSONS', 1)
        mp.setattr(ops, 'TILE_ROWS_PLAIN_LAUNCHES', True)
        mp.setattr(ops, 'TILE_ROWS', tiles)
        rec = ops.ResidentMatrix(r, m)
        rec.tiles = image
        r._vibo_row_counts = rec
        try:
            yield sent
        finally:
            del r._vibo_row_counts


def both_with(spec, reg_mode, r, m, image, table, item):
    """both() with gradients and given noise, under the caller's spec and regulariser mode."""
    P = r.shape[0]
    eps = torch.randn(P, spec.ability_dim, generator=torch.Generator().manual_seed(P)).to(dev())
    out = []
    for tiles in (False, True):
        with pinned(r, m, image, tiles) as sent:
            out.append(ops._hip_launch_elbo(spec, r, m, _lib.MASK_U8, None, table, item, eps, None, reg_mode, True, P))
        assert sent == [_lib.MASK_TILES if tiles else _lib.MASK_U8], sent
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('A', [1, 8])
@pytest.mark.parametrize('batches', ['2G+1 batches, tail 7', 'G+1 batches'])
@pytest.mark.parametrize('form', ['REG_SAMPLED', 'drop_missing'])
def test_sampled_regulariser_and_dropped_missing_cells(form, batches, A):
    P = persons(2, 1, 7) if batches.startswith('2G') else persons(1, 1)
    # (a person without a single answer has no posterior once the missing cells' prior experts are dropped -- precision 0, NaN in the
    #  reference model as well: those launches start at row 1)
    r, m, image, n_obs = device_case(P, first=1 if form == 'drop_missing' else 0)
    _, table, item = problem(2, A, I)
    spec = ops.ElboSpec(irt_model=2, ability_dim=A, drop_missing=form == 'drop_missing')
    reg_mode = _lib.REG_SAMPLED if form == 'REG_SAMPLED' else _lib.REG_KL
    ref, got = both_with(spec, reg_mode, r, m, image, table, item)
    assert_same_outputs(ref, got, n_obs)
    # (the constants do reach the kernel: the launch differs from the plain one)
    plain, _ = both_with(ops.ElboSpec(irt_model=2, ability_dim=A), _lib.REG_KL, r, m, image, table, item)
    assert not torch.equal(plain.flat, ref.flat)


# ---------------------------------------------------------------------------
# the sums that leave the registers once
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('draw', [False, True], ids=['given noise', 'drawing step'])
@pytest.mark.parametrize('population', ['G-1 batches', 'G+1 batches and a row'])
def test_sums_flushed_from_registers(population, draw):
    """Two workgroup populations in one launch: G - 1 batches leave a workgroup without a batch (its sums: zeros), G + 1 batches and a
    row give workgroup 0 two full batches, workgroup 1 a full one and a one-row one, and the rest one each.  The table-gradient block
    (terms k < 8 of the running sums) and the scalars the terms 8..11 end in -- kl | logq0 | logp | nobs, with the regulariser they
    sum to and the flows' (zero) log-det beside them: entries 1..6 of `flat` -- entry for entry."""
    P = persons(1, -1) if population.startswith('G-1') else persons(1, 1, 1)
    r, m, image, n_obs = device_case(P)
    spec, table, item = problem(2, 8, I)
    ref, got = both(spec, r, m, _lib.MASK_U8, image, table, item, want_grad=True, draw=draw)
    n = _lib.NUM_SCALARS
    for k in (_lib.S_REG, _lib.S_KL, _lib.S_LOGQ0, _lib.S_LOGP, _lib.S_LADJ, _lib.S_NOBS):
        assert torch.equal(ref.flat[k], got.flat[k]), (k, float(ref.flat[k]), float(got.flat[k]))
    assert int(got.flat[_lib.S_NOBS]) == n_obs and float(got.flat[_lib.S_KL]) != 0.0
    tab_ref, tab_got = ref.flat[n:n + 2 * ref.n_table], got.flat[n:n + 2 * got.n_table]
    assert bool((tab_ref != 0).any()) and not torch.isnan(tab_ref).any()
    assert torch.equal(tab_ref, tab_got), (tab_ref - tab_got).abs().max()
    assert_same_outputs(ref, got, n_obs, draw=draw)


# ---------------------------------------------------------------------------
# a captured replay
# ---------------------------------------------------------------------------
def test_captured_drawing_step_replays_as_eager():
    """The drawing step on the image, captured once and replayed three times, against three eager calls: the same bits call by call."""
    P = persons(2, 1)
    r, m, image, n_obs = device_case(P)
    spec, table, item = problem(2, 8, I)

    def new_tick():
        return torch.tensor([0, 7], dtype=torch.int32, device=dev())

    def step(tick):
        return ops._hip_launch_elbo(spec, r, m, _lib.MASK_U8, None, table, item, None, None, _lib.REG_KL, True, P,
                                    train_step=(tick, False, (SEED, STREAM), True))
    with pinned(r, m, image, True) as sent:
        tick_e, tick_g = new_tick(), new_tick()
        eager = [step(tick_e).flat.clone() for _ in range(3)]
        torch.cuda.synchronize()
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                out = step(tick_g)
        torch.cuda.current_stream().wait_stream(side)
        replayed = []
        for _ in range(3):
            graph.replay()
            replayed.append(out.flat.clone())
        torch.cuda.synchronize()
    assert sent == [_lib.MASK_TILES] * 4, sent
    assert torch.equal(tick_e, tick_g)
    assert int(eager[0][_lib.S_NOBS]) == n_obs and not torch.isnan(eager[0]).any()
    for k, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, b), (k, float((a - b).abs().max()))
