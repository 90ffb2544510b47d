"""The chain waves of the matrix kernel on tile rows (csrc/vibo_msplit_kernel.hpp, `CW`; vibo_variant.hpp, ms_chain_waves): at 8 tile
waves (897..1024 items), with gradients, 1PL and 2PL, the (person, dim) chains of every batch run on waves 8-11 of a 768-thread
workgroup -- one per SIMD, each the owner of one slot of BOTH batch parities, with two sets of the running sums, the kept state and the
held LDS addresses -- and waves 0-7 run tiles only.

So: the 8-wave range's edge, the benchmark's width and the full width; the corners of the slot-lane mapping (ability_dim 1, 2, 7, 8);
both models; launches in which neighbouring workgroups hold 0 | 1, 1 | 2, 2 | 3, 3 | 4 and 4 | 5 batches (a workgroup's batch counts
differ by one at most within a launch), the extra batch of the last of them a partial one -- both parities at the tail, the sums of a
workgroup without a batch, the backward behind the loop on either register set; the caller's noise and the drawn one, with the
per-person outputs given, the sample alone, and none; the other values of the launch constants the chains test (the sampled regulariser,
dropped missing cells); a captured replay; and 3PL and forward-only launches, which keep the form without chain waves.

The standard is that of test_gpu_tile_rows_one_barrier.py / test_gpu_tile_rows_chains.py, whose helpers this file uses: every output of
the launch on the image against the launch on the source rows -- the two-barrier loop on eight waves, which the fp64-oracle suites
hold -- with torch.equal, and every launch on the image twice: a race between the chain waves and the tile waves would show there."""
import functools

import pytest
import torch

from gpu_common import dev
from test_gpu_tile_rows_chains import pinned
from test_gpu_tile_rows_one_barrier import same_outputs
from tile_rows_gpu_common import SEED, STREAM, build, grid_of, host_rows, problem, strided
from vibo_amd import _lib, ops

pytestmark = pytest.mark.gpu

ITEMS = (897, 1000, 1024)
DIMS = (1, 2, 7, 8)
# neighbouring workgroups with a | a + 1 batches: a G + 3 batches over the launch's G workgroups (workgroups 0-2 hold the extra one),
# the last of them 7 rows
POPULATIONS = {'0|1': 0, '1|2': 1, '2|3': 2, '3|4': 3, '4|5': 4}
TAIL = 7
NOISE = ('given', 'drawn, no outputs', 'drawn, sample kept')


def persons(a):
    return 32 * (a * grid_of(1024) + 2) + TAIL


@functools.lru_cache(maxsize=1)
def all_rows():
    """Host rows of the largest shape (and one more) at the full width, made once: every case takes P rows from row `first` on and the
    first I columns (host_rows: row 0 all missing, row 1 all observed, item column 2 all missing)."""
    return host_rows(persons(max(POPULATIONS.values())) + 1, max(ITEMS), seed=31)


@functools.lru_cache(maxsize=2)
def device_case(I, a, first=0):
    """(response, u8 mask, image, observed cells) on the device, never written."""
    P = persons(a)
    resp, mask = all_rows()
    resp, mask = resp[first:first + P, :I], mask[first:first + P, :I]
    r, m = strided(resp, (I + 3) & ~3, 1.0), strided(mask.to(torch.uint8), (I + 3) & ~3, 1)
    return r, m, build(r, m, _lib.MASK_U8, P), int(mask.sum())


def launch(spec, reg_mode, r, m, image, table, item, noise, tiles, want_grad=True):
    """One launch, matrix kernel pinned, on the source rows or (tiles) on their image.  noise: the caller's, with the three per-person
    outputs; or the folded step's own draws with no per-person output, or with the sample alone."""
    P = r.shape[0]
    eps, step = None, None
    if noise == 'given':
        eps = torch.randn(P, spec.ability_dim, generator=torch.Generator().manual_seed(P)).to(dev())
    else:
        step = (torch.tensor([0, 7], dtype=torch.int32, device=dev()), False, (SEED, STREAM), noise == 'drawn, no outputs')
    with pinned(r, m, image, tiles) as sent:
        out = ops._hip_launch_elbo(spec, r, m, _lib.MASK_U8, None, table, item, eps, None, reg_mode, want_grad, P, train_step=step)
    torch.cuda.synchronize()
    assert sent == [_lib.MASK_TILES if tiles else _lib.MASK_U8], sent
    return out


def rows_image_image(spec, reg_mode, case, I, table, item, noise, want_grad=True):
    """The launch on the rows, then the launch on the image twice: every output of the three the same bits."""
    r, m, image, n_obs = case
    ref = launch(spec, reg_mode, r, m, image, table, item, noise, False, want_grad)
    for _ in range(2):
        got = launch(spec, reg_mode, r, m, image, table, item, noise, True, want_grad)
        if noise == 'drawn, sample kept':       # (the gradients and scalars as same_outputs holds them; of the per-person outputs the sample)
            assert got.ability_mu is None and ref.ability_mu is None and got.ability_logvar is None
            assert not torch.isnan(ref.flat).any() and torch.equal(ref.flat, got.flat), float((ref.flat - got.flat).abs().max())
            assert not torch.isnan(ref.ability).any() and torch.equal(ref.ability, got.ability)
        else:
            same_outputs(ref, got, n_obs, I, want_grad=want_grad, draw=noise == 'drawn, no outputs')
    return ref


@pytest.mark.parametrize('I,population', [(I, k) for I in ITEMS for k in POPULATIONS])
def test_image_launch_equals_row_launch_and_itself(I, population):
    case = device_case(I, POPULATIONS[population])
    for irt in (1, 2):
        for A in DIMS:
            spec, table, item = problem(irt, A, I)
            for noise in NOISE:
                rows_image_image(spec, _lib.REG_KL, case, I, table, item, noise)


@pytest.mark.parametrize('form', ['REG_SAMPLED', 'drop_missing'])
@pytest.mark.parametrize('population', ['1|2', '2|3'])
def test_sampled_regulariser_and_dropped_missing_cells(population, form):
    """The other values of the constants in the chains' scalar mask, on either register set at the tail."""
    I = 1000
    # (a person without a single answer has no posterior once the missing cells' prior experts are dropped: those launches start at row 1)
    case = device_case(I, POPULATIONS[population], 1 if form == 'drop_missing' else 0)
    reg_mode = _lib.REG_SAMPLED if form == 'REG_SAMPLED' else _lib.REG_KL
    for irt in (1, 2):
        for A in (2, 7):
            _, table, item = problem(irt, A, I)
            spec = ops.ElboSpec(irt_model=irt, ability_dim=A, drop_missing=form == 'drop_missing')
            # (the folded step, which draws, takes the KL regulariser alone)
            for noise in ('given',) if form == 'REG_SAMPLED' else ('given', 'drawn, no outputs'):
                ref = rows_image_image(spec, reg_mode, case, I, table, item, noise)
                # (the constants do reach the kernel: the launch differs from the plain one)
                plain = launch(ops.ElboSpec(irt_model=irt, ability_dim=A), _lib.REG_KL, *case[:3], table, item, noise, True)
                assert not torch.equal(plain.flat, ref.flat)


@pytest.mark.parametrize('irt,A,noise', [(2, 8, 'drawn, no outputs'), (1, 2, 'given')])
def test_captured_step_replays_as_eager(irt, A, noise):
    """The folded step on the image, captured once and replayed three times, against three eager calls: the same bits call by call."""
    I = 1000
    r, m, image, n_obs = device_case(I, POPULATIONS['2|3'])
    P = r.shape[0]
    spec, table, item = problem(irt, A, I)
    eps = torch.randn(P, A, generator=torch.Generator().manual_seed(P)).to(dev()) if noise == 'given' else None

    def new_tick():
        return torch.tensor([0, 7], dtype=torch.int32, device=dev())

    def step(tick):
        call = (tick, False) if noise == 'given' else (tick, False, (SEED, STREAM), True)
        return ops._hip_launch_elbo(spec, r, m, _lib.MASK_U8, None, table, item, eps, None, _lib.REG_KL, True, P, train_step=call)
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
    assert not torch.isnan(eager[0]).any() and float(eager[0][_lib.S_KL]) != 0.0
    for k, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, b), (k, float((a - b).abs().max()))


@pytest.mark.parametrize('irt,want_grad', [(3, True), (2, False), (1, False)], ids=['3pl', '2pl forward only', '1pl forward only'])
def test_launches_without_chain_waves_keep_their_bits(irt, want_grad):
    """3PL and forward-only launches at 8 tile waves run the form without chain waves (ms_chain_waves): the rows' bits, as before."""
    I = 1000
    case = device_case(I, POPULATIONS['2|3'])
    for A in (1, 8):
        spec, table, item = problem(irt, A, I)
        for noise in ('given',) if not want_grad else ('given', 'drawn, no outputs'):
            rows_image_image(spec, _lib.REG_KL, case, I, table, item, noise, want_grad)
