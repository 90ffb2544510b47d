"""Tile rows under a caller-supplied posterior on the GPU (include/vibo_hip_given_tiles.h: VIBO_MASK_TILES with VIBO_POSTERIOR_GIVEN):
the matrix row-split kernel on a matrix' image against the same library's VIBO_POSTERIOR_GIVEN launch on the source rows,
torch.equal on every output, at every workgroup width the kernel takes another path at; and the three trainers whose ELBO launch
runs in that mode -- FusedMeanTrainer, FusedVITrainer, FusedMLETrainer -- end to end, eager and replayed from a hipGraph.

The reference of every comparison is the launch on the rows the image was built from: the path the fp64 oracle and the existing
suites already hold.  The image carries the code words and counts that launch forms itself, and the posterior comes from memory
either way, so every output has the same bits.

S_NOBS: in VIBO_POSTERIOR_GIVEN mode every cell counts as observed (include/vibo_hip.h: NOBS = num_person x num_item, no
missing-prior expert), on rows and on the image alike; it is held to that product exactly -- rows past the end of the last batch
and padding cells are counted nowhere."""
import functools

import pytest
import torch

from gpu_common import assert_same_parameters, dev
from tile_rows_gpu_common import build, device_rows, grid_of, host_rows
from vibo_amd import _lib, ops
from vibo_amd.torch_core import models as M
from vibo_amd.trainer import FusedMeanTrainer, FusedMLETrainer, FusedTrainer, FusedVITrainer

pytestmark = pytest.mark.gpu
ENTRY = 'vibo_elbo_fwd_bwd_given_tiles'


# ---------------------------------------------------------------------------
# the kernel on the image against the kernel on the source rows
# ---------------------------------------------------------------------------
def problem(irt, A, P, I, seed=9):
    """-> (spec, posterior [P, 2A] = (mu ~ 0.7 N(0, 1) | logvar ~ 0.5 N(0, 1)), item sample, noise), seeded."""
    g = torch.Generator().manual_seed(seed + 1000 * A + irt)
    D = {1: 1, 2: A + 1, 3: A + 2}[irt]
    post = torch.cat([0.7 * torch.randn(P, A, generator=g), 0.5 * torch.randn(P, A, generator=g)], dim=1)
    item = torch.randn(I, D, generator=g)
    eps = torch.randn(P, A, generator=g)
    return ops.ElboSpec(irt_model=irt, ability_dim=A, given=True), post.to(dev()), item.to(dev()), eps.to(dev())


def both(spec, r, m, code, image, post, item, eps, want_grad=True):
    """-> (the launch on the source rows, the launch on their image), matrix kernel pinned, each as a trainer's resident step.
    The image goes out through the resident-matrix record, as in use."""
    P = r.shape[0]
    sent, real_call, out = [], ops._call, []

    def logging_call(name, *args):
        if name.startswith('vibo_elbo_fwd_bwd'):
            sent.append((name, args[0]._obj.mask_dtype))
        return real_call(name, *args)
    with pytest.MonkeyPatch.context() as mp, ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        mp.setattr(ops, '_call', logging_call)
        mp.setattr(ops, 'SIGN_ROWS', False)
        mp.setattr(ops, 'TILE_ROWS', True)
        mp.setattr(ops, 'TILE_ROWS_MIN_PERSONS', 1)
        mp.setattr(ops, 'TILE_ROWS_GIVEN_MIN_PERSONS', 0)
        for tiles in (False, True):
            mp.setattr(ops, 'TILE_ROWS_GIVEN', tiles)
            rec = ops.ResidentMatrix(r, None if code == _lib.MASK_CODES else m)
            rec.tiles = image
            r._vibo_row_counts = rec
            out.append(ops._hip_launch_elbo(spec, r, m, code, None, post, item, eps, None, _lib.REG_KL, want_grad, P, resident_step=True))
        del r._vibo_row_counts
    torch.cuda.synchronize()
    assert sent == [('vibo_elbo_fwd_bwd', code), (ENTRY, _lib.MASK_TILES)], sent
    return out


def assert_same_outputs(ref, got, P, I, A, want_grad=True):
    assert int(ref.scalars[_lib.S_NOBS]) == P * I == int(got.scalars[_lib.S_NOBS])            # (see the module's docstring)
    flat_ref, flat_got = (ref.flat, got.flat) if want_grad else (ref.scalars, got.scalars)
    if want_grad:                # scalars | both gradient sets 2 x P x 2A | item gradient
        assert flat_ref.numel() == _lib.NUM_SCALARS + 2 * P * 2 * A + ref.n_item and ref.n_table == P * 2 * A
    assert not torch.isnan(flat_ref).any() and not torch.isnan(flat_got).any()
    assert torch.equal(flat_ref, flat_got), float((flat_ref - flat_got).abs().max())
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        assert not torch.isnan(getattr(ref, k)).any(), k
        assert torch.equal(getattr(ref, k), getattr(got, k)), k


def assert_same_launch(a, b, want_grad):
    """The second launch of a pair against the first: the same bits."""
    for x, y in zip(a, b):
        assert torch.equal(x.flat if want_grad else x.scalars, y.flat if want_grad else y.scalars)
        for k in ('ability_mu', 'ability_logvar', 'ability'):
            assert torch.equal(getattr(x, k), getattr(y, k)), k


# one batch with tail rows | per width: 32 (2 G + 40) + 7 rows -- some workgroups run three batches and the rest two, both parities
# occur at the tail, the last batch is partial.  1000 / 897 items: 8 waves on the two-barrier loop (which no other instantiation
# runs on an image); 896: 7 waves; 512: 4, the narrowest workgroup that takes the posterior a batch ahead; 384: 3, 130: 2 -- the
# branch that loads posterior and noise between the barriers (130: four workgroups per compute unit)
KERNEL_SHAPES = [('one batch', 1000), ('loop', 1000), ('loop', 897), ('loop', 896), ('loop', 512), ('loop', 384), ('loop', 130)]


@pytest.mark.parametrize('kind,I', KERNEL_SHAPES)
def test_kernel_on_the_image_equals_the_kernel_on_the_rows(kind, I):
    P = 229 if kind == 'one batch' else 32 * (2 * grid_of(I) + 40) + 7
    r, m, image = device_rows(P, I)
    for irt in (1, 2, 3):
        for A in (1, 3, 8):
            spec, post, item, eps = problem(irt, A, P, I)
            for want_grad in (False, True):
                first = both(spec, r, m, _lib.MASK_U8, image, post, item, eps, want_grad=want_grad)
                assert_same_outputs(*first, P, I, A, want_grad=want_grad)
                again = both(spec, r, m, _lib.MASK_U8, image, post, item, eps, want_grad=want_grad)
                assert_same_launch(first, again, want_grad)


@pytest.mark.parametrize('source', ['fp32, no mask', 'cell codes'])
def test_kernel_on_images_of_the_other_sources(source):
    P, I, A = 32 * 9 + 5, 1000, 8
    resp, mask = host_rows(P, I, seed=13)
    spec, post, item, eps = problem(2, A, P, I)
    if source == 'fp32, no mask':
        r, m, code = (resp == 1.0).float().to(dev()), None, _lib.MASK_NONE
    else:
        codes = torch.where(mask, (resp == 1.0).to(torch.uint8), torch.tensor(2, dtype=torch.uint8)).to(dev())
        r, m, code = codes, codes, _lib.MASK_CODES
    image = build(r, m, code, P)
    ref, got = both(spec, r, m, code, image, post, item, eps)
    assert_same_outputs(ref, got, P, I, A)


# ---------------------------------------------------------------------------
# the trainers end to end
# ---------------------------------------------------------------------------
P_E2E, I_E2E, A_E2E = 17671, 1000, 8


@functools.lru_cache(maxsize=1)
def e2e_rows():
    """Host (response with -1 under the mask, bool mask) of the end-to-end matrix, drawn once and never written.  (host_rows' row
    without a single answer takes a neighbour's cells: the mean merge of no answers is 0 / 0 in the reference as well, and a loss
    of NaN would compare nothing.)"""
    resp, mask = host_rows(P_E2E, I_E2E, seed=21)
    resp[0], mask[0] = resp[5], mask[5]
    assert bool(mask.any(dim=1).all())
    return torch.where(mask, resp, torch.tensor(-1.0)), mask


def make_trainer(kind):
    torch.manual_seed(7)
    if kind == 'mean':
        model = M.VIBO_2PL(A_E2E, I_E2E, ability_merge='mean').to(dev())
    elif kind == 'vi':
        model = M.VI_2PL(A_E2E, P_E2E, I_E2E).to(dev())
    else:
        model = M.MLE_2PL(A_E2E, P_E2E, I_E2E).to(dev())
    trainer = FusedTrainer(model, lr=5e-3, rng='native', seed=3)
    assert type(trainer) is {'mean': FusedMeanTrainer, 'vi': FusedVITrainer, 'mle': FusedMLETrainer}[kind]
    return model, trainer


def _steps(kind, given_tiles, graph, edit=False, row_index=False, min_persons=None):
    """-> (losses, model, trainer, the ELBO entry points in the order they were issued)."""
    resp, mask = e2e_rows()
    r, m = resp.to(dev()), mask.to(dev())
    rows = torch.randperm(P_E2E, generator=torch.Generator().manual_seed(5))[:4096].to(dev()) if row_index else None
    names = []
    real_call = ops._call

    def logging_call(name, *args):
        if name.startswith('vibo_elbo_fwd_bwd'):
            names.append(name)
            assert (args[0]._obj.mask_dtype == _lib.MASK_TILES) == (name == ENTRY)
        return real_call(name, *args)
    with pytest.MonkeyPatch.context() as mp, ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        mp.setattr(ops, 'TILE_ROWS', True)
        mp.setattr(ops, 'TILE_ROWS_GIVEN', given_tiles)
        mp.setattr(ops, 'TILE_ROWS_GIVEN_MIN_PERSONS', 0)
        mp.setattr(ops, 'TILE_ROWS_PLAIN_LAUNCHES', False)
        mp.setattr(ops, 'SIGN_ROWS', False)
        mp.setattr(ops, '_call', logging_call)
        if min_persons is not None:
            mp.setattr(ops, 'TILE_ROWS_MIN_PERSONS', min_persons)
        model, trainer = make_trainer(kind)
        losses = []
        if not graph:
            for k in range(8 if edit else 5):
                if edit and k == 4:
                    r[0, 0] = 1.0 - r[0, 0].clamp(0.0, 1.0)          # an in-place edit: back to the source rows, a new image
                    m[0, 0] = True
                losses.append(trainer.step(r, m, row_index=rows).clone())
        else:
            for _ in range(2):
                losses.append(trainer.step(r, m, row_index=rows).clone())
            torch.cuda.synchronize()
            g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    loss = trainer.step(r, m, row_index=rows)
            torch.cuda.current_stream().wait_stream(side)
            for _ in range(3):
                g.replay()
                losses.append(loss.clone())
        torch.cuda.synchronize()
    return losses, model, trainer, names


def assert_same_training(off, on, kind):
    (off_losses, off_model, off_trainer, _), (on_losses, on_model, on_trainer, _) = off, on
    assert len(on_losses) == len(off_losses) >= 5
    for k, (a, b) in enumerate(zip(off_losses, on_losses)):
        assert not torch.isnan(a).any()
        assert torch.equal(a, b), (k, float(a), float(b))
    assert_same_parameters(off_model, on_model)                   # (VI / MLE: the person tables are parameters of the model)
    for name in ('item_m', 'item_v') + (('person_m', 'person_v') if kind != 'mean' else ('par_m', 'par_v')):
        assert torch.equal(getattr(off_trainer, name), getattr(on_trainer, name)), name


# The launch sequences as observed.  The mean trainer's ops.row_counts creates the matrix' record in front of its first ELBO launch, so
# that launch is already the second sighting: it builds and still reads the rows, the second step goes out on the image.  VI / MLE: first
# sighting, build, image.
ROWS = 'vibo_elbo_fwd_bwd'
EAGER = {'mean': [ROWS] + [ENTRY] * 4, 'vi': [ROWS, ROWS] + [ENTRY] * 3, 'mle': [ROWS, ROWS] + [ENTRY] * 3}


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'hipGraph'])
@pytest.mark.parametrize('kind', ['mean', 'vi', 'mle'])
def test_trainers_end_to_end(kind, graph):
    """17 671 x 1000, ability_dim 8, 2PL, rng='native', the same seed: five steps with ops.TILE_ROWS_GIVEN on against five with it off
    -- every step's loss, every parameter and every Adam moment after the last step are the same bits.  The ELBO launches start on the
    rows and end on the image; under capture (two eager steps, capture, three replays) the captured step uses the image."""
    off = _steps(kind, False, graph)
    on = _steps(kind, True, graph)
    assert set(off[3]) == {ROWS} and len(off[3]) == (3 if graph else 5)
    assert on[3] == (EAGER[kind][:2] + [ENTRY] if graph else EAGER[kind]), on[3]
    assert_same_training(off, on, kind)


def test_a_row_index_minibatch_never_leaves_the_rows():
    _, _, _, names = _steps('mean', True, False, row_index=True)
    assert names == [ROWS] * 5, names
    _, _, _, names = _steps('vi', True, True, row_index=True)
    assert names == [ROWS] * 3, names


def test_below_the_threshold_never_leaves_the_rows():
    _, _, _, names = _steps('mean', True, False, min_persons=P_E2E + 1)
    assert names == [ROWS] * 5, names
    _, _, _, names = _steps('mle', True, True, min_persons=P_E2E + 1)
    assert names == [ROWS] * 3, names


def test_an_in_place_edit_returns_the_mean_trainer_to_the_source_rows_and_rebuilds():
    off = _steps('mean', False, False, edit=True)
    on = _steps('mean', True, False, edit=True)
    # (the edit throws the record away; row_counts makes the new one, the launch behind it builds and reads the rows)
    assert on[3] == [ROWS, ENTRY, ENTRY, ENTRY, ROWS, ENTRY, ENTRY, ENTRY], on[3]
    assert set(off[3]) == {ROWS}
    assert_same_training(off, on, 'mean')
