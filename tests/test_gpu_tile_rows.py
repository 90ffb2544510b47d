"""Tile rows on the GPU (VIBO_MASK_TILES, include/vibo_hip_tile_rows.h): the builder of a matrix' image against the numpy model
of the header's layout (tile_rows_common.py), byte for byte; the matrix row-split kernel on the image against the same library's
launch on the source rows, torch.equal on every output; and a trainer end to end.

The reference of every kernel comparison is the launch on the rows the image was built from -- the path the fp64 oracle and the
cell-by-cell suites already hold.  The image carries the code words that launch forms itself, so every output has the same bits."""
import numpy as np
import pytest
import torch

import tile_rows_common as T
from gpu_common import assert_same_parameters, dev, twin_trainers
from tile_rows_gpu_common import assert_same_outputs, both, build, device_rows, grid_of, host_rows, problem, strided
from vibo_amd import _lib, ops
from vibo_amd.torch_core.models import VIBO_2PL

pytestmark = pytest.mark.gpu


# (P, I, row stride or None); 999 items in a stride of 1000: the tail mask, with padding cells that look observed and right
BUILD_SHAPES = [(1, 4, None), (33, 8, None), (95, 130, None), (64, 896, None), (97, 897, 900), (229, 1000, None), (64, 1024, 1040),
                (70, 999, 1000)]


@pytest.mark.parametrize('source', ['fp32 + mask', 'fp32, no mask', 'sign rows', 'cell codes'])
@pytest.mark.parametrize('P,I,stride', BUILD_SHAPES)
def test_builder_against_the_model(P, I, stride, source):
    resp, mask = host_rows(P, I)
    pad = I if stride is None else stride
    if source == 'fp32 + mask':
        obs, right = T.observed_and_right(resp.numpy(), mask.to(torch.uint8).numpy())
        image = build(strided(resp, pad, 1.0), strided(mask.to(torch.uint8), pad, 1), _lib.MASK_U8, P)
    elif source == 'fp32, no mask':
        obs, right = T.observed_and_right(resp.numpy(), None)
        image = build(strided(resp, pad, 1.0), None, _lib.MASK_NONE, P)
    elif source == 'sign rows':
        signed = torch.where(mask, resp, torch.copysign(resp.abs(), torch.tensor(-1.0)))       # -1, -0.0, -7.5, -NaN under the mask
        obs, right = T.observed_and_right(signed.numpy(), None, sign=True)
        assert np.array_equal(obs, mask.numpy())
        image = build(strided(signed, pad, 1.0), None, _lib.MASK_SIGN, P)
    else:
        codes = torch.where(mask, (resp == 1.0).to(torch.uint8), torch.tensor(2, dtype=torch.uint8))
        obs, right = T.observed_and_right(codes=codes.numpy())
        codes = strided(codes, pad, 1)
        image = build(codes, codes, _lib.MASK_CODES, P)
    want = T.build_image(obs, right)
    got = image.cpu().numpy()
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    # the model's own walk of the offset formula, cell by cell, at the corners and a few random cells
    g = np.random.default_rng(P * 7 + I)
    cells = [(0, 0), (P - 1, I - 1), (0, I - 1), (P - 1, 0)] + [(int(g.integers(P)), int(g.integers(I))) for _ in range(32)]
    for row, col in cells:
        expect = T.RIGHT if right[row, col] else T.WRONG if obs[row, col] else T.MISSING
        assert T.cell_byte(got, P, I, row, col) == expect, (row, col)


def test_builder_refusals():
    """Host-side refusals: nothing is launched."""
    r = torch.zeros(64, 1000, device=dev())
    spec = ops.ElboSpec(irt_model=2, ability_dim=8)
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        with pytest.raises(_lib.ViboLibraryError, match='too small'):
            ops._hip_tile_rows_build(spec, r, None, _lib.MASK_NONE, 64, _lib.REG_KL, True, 4096)
        with pytest.raises(_lib.ViboLibraryError, match='rc=-8'):
            ops._hip_tile_rows_build(spec, r, r.long(), _lib.MASK_I64, 64, _lib.REG_KL, True, T.image_bytes(64, 1000))
        with pytest.raises(_lib.ViboLibraryError, match='rc=-5'):
            ops._hip_tile_rows_build(spec, r, None, _lib.MASK_U8, 64, _lib.REG_KL, True, T.image_bytes(64, 1000))


# ---------------------------------------------------------------------------
# the kernel on the image against the kernel on the source rows
# ---------------------------------------------------------------------------
# one batch with tail rows | per width: 32 (2 G + 40) + 7 rows -- some workgroups run three batches and the rest two, the last batch
# is partial: the loop's look-ahead, its parity and the "one batch more" workgroups.  1000 / 897 items: 8 waves; 896: 7 (not NW8);
# 130: 2 waves, four workgroups per compute unit
KERNEL_SHAPES = [('one batch', 1000), ('loop', 1000), ('loop', 130), ('loop', 896), ('loop', 897)]


@pytest.mark.parametrize('kind,I', KERNEL_SHAPES)
def test_kernel_on_the_image_equals_the_kernel_on_the_rows(kind, I):
    P = 229 if kind == 'one batch' else 32 * (2 * grid_of(I) + 40) + 7
    r, m, image = device_rows(P, I)
    n_obs = int(m.sum())
    for irt in (1, 2, 3):
        for A in (1, 3, 8):
            spec, table, item = problem(irt, A, I)
            for want_grad in (False, True):
                ref, got = both(spec, r, m, _lib.MASK_U8, image, table, item, want_grad=want_grad)
                assert_same_outputs(ref, got, n_obs, want_grad=want_grad)
            ref, got = both(spec, r, m, _lib.MASK_U8, image, table, item, draw=True)      # (the drawing step exists with gradients only)
            assert_same_outputs(ref, got, n_obs, draw=True)


@pytest.mark.parametrize('source', ['fp32, no mask', 'cell codes'])
def test_kernel_on_images_of_the_other_sources(source):
    P, I = 32 * 9 + 5, 1000
    resp, mask = host_rows(P, I, seed=13)
    spec, table, item = problem(2, 8, I)
    if source == 'fp32, no mask':
        r, m, code, n_obs = (resp == 1.0).float().to(dev()), None, _lib.MASK_NONE, P * I
    else:
        codes = torch.where(mask, (resp == 1.0).to(torch.uint8), torch.tensor(2, dtype=torch.uint8)).to(dev())
        r, m, code, n_obs = codes, codes, _lib.MASK_CODES, int(mask.sum())
    image = build(r, m, code, P)
    for draw in (False, True):
        ref, got = both(spec, r, m, code, image, table, item, draw=draw)
        assert_same_outputs(ref, got, n_obs, draw=draw)


def test_a_misaligned_image_and_gathered_rows_are_refused():
    """Host-side refusals of the launch: nothing runs on them."""
    P, I = 229, 1000
    spec, table, item = problem(2, 8, I)
    eps = torch.zeros(P, 8, device=dev())
    image = torch.zeros(T.image_bytes(P, I) + 16, dtype=torch.uint8, device=dev())
    lib, vp = _lib.load(), ops._ptr
    ws = torch.empty(1 << 24, dtype=torch.uint8, device=dev())
    flat = torch.empty(8 + 64 + I * 9, device=dev())
    post = torch.empty(3, P, 8, device=dev())
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        d = ops._tile_desc(spec, P, I, _lib.REG_KL, True)

        def launch(img, row_index):
            return lib.vibo_elbo_fwd_bwd(d, vp(img), None, vp(row_index), vp(table), vp(item), vp(eps), None, vp(flat), vp(post[0]), vp(post[1]),
                                         vp(post[2]), None, None, vp(flat[8:]), vp(flat[72:]), None, vp(ws), ws.numel(), None)
        assert launch(image[4:], None) == -8 and b'aligned' in lib.vibo_last_error_string()
        assert launch(image, torch.arange(P, device=dev())) == -8 and b'row_index' in lib.vibo_last_error_string()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _steps(tile_rows, graph, edit=False, plain=False):
    """-> (losses, model, mask codes of the ELBO launches in the order they were issued, the last step's ability sample)."""
    P, I, A = 17671, 1000, 8
    resp, mask = host_rows(P, I, seed=21)
    r, m = torch.where(mask, resp, torch.tensor(-1.0)).to(dev()), mask.to(dev())
    codes = []
    real_call = ops._call

    def logging_call(name, *args):
        if name.startswith('vibo_elbo_fwd_bwd'):
            codes.append(args[0]._obj.mask_dtype)
        return real_call(name, *args)
    with pytest.MonkeyPatch.context() as mp, ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        mp.setattr(ops, 'TILE_ROWS', tile_rows)
        mp.setattr(ops, 'TILE_ROWS_PLAIN_LAUNCHES', plain)
        mp.setattr(ops, 'SIGN_ROWS', False)
        mp.setattr(ops, '_call', logging_call)
        model, _, trainer, _ = twin_trainers(VIBO_2PL, A, I, 7, dict(rng='native', seed=3))
        losses = []
        if not graph:
            for k in range(8 if edit else 5):
                if edit and k == 4:
                    r[0, 0] = 1.0 - r[0, 0].clamp(0.0, 1.0)          # an in-place edit: back to the source rows, a new image
                    m[0, 0] = True
                losses.append(trainer.step(r, m).clone())
        else:
            for _ in range(2):
                losses.append(trainer.step(r, m).clone())
            torch.cuda.synchronize()
            g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    loss = trainer.step(r, m)
            torch.cuda.current_stream().wait_stream(side)
            for _ in range(3):
                g.replay()
                losses.append(loss.clone())
        n_step_launches = len(codes)
        ability = trainer.last.ability.clone()                         # (rebuilt on demand: one more launch, on the same rows)
        torch.cuda.synchronize()
    return losses, model, codes[:n_step_launches], codes[n_step_launches:], ability


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'hipGraph'])
def test_trainer_end_to_end(graph):
    """FusedTrainer on a resident 17 671 x 1000 matrix: five steps with ops.TILE_ROWS against five without, from the same seed -- the
    loss of every step, every parameter after the last and the last step's ability sample are the same bits; the first two launches
    go out on the source rows (sighting, build), every later one as VIBO_MASK_TILES (under capture: the folded step uses the
    image).  The hipGraph case also switches ops.TILE_ROWS_PLAIN_LAUNCHES on: the rebuilt sample then comes from the image."""
    off_losses, off_model, off_codes, _, off_ability = _steps(False, graph)
    on_losses, on_model, on_codes, on_read, on_ability = _steps(True, graph, plain=graph)
    assert set(off_codes) == {_lib.MASK_U8}
    assert on_codes == [_lib.MASK_U8, _lib.MASK_U8] + [_lib.MASK_TILES] * (1 if graph else 3), on_codes
    # the sample's rebuild is a plain launch: on the rows by default, on the image with ops.TILE_ROWS_PLAIN_LAUNCHES -- the same bits
    assert on_read == [_lib.MASK_TILES if graph else _lib.MASK_U8]
    assert len(on_losses) == 5
    for k, (a, b) in enumerate(zip(off_losses, on_losses)):
        assert torch.equal(a, b), (k, float(a), float(b))
    assert_same_parameters(off_model, on_model)
    assert torch.equal(off_ability, on_ability)


def test_an_in_place_edit_returns_to_the_source_rows_and_rebuilds():
    off_losses, off_model, _, _, off_ability = _steps(False, False, edit=True)
    on_losses, on_model, on_codes, _, on_ability = _steps(True, False, edit=True)
    U8, TILES = _lib.MASK_U8, _lib.MASK_TILES
    assert on_codes == [U8, U8, TILES, TILES, U8, U8, TILES, TILES], on_codes
    for k, (a, b) in enumerate(zip(off_losses, on_losses)):
        assert torch.equal(a, b), (k, float(a), float(b))
    assert_same_parameters(off_model, on_model)
    assert torch.equal(off_ability, on_ability)
