"""What the GPU tests of the tile rows (VIBO_MASK_TILES) share, once each: the host rows with everything a mask can hide under it, their
strided device copies, the builder's call, the matrix kernel's grid, one problem, and the launch on the source rows beside the launch
on their image with the comparison of every output.  A plain module, importable without a GPU: only calling into it needs one."""
import functools

import pytest
import torch

import tile_rows_common as T
from gpu_common import dev
from vibo_amd import _lib, ops

SEED, STREAM = 0x71_1E_00_01, 3
UNDER_THE_MASK = [-1.0, 0.0, 1.0, 7.5, float('nan')]


def host_rows(P, I, seed=3):
    """Host (response fp32, mask bool): 15 % missing with -1 / 0.0 / 1.0 / 7.5 / NaN under the masked cells, row 0 all missing, row 1
    all observed, one item column all missing (where the shape has room for them)."""
    g = torch.Generator().manual_seed(seed + 1000 * P + I)
    mask = torch.rand(P, I, generator=g) >= 0.15
    if P > 2:
        mask[:, 2 % I] = False
        mask[0], mask[1] = False, True
    answers = (torch.rand(P, I, generator=g) < 0.5).float()
    junk = torch.tensor(UNDER_THE_MASK)[torch.randint(0, len(UNDER_THE_MASK), (P, I), generator=g)]
    return torch.where(mask, answers, junk), mask


def strided(t, stride, fill):
    """A device copy of the [P, I] tensor whose rows lie `stride` cells apart, the padding cells holding `fill`."""
    full = torch.full((t.shape[0], stride), fill, dtype=t.dtype)
    full[:, :t.shape[1]] = t
    return full.to(dev())[:, :t.shape[1]]


def build(r, m, code, P):
    """vibo_tile_rows_build of the device rows (r, m) read as mask format `code` -> the image (device uint8)."""
    spec = ops.ElboSpec(irt_model=2, ability_dim=8)
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        nbytes = ops._hip_tile_rows_bytes(ops._tile_desc(spec, P, r.shape[1], _lib.REG_KL, True))
        assert nbytes == T.image_bytes(P, r.shape[1])
        return ops._hip_tile_rows_build(spec, r, m, code, P, _lib.REG_KL, True, nbytes)


def grid_of(I):
    """Workgroups of the matrix kernel's launch at I items on this device (vibo_planner.hip, msplit_blocks)."""
    nw = (I + 127) // 128
    return torch.cuda.get_device_properties(dev()).multi_processor_count * max(1, 8 // nw)


@functools.lru_cache(maxsize=2)
def device_rows(P, I):
    """(response, u8 mask, image) on the device, built once per shape and never written."""
    resp, mask = host_rows(P, I, seed=11)
    # (rows in whole 4-cell chunks, as ops.pad_rows leaves them: the launch on the source rows runs the matrix kernel too)
    r, m = strided(resp, (I + 3) & ~3, 1.0), strided(mask.to(torch.uint8), (I + 3) & ~3, 1)
    return r, m, build(r, m, _lib.MASK_U8, P)


def problem(irt, A, I, seed=9):
    g = torch.Generator().manual_seed(seed)
    D = {1: 1, 2: A + 1, 3: A + 2}[irt]
    return (ops.ElboSpec(irt_model=irt, ability_dim=A), (torch.randn(2, 2 * A, generator=g) * 0.7).to(dev()),
            torch.randn(I, D, generator=g).to(dev()))


def both(spec, r, m, code, image, table, item, want_grad=True, draw=False):
    """-> (the launch on the source rows, the launch on their image), matrix kernel pinned; draw: the folded step that draws its own
    noise and is handed no ability outputs, else given noise.  The image goes out through the resident-matrix record, as in use."""
    P, A = r.shape[0], spec.ability_dim
    eps = None if draw else torch.randn(P, A, generator=torch.Generator().manual_seed(P)).to(dev())
    sent, real_call, out = [], ops._call, []

    def logging_call(name, *args):
        if name.startswith('vibo_elbo_fwd_bwd'):
            sent.append(args[0]._obj.mask_dtype)
        return real_call(name, *args)
    with pytest.MonkeyPatch.context() as mp, ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        mp.setattr(ops, '_call', logging_call)
        mp.setattr(ops, 'SIGN_ROWS', False)
        mp.setattr(ops, 'TILE_ROWS_MIN_PERSONS', 1)
        mp.setattr(ops, 'TILE_ROWS_PLAIN_LAUNCHES', True)
        for tiles in (False, True):
            mp.setattr(ops, 'TILE_ROWS', tiles)
            rec = ops.ResidentMatrix(r, None if code == _lib.MASK_CODES else m)
            rec.tiles = image
            r._vibo_row_counts = rec
            step = (torch.tensor([0, 7], dtype=torch.int32, device=dev()), False, (SEED, STREAM), True) if draw else None
            out.append(ops._hip_launch_elbo(spec, r, m, code, None, table, item, eps, None, _lib.REG_KL, want_grad, P, train_step=step))
        del r._vibo_row_counts
    torch.cuda.synchronize()
    assert sent == [code, _lib.MASK_TILES], sent
    return out


def assert_same_outputs(ref, got, n_obs, want_grad=True, draw=False):
    assert int(ref.scalars[_lib.S_NOBS]) == n_obs == int(got.scalars[_lib.S_NOBS])          # (rows past the end, padding cells: not counted)
    flat_ref, flat_got = (ref.flat, got.flat) if want_grad else (ref.scalars, got.scalars)
    assert not torch.isnan(flat_ref).any()
    assert torch.equal(flat_ref, flat_got), float((flat_ref - flat_got).abs().max())
    if draw:
        assert got.ability_mu is None and got._ability is None
        return
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        assert torch.equal(getattr(ref, k), getattr(got, k)), k
