"""Sign-as-mask fp32 rows on the GPU (VIBO_MASK_SIGN, include/vibo_hip_sign_rows.h): the matrix row-split kernel's mode that reads
no mask bytes, the verifier that says when a (response, mask) pair may use it, and a trainer end to end.

The reference of every kernel comparison is the same library's VIBO_MASK_U8 call on the same rows with mask = [sign bit clear] --
the path the fp64 oracle and the cell-by-cell suites already hold.  The two calls form identical code words by construction, so
every output is compared with torch.equal."""
import pytest
import torch

from gpu_common import assert_same_parameters, dev, twin_trainers
from vibo_amd import _lib, ops
from vibo_amd.torch_core.models import VIBO_2PL

pytestmark = pytest.mark.gpu
SEED, STREAM = 0x51_6E_00_01, 3
NEG_NAN = torch.tensor([-4194304], dtype=torch.int32).view(torch.float32)[0]          # 0xFFC00000


def rows(P, I, missing=-1.0, pad=None, seed=5, full_row=True):
    """Device (response, u8 mask) of P x I cells: 10 % missing, row 0 all missing, one item column all missing, and with full_row
    row 1 all observed (that column included); `missing` is what the response holds at missing cells.  pad: the row stride is
    padded to a multiple of 4 and the padding cells hold this value (their mask bytes 1: only the kernel's tail mask keeps them
    out)."""
    g = torch.Generator().manual_seed(seed + 1000 * P + I)
    mask = torch.rand(P, I, generator=g) >= 0.1
    mask[0] = False
    mask[:, 2 % I] = False
    if full_row:
        mask[1] = True
    answers = (torch.rand(P, I, generator=g) < 0.5).float()
    resp = torch.where(mask, answers, torch.as_tensor(missing))
    assert torch.equal(mask, ~torch.signbit(resp))
    if pad is None:
        return resp.to(dev()), mask.to(torch.uint8).to(dev())
    I4 = (I + 3) & ~3
    full_r, full_m = torch.full((P, I4), float(pad)), torch.ones(P, I4, dtype=torch.uint8)
    full_r[:, :I], full_m[:, :I] = resp, mask.to(torch.uint8)
    return full_r.to(dev())[:, :I], full_m.to(dev())[:, :I]


def problem(irt, A, I, seed=9):
    g = torch.Generator().manual_seed(seed)
    D = {1: 1, 2: A + 1, 3: A + 2}[irt]
    return (ops.ElboSpec(irt_model=irt, ability_dim=A), (torch.randn(2, 2 * A, generator=g) * 0.7).to(dev()),
            torch.randn(I, D, generator=g).to(dev()))


def both(spec, r, m, table, item, want_grad=True, draw=False):
    """-> (the VIBO_MASK_U8 call on (r, m), the VIBO_MASK_SIGN call on r alone), matrix kernel pinned; draw: the folded step that
    draws its own noise and is handed no ability outputs, else given noise."""
    P, A = r.shape[0], spec.ability_dim
    eps = None if draw else torch.randn(P, A, generator=torch.Generator().manual_seed(P)).to(dev())
    out = []
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        assert ops.plan_kernel(spec, P, r.shape[1], _lib.MASK_SIGN, want_grad).startswith('matrix')
        for mask, code in ((m, _lib.MASK_U8), (None, _lib.MASK_SIGN)):
            step = (torch.tensor([0, 7], dtype=torch.int32, device=dev()), False, (SEED, STREAM), True) if draw else None
            out.append(ops._hip_launch_elbo(spec, r, mask, code, None, table, item, eps, None, _lib.REG_KL, want_grad, P, train_step=step))
    torch.cuda.synchronize()
    return out


def assert_same_outputs(ref, got, r, m, want_grad=True, draw=False):
    n_obs = int((m != 0).sum())
    assert int(ref.scalars[_lib.S_NOBS]) == n_obs == int(got.scalars[_lib.S_NOBS])          # (rows past the end, padding cells: not counted)
    flat_ref, flat_got = (ref.flat, got.flat) if want_grad else (ref.scalars, got.scalars)
    assert not torch.isnan(flat_ref).any()
    assert torch.equal(flat_ref, flat_got), float((flat_ref - flat_got).abs().max())
    if draw:
        assert got.ability_mu is None and got._ability is None
        return
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        assert torch.equal(getattr(ref, k), getattr(got, k)), k
    if want_grad:
        assert torch.equal(ref.grad_table(0), got.grad_table(0)) and torch.equal(ref.grad_item(tuple(r.shape[1:]) + (-1,)), got.grad_item(tuple(r.shape[1:]) + (-1,)))


@pytest.fixture(autouse=True)
def explicit_formats(monkeypatch):
    """The kernel tests name their row format themselves; the deciding function stays out of them (the end-to-end test switches it)."""
    monkeypatch.setattr(ops, 'SIGN_ROWS', False)


# items: 1000 = 8 waves, last chunk of the row short of the wave's span; 1024 full; 997 in a stride of 1000: the tail mask, padding
# cells +1.0 / -1.0; 132 = 2 waves (the non-NW8 instantiation); 4.  persons: 31 < one batch; 32; 229 = 7 batches + 5 rows (rows past
# the end of the matrix in the last batch read as zeros: observed wrong answers unless the pack masks them).
ITEMS = [(1000, None), (1024, None), (997, 1.0), (997, -1.0), (132, None), (4, None)]


@pytest.mark.parametrize('P', [31, 32, 32 * 7 + 5])
@pytest.mark.parametrize('I,pad', ITEMS)
def test_items_by_persons(I, pad, P):
    r, m = rows(P, I, pad=pad)
    spec, table, item = problem(2, 8, I)
    ref, got = both(spec, r, m, table, item)
    assert_same_outputs(ref, got, r, m)


def test_more_than_one_batch_per_workgroup():
    """16 389 x 1000: 512 batches + 5 rows on at most 256 workgroups -- the double-buffered prefetch, its parity and the late start."""
    r, m = rows(16389, 1000)
    for draw in (False, True):
        spec, table, item = problem(2, 8, 1000)
        ref, got = both(spec, r, m, table, item, draw=draw)
        assert_same_outputs(ref, got, r, m, draw=draw)


@pytest.mark.parametrize('A', [1, 8])
@pytest.mark.parametrize('want_grad', [True, False])
@pytest.mark.parametrize('irt', [1, 2, 3])
def test_models_and_modes(irt, want_grad, A):
    r, m = rows(229, 1000)
    spec, table, item = problem(irt, A, 1000)
    ref, got = both(spec, r, m, table, item, want_grad=want_grad)
    assert_same_outputs(ref, got, r, m, want_grad=want_grad)
    if want_grad:                                   # the drawing step (eps NULL, NULL ability outputs) exists with gradients only
        ref, got = both(spec, r, m, table, item, draw=True)
        assert_same_outputs(ref, got, r, m, draw=True)


@pytest.mark.parametrize('missing', [-1.0, -0.0, -3.5, 'negative NaN'])
def test_what_a_missing_cell_holds(missing):
    r, m = rows(229, 1000, missing=NEG_NAN if missing == 'negative NaN' else missing, full_row=False)
    assert not m[:, 2].any() and not m[0].any()
    spec, table, item = problem(2, 8, 1000)
    ref, got = both(spec, r, m, table, item)
    assert_same_outputs(ref, got, r, m)


def test_gathered_rows_and_unaligned_rows_are_refused():
    r, m = rows(229, 1000)
    spec, table, item = problem(2, 8, 1000)
    eps = torch.zeros(229, 8, device=dev())
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        with pytest.raises(_lib.ViboLibraryError, match='row_index'):
            ops._hip_launch_elbo(spec, r, None, _lib.MASK_SIGN, torch.arange(229, device=dev()), table, item, eps, None, _lib.REG_KL, True, 229)
        shifted = torch.empty(229 * 1000 + 1, device=dev())[1:].view(229, 1000)          # rows that are not 16-byte aligned
        with pytest.raises(_lib.ViboLibraryError, match='aligned'):
            ops._hip_launch_elbo(spec, shifted, None, _lib.MASK_SIGN, None, table, item, eps, None, _lib.REG_KL, True, 229)
    torch.cuda.synchronize()


@pytest.mark.parametrize('layout', ['base off by 4 bytes', 'stride 1004, base off by 4 bytes', 'stride 1002'])
def test_rows_the_matrix_kernel_cannot_load_stay_on_the_mask_path(monkeypatch, layout):
    """A resident fp32 matrix whose rows the 16-byte loads cannot take (the planner names the matrix kernel, the launch falls back):
    with ops.SIGN_ROWS on, five calls on the same tensors all go out with the mask and return the bits of the call with it off."""
    P, I = 229, 1000
    r0, m = rows(P, I)
    if layout == 'base off by 4 bytes':
        r = torch.empty(P * I + 1, device=dev())[1:].view(P, I)
    elif layout == 'stride 1004, base off by 4 bytes':
        r = torch.empty(P, 1004, device=dev())[:, 1:1001]
    else:
        r = torch.empty(P, 1002, device=dev())[:, :1000]
    r.copy_(r0)
    assert r.data_ptr() % 16 != 0 or r.stride(0) % 4 != 0
    spec, table, item = problem(2, 8, I)
    eps = torch.randn(P, 8, generator=torch.Generator().manual_seed(P)).to(dev())
    codes, real_call = [], ops._call

    def logging_call(name, *args):
        if name.startswith('vibo_elbo_fwd_bwd'):
            codes.append(args[0]._obj.mask_dtype)
        return real_call(name, *args)
    monkeypatch.setattr(ops, '_call', logging_call)
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        ref = ops._hip_launch_elbo(spec, r, m, _lib.MASK_U8, None, table, item, eps, None, _lib.REG_KL, True, P)
        monkeypatch.setattr(ops, 'SIGN_ROWS', True)
        for _ in range(5):
            got = ops._hip_launch_elbo(spec, r, m, _lib.MASK_U8, None, table, item, eps, None, _lib.REG_KL, True, P)
            assert torch.equal(ref.flat, got.flat) and torch.equal(ref.ability, got.ability)
    torch.cuda.synchronize()
    assert codes == [_lib.MASK_U8] * 6 and not hasattr(r, '_vibo_row_counts')


# ---------------------------------------------------------------------------
# the verifier
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('padded', [False, True], ids=['stride 997', 'stride 1000'])
def test_verifier(padded):
    """229 x 997, rows as they come (one cell per thread) and in a stride of 1000 (4 cells per thread).  0 on consistent data; 1 for a
    single +1.0 under a mask 0, a single -1.0 or -0.0 under a mask 1 -- each alone, in the first row, the last row and the last cell
    of a row; 0 when the only inconsistencies sit in the row padding."""
    P, I = 229, 997
    r, m = rows(P, I, pad=-1.0 if padded else None)
    m[1, 2] = 0                                     # (row 1 is all observed: make room for a mask 0 in every row used below)
    r[1, 2] = -1.0
    assert ops._hip_sign_is_mask(r, m)
    if padded:
        base_r, base_m = r._base if r._base is not None else r, m._base if m._base is not None else m
        base_r[:, I:], base_m[:, I:] = 1.0, 0       # padding: an observed-looking value under a mask 0, in every row
        assert ops._hip_sign_is_mask(r, m)
        base_r[:, I:], base_m[:, I:] = -1.0, 1
        assert ops._hip_sign_is_mask(r, m)
    # ... and for a mask byte above 1 over an observed answer (the matrix kernel reads mask bytes as 0 / 1: only those give the
    # code words of the sign format)
    for row, col in ((0, 5), (P - 1, 5), (0, I - 1), (P - 1, I - 1), (100, I - 1)):
        for value, bit in ((1.0, 0), (-1.0, 1), (-0.0, 1), (1.0, 2), (0.0, 255)):
            keep_r, keep_m = r[row, col].clone(), m[row, col].clone()
            r[row, col], m[row, col] = value, bit
            assert not ops._hip_sign_is_mask(r, m), (row, col, value, bit)
            r[row, col], m[row, col] = keep_r, keep_m
            assert ops._hip_sign_is_mask(r, m)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _five_steps(sign_rows, graph):
    """-> (losses, model, mask codes of the ELBO launches in the order they were issued)."""
    P, I, A = 4133, 1000, 8
    r, m = rows(P, I, seed=21)
    m = m.bool()
    codes = []
    real_call = ops._call

    def logging_call(name, *args):
        if name.startswith('vibo_elbo_fwd_bwd'):
            codes.append(args[0]._obj.mask_dtype)
        return real_call(name, *args)
    with pytest.MonkeyPatch.context() as mp, ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        mp.setattr(ops, 'SIGN_ROWS', sign_rows)
        mp.setattr(ops, '_call', logging_call)
        model, _, trainer, _ = twin_trainers(VIBO_2PL, A, I, 7, dict(rng='native', seed=3))
        losses = []
        if not graph:
            for _ in range(5):
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
        torch.cuda.synchronize()
    return losses, model, codes


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'hipGraph'])
def test_trainer_end_to_end(graph):
    """FusedTrainer on a resident 4 133 x 1000 matrix: five steps with ops.SIGN_ROWS against five without, from the same seed -- the
    loss of every step and every parameter after the last are the same bits; the first two launches carry the mask (sighting,
    verification), every later one goes out as VIBO_MASK_SIGN (under capture: the folded step uses the verified fact)."""
    off_losses, off_model, off_codes = _five_steps(False, graph)
    on_losses, on_model, on_codes = _five_steps(True, graph)
    assert set(off_codes) == {_lib.MASK_U8}
    assert on_codes == [_lib.MASK_U8, _lib.MASK_U8] + [_lib.MASK_SIGN] * (1 if graph else 3), on_codes
    for k, (a, b) in enumerate(zip(off_losses, on_losses)):
        assert torch.equal(a, b), (k, float(a), float(b))
    assert len(on_losses) == 5
    assert_same_parameters(off_model, on_model)
