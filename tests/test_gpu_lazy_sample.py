"""The folded train step that draws its own ability noise (matrix row-split kernel) stores no sample any more: the kernel is handed
ability = NULL, and `trainer.last.ability` rebuilds the sample when read -- the step's noise at its counter, then the plain ELBO call
on the step's rows with the expert table the step ran on, which vibo_train_epilogue_fused keeps behind the next one.  Held here bit
for bit against the four-launch form (fold=False), which stores the sample; also that nothing is stored, and how long the rebuild
stays valid."""
import ctypes

import pytest
import torch

from gpu_common import assert_same_parameters, coin_flip_rows, dev, simulated, twin_trainers
from vibo_amd import _lib, ops
from vibo_amd.torch_core.models import VIBO_2PL

pytestmark = pytest.mark.gpu
SEED = 3


def problem(B, I, A, mask_kind, seed=11):
    """Device rows of a resident [B, I] matrix, padded to 16-byte row strides (130 items) so that the folded step takes them.
    mask_kind: 'missing' (bool, 10 % missing), 'none' (mask=None, every cell answered), 'empty row' (10 % missing and one person
    who answered nothing)."""
    resp, mask, _ = simulated(2, B, I, A, 0.0 if mask_kind == 'none' else 0.1, seed)
    mask = mask.bool()
    if mask_kind == 'empty row':
        mask[B // 2] = False
        resp[B // 2] = -1.0
    resp, mask = ops.pad_rows(resp.to(dev()), None if mask_kind == 'none' else mask.to(dev()))
    return resp, mask


def twins(A, I, **kw):
    """(folded trainer that draws its noise, four-launch trainer that stores the sample), same model, seed and noise streams."""
    m1, m2, t1, t2 = twin_trainers(VIBO_2PL, A, I, 7, dict(rng='native', seed=SEED, **kw), dict(rng='native', seed=SEED, fold=False))
    return m1, m2, t1, t2


def same_step(t1, t2, m1, m2, what):
    assert t1._draw_mode and t1.last.ability_mu is None, what
    assert t1.last._ability is None and t1.last.ability_source is not None, what          # nothing stored, nothing rebuilt yet
    assert torch.equal(t1.last.ability, t2.last.ability), what
    assert torch.equal(t1.last.flat, t2.last.flat), what
    assert_same_parameters(m1, m2)


# B = 33: one full batch of 32 rows and a 1-row tail; 8 224 = 257 batches: with 256 workgroups exactly one runs a second batch.
# I = 1000: 8 waves per workgroup; 130: 3 waves.  The planner gives none of the short ones to the matrix kernel: pinned.
@pytest.mark.parametrize('mask_kind', ['missing', 'none', 'empty row'])
@pytest.mark.parametrize('A', [1, 8])
@pytest.mark.parametrize('I', [1000, 130])
@pytest.mark.parametrize('B', [33, 8224])
def test_rebuilt_sample_equals_the_stored_one(B, I, A, mask_kind):
    resp, mask = problem(B, I, A, mask_kind)
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        m1, m2, t1, t2 = twins(A, I)
        for k in range(3):
            la, lb = t1.step(resp, mask), t2.step(resp, mask)
            assert torch.equal(la, lb), k
            same_step(t1, t2, m1, m2, k)


@pytest.mark.parametrize('I', [1000, 130])
def test_rebuilt_sample_of_a_gathered_minibatch(I):
    """row_index: a permutation of 64 rows out of 200 -- the rebuild gathers the same rows in the same order.  At 130 items (fp32
    rows gathered at fewer than 8 waves: the library's one exception) the drawing step still stores its sample."""
    A = 8
    resp, mask = problem(200, I, A, 'missing')
    rows = torch.randperm(200, generator=torch.Generator().manual_seed(5))[:64].to(dev())
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        m1, m2, t1, t2 = twins(A, I)
        for k in range(3):
            assert torch.equal(t1.step(resp, mask, row_index=rows), t2.step(resp, mask, row_index=rows)), k
            if I == 1000:
                same_step(t1, t2, m1, m2, k)
            else:
                assert t1._draw_mode and t1.last.ability_source is None and t1.last._ability is not None
                assert torch.equal(t1.last.ability, t2.last.ability) and torch.equal(t1.last.flat, t2.last.flat)
        assert_same_parameters(m1, m2)
        if I == 130:            # ... and the library refuses the NULL there
            raw = ops._BACKEND['elbo']
            with pytest.raises(_lib.ViboLibraryError, match='null ability'):
                raw(m1.spec, *ops.prepare_rows(resp, mask), rows, t1.table, t1.item_feat, None, None, _lib.REG_KL, True, 64,
                    train_step=(t1._steps.clone(), False, (SEED, 1), True))


@pytest.mark.parametrize('rows', ['in order', 'gathered', 'codes'])
@pytest.mark.parametrize('I', [896, 900])
def test_null_sample_is_taken_exactly_where_the_query_says(I, rows, monkeypatch):
    """vibo_train_step_sample_optional against the call it speaks for, on both sides of the 8-wave line (896 items: 7 waves of 128, 900:
    8) for each way the rows reach the matrix kernel.  Where it answers 1, vibo_elbo_fwd_bwd_step_noise takes ability = NULL and its
    `flat` equals, bit for bit, that of the same call (seed, step counter) with the sample stored; where it answers 0 the call
    returns -5 before anything is launched."""
    monkeypatch.setattr(ops, 'SIGN_ROWS', False)
    B, A = 64, 1
    spec, r, mk, table, item, g = coin_flip_rows(B + 37 if rows == 'gathered' else B, I, A, 7)
    index = torch.randperm(B + 37, device=r.device, generator=g)[:B] if rows == 'gathered' else None
    r, m8, code = ops.prepare_rows(ops.pack_cell_codes(r, mk) if rows == 'codes' else r, None if rows == 'codes' else mk)

    def launch(no_sample):
        steps = torch.tensor([0, 11], dtype=torch.int32, device=dev())
        return ops._hip_launch_elbo(spec, r, m8, code, index, table, item, None, None, _lib.REG_KL, True, B,
                                    train_step=ops.TrainStepCall(steps, False, (SEED, 1), no_sample=no_sample))

    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        desc = ops._rows_desc(spec, B, r, m8, code, _lib.REG_KL, True)
        optional = _lib.load().vibo_train_step_sample_optional(ctypes.byref(desc), int(index is not None))
        assert optional == (0 if rows == 'gathered' and I == 896 else 1)
        if not optional:
            with pytest.raises(_lib.ViboLibraryError, match=r'rc=-5\).*null ability'):
                launch(True)
            return
        lazy, stored = launch(True), launch(False)
    torch.cuda.synchronize()
    assert lazy.ability is None and stored.ability is not None
    assert torch.equal(lazy.flat.view(torch.int32), stored.flat.view(torch.int32))


def test_the_kernel_is_handed_no_sample_buffer_and_none_is_allocated(monkeypatch):
    """The drawing launch gets NULL for ability_mu, ability_logvar AND ability, and the step's record holds no [B, A] tensor until the
    sample is read; read before update() (the table still in place, the counter not yet ticked) it is the twin's stored sample too."""
    B, I, A = 2100, 1000, 8
    resp, mask = problem(B, I, A, 'missing')
    calls = []
    real_call = ops._call

    def recording_call(name, *args):
        calls.append((name, args))
        return real_call(name, *args)

    monkeypatch.setattr(ops, '_call', recording_call)
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        m1, m2, t1, t2 = twins(A, I)
        raw = t1.forward_backward(resp, mask)
        launch = [args for name, args in calls if name == 'vibo_elbo_fwd_bwd_step_noise']
        assert len(launch) == 1
        # (descriptor, step_count, skip_finalize, response, mask, row_index, table, item, eps, seed, stream id, out_scalars, then:)
        eps, (ability_mu, ability_logvar, ability) = launch[0][8], launch[0][12:15]
        assert all(p is None or (isinstance(p, ctypes.c_void_p) and not p.value) for p in (eps, ability_mu, ability_logvar, ability))
        assert not any(isinstance(v, torch.Tensor) and v.numel() == B * A for v in vars(raw).values())
        open_sample = raw.ability.clone()                    # (rebuilt from `table` and step_count[1] as they stand)
        t1.update()
        t2.step(resp, mask)
        assert torch.equal(open_sample, t2.last.ability)
        assert torch.equal(t1.last.flat, t2.last.flat)
    assert_same_parameters(m1, m2)


def test_the_rebuild_is_refused_after_the_next_update_and_under_capture():
    B, I, A = 2100, 1000, 8
    resp, mask = problem(B, I, A, 'missing')
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        m1, m2, t1, t2 = twins(A, I, max_batch=B)
        t1.step(resp, mask)
        first = t1.last
        t1.step(resp, mask)
        with pytest.raises(RuntimeError, match='before the next update'):
            first.ability
        second = t1.last
        torch.cuda.synchronize()
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                with pytest.raises(RuntimeError, match='after the capture'):
                    second.ability
                t1.step(resp, mask)
        torch.cuda.current_stream().wait_stream(side)


def test_a_replayed_step_returns_the_replayed_sample():
    """Capture once, replay twice: `last.ability` of the captured step is rebuilt from what the last replay left, and equals the
    eager four-launch twin's stored sample of the same step; another replay, another sample (nothing cached across replays)."""
    B, I, A = 2100, 1000, 8
    resp, mask = problem(B, I, A, 'missing')
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        m1, m2, t1, t2 = twins(A, I, max_batch=B)
        for _ in range(2):
            assert torch.equal(t1.step(resp, mask), t2.step(resp, mask))
        torch.cuda.synchronize()
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                loss = t1.step(resp, mask)
        torch.cuda.current_stream().wait_stream(side)
        captured = t1.last
        for _ in range(2):
            graph.replay()
            assert torch.equal(loss, t2.step(resp, mask))
        assert torch.equal(captured.ability, t2.last.ability) and torch.equal(captured.flat, t2.last.flat)
        before = captured.ability.clone()
        graph.replay()
        t2.step(resp, mask)
        assert torch.equal(captured.ability, t2.last.ability) and not torch.equal(captured.ability, before)
    assert_same_parameters(m1, m2)
