"""The folded train step on the matrix row-split kernel draws its ability noise in the kernel (vibo_elbo_fwd_bwd_step_noise
with eps NULL) and may leave the posterior's mean / log-variance unwritten.  The drawn noise has to be, bit for bit, what
vibo_fill_normal leaves in memory at the same counter, so the sample, the loss and every gradient stay what they were."""
import ctypes

import pytest
import torch

from gpu_common import assert_same_parameters, coin_flip_rows, simulated, twin_trainers
from vibo_amd import _lib, ops
from vibo_amd.torch_core.models import VIBO_2PL

SEED, STREAM = 0x1234_5678_9ABC, 3


def _problem(B, I, A, gathered, seed=7, codes=False):
    P = B + 37 if gathered else B
    spec, r, mk, table, item, g = coin_flip_rows(P, I, A, seed)
    rows = torch.randperm(P, device=r.device, generator=g)[:B] if gathered else None
    r2, m8, code = ops.prepare_rows(ops.pack_cell_codes(r, mk) if codes else r, None if codes else mk)
    return spec, r2, m8, code, rows, table, item


def _fill(n, steps, stream=STREAM):
    out = torch.empty(n, device=steps.device)
    cur = ctypes.c_void_p(torch.cuda.current_stream(steps.device).cuda_stream)
    _lib.check(_lib.load().vibo_fill_normal(ops._ptr(out), n, SEED, ctypes.c_void_p(steps.data_ptr() + 4), stream, cur), 'vibo_fill_normal')
    return out


def _drawn_against_filled(spec, r, m8, code, rows, table, item, B, I, A):
    """One drawing call and one call reading vibo_fill_normal's noise at the same counter -> (drawn, ref, eps)."""
    d = item.device
    steps = torch.tensor([0, 11], dtype=torch.int32, device=d)
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        desc = ops._make_desc(spec, B, I, code, _lib.REG_KL, True, (I + 3) & ~3, (I + 3) & ~3)
        assert _lib.load().vibo_train_step_draws_noise(ctypes.byref(desc)) == 1
        drawn = ops._hip_launch_elbo(spec, r, m8, code, rows, table, item, None, None, _lib.REG_KL, True, B,
                                     train_step=(steps, False, (SEED, STREAM)))
        eps = _fill(B * A, steps).view(B, A)
        ref = ops._hip_launch_elbo(spec, r, m8, code, rows, table, item, eps, None, _lib.REG_KL, True, B, train_step=(steps, False))
    torch.cuda.synchronize()
    assert drawn.ability_mu is None and drawn.ability_logvar is None
    assert int(steps[0]) == 2 and int(steps[1]) == 11          # ([1] is the draw counter: read, never written)
    return drawn, ref, eps


@pytest.mark.gpu
@pytest.mark.parametrize('B,I,A,rows', [(20000, 1000, 8, 'all'), (20000, 1000, 5, 'gathered'), (20011, 1000, 8, 'codes'),
                                        (70000, 200, 2, 'all'), (40001, 640, 8, 'gathered'), (33000, 384, 1, 'all')])
def test_drawn_noise_over_many_batches_per_workgroup(B, I, A, rows):
    """The minibatch's 32-row batches outnumber the matrix kernel's workgroups (256 of the 8-wave width on 256 CUs, 1024 at
    2 waves), by a count that is no multiple of the grid: every workgroup draws in its batch loop for the next batch (both call
    sites: fp32 rows in order / gathered and cell codes), the drawing wave rotates over all waves of the workgroup (8, 5, 3 and 2
    waves), the one LDS noise buffer is reused across the loop's back edge, and the workgroups with one batch fewer start
    `late`.  Sample, scalars and gradients bit for bit against the call that reads vibo_fill_normal's noise."""
    spec, r, m8, code, idx, table, item = _problem(B, I, A, rows == 'gathered', codes=rows == 'codes')
    nw = (I + 127) // 128
    grid = torch.cuda.get_device_properties(0).multi_processor_count * max(1, 8 // nw)
    n_batches = (B + 31) // 32
    assert n_batches > 2 * grid and n_batches % grid != 0, (n_batches, grid)
    drawn, ref, eps = _drawn_against_filled(spec, r, m8, code, idx, table, item, B, I, A)
    assert torch.equal(drawn.ability.view(torch.int32), ref.ability.view(torch.int32))
    assert torch.equal(drawn.flat.view(torch.int32), ref.flat.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('A', [1, 2, 4, 5, 8])
@pytest.mark.parametrize('B,I', [(301, 1000), (77, 200), (1030, 640)])
@pytest.mark.parametrize('gathered', [False, True])
def test_drawn_noise_equals_the_filled_noise(A, B, I, gathered):
    """theta of the drawing call = mu + exp(logvar / 2) eps with eps = vibo_fill_normal at the same counter, and the whole call
    (sample, scalars, gradients) equals the call that reads that eps -- bit for bit.  B is no multiple of 4 or 32; 200 items
    run 2 waves per workgroup (the slot loop), 640 five, 1000 eight."""
    spec, r, m8, code, rows, table, item = _problem(B, I, A, gathered)
    drawn, ref, eps = _drawn_against_filled(spec, r, m8, code, rows, table, item, B, I, A)
    assert torch.equal(drawn.ability.view(torch.int32), ref.ability.view(torch.int32))
    assert torch.equal(drawn.flat.view(torch.int32), ref.flat.view(torch.int32))
    theta = ref.ability_mu + torch.exp(0.5 * ref.ability_logvar) * eps
    assert (drawn.ability - theta).abs().max() <= 1e-5 * max(1.0, float(theta.abs().max()))


@pytest.mark.gpu
def test_step_with_null_posterior_outputs_leaves_them_untouched():
    """vibo_elbo_fwd_bwd_step with NULL ability_mu / ability_logvar (explicit eps): the sample and the records are those of the
    call that writes the posterior, and buffers handed to neither call keep their sentinel."""
    B, I, A = 2100, 1000, 8
    spec, r, m8, code, rows, table, item = _problem(B, I, A, False)
    d = r.device
    lib = _lib.load()
    steps = torch.zeros(2, dtype=torch.int32, device=d)
    eps = torch.randn(B, A, device=d)
    sentinel = float('-1.25e+30')
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX):
        desc = ops._make_desc(spec, B, I, code, _lib.REG_KL, True, r.stride(0), m8.stride(0))
        ws = torch.empty(lib.vibo_workspace_bytes(ctypes.byref(desc)), dtype=torch.uint8, device=d)
        cur = ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream)
        outs = []
        for with_post in (True, False):
            flat = torch.empty(8 + 2 * 2 * 2 * A + I * (A + 1), device=d)
            post = torch.full((3, B, A), sentinel, device=d)
            p = ops._ptr
            rc = lib.vibo_elbo_fwd_bwd_step(ctypes.byref(desc), p(steps), 0, p(r), p(m8), None, p(table), p(item), p(eps), p(flat),
                                            p(post[0]) if with_post else None, p(post[1]) if with_post else None, p(post[2]),
                                            ctypes.c_void_p(flat.data_ptr() + 4 * 8), ctypes.c_void_p(flat.data_ptr() + 4 * (8 + 8 * A)),
                                            p(ws), ws.numel(), cur)
            _lib.check(rc, 'vibo_elbo_fwd_bwd_step')
            outs.append((flat, post))
    torch.cuda.synchronize()
    (f1, p1), (f2, p2) = outs
    assert torch.equal(f1.view(torch.int32), f2.view(torch.int32))
    assert torch.equal(p1[2].view(torch.int32), p2[2].view(torch.int32))
    assert bool((p1[0] != sentinel).all()) and bool((p1[1] != sentinel).all())
    assert bool((p2[0] == sentinel).all()) and bool((p2[1] == sentinel).all())


@pytest.mark.gpu
@pytest.mark.parametrize('pin,P,B', [(True, 4700, 4096), (False, 4700, 4096), (False, 20600, 20000)])
def test_drawing_step_survives_graph_replays_and_a_shorter_minibatch(pin, P, B):
    """The folded step (drawing its noise) replayed from a hipGraph, with an eager, shorter minibatch between replays, against
    the four-launch form: bit for bit.  pin=False: the planner's own choice -- the full minibatch on the matrix kernel, the
    short one on the VALU kernel, which then has to fill the noise buffer itself (no epilogue does any more).  20 000 persons:
    625 batches over 256 workgroups (the batch loop's draws, the `late` workgroups) inside the captured step."""
    dev = torch.device('cuda:0')
    I, A, n_short = 1000, 8, 45
    resp, mask, g = simulated(2, P, I, A, 0.1, seed=4)
    resp, mask = resp.to(dev), mask.bool().to(dev)
    rows = torch.randperm(P, generator=g)[:B].to(dev)
    short = torch.arange(P - n_short, P, device=dev)
    with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX if pin else 0):
        m1, m2, t1, t2 = twin_trainers(VIBO_2PL, A, I, 2, dict(rng='native', seed=3, max_batch=B), dict(rng='native', seed=3, fold=False))
        kinds = {ops.plan_kernel(m1.spec, n, I).split()[0] for n in (B, n_short)}
        assert kinds == ({'matrix'} if pin else {'matrix', 'VALU'}), kinds
        for k in range(3):
            rr = short if k == 1 else rows
            la, lb = t1.step(resp, mask, row_index=rr), t2.step(resp, mask, row_index=rr)
            assert torch.equal(la, lb), k
            assert torch.equal(t1.last.ability, t2.last.ability) and torch.equal(t1.last.flat, t2.last.flat), k
        assert t1.last.ability_mu is None and t1.last.ability_logvar is None
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                lg = t1.step(resp, mask, row_index=rows)
        torch.cuda.current_stream().wait_stream(side)
        for it in range(4):
            if it == 2:
                la, lb = t1.step(resp, mask, row_index=short), t2.step(resp, mask, row_index=short)
            else:
                graph.replay()
                la, lb = lg, t2.step(resp, mask, row_index=rows)
            assert torch.equal(la, lb), it
    assert_same_parameters(m1, m2)


def test_drawing_entry_points_check_their_arguments():
    """Host-side checks of the drawing entry point and its query (no GPU needed)."""
    lib = _lib.load()
    d = _lib.ViboDesc()
    assert lib.vibo_train_step_draws_noise(ctypes.byref(d)) == 0               # (zeroed descriptor: wrong abi_version)
    assert lib.vibo_elbo_fwd_bwd_step_noise(ctypes.byref(d), None, 0, None, None, None, None, None, None, 0, 0,
                                            *([None] * 6), None, 0, None) == -5
    d.abi_version = _lib.ABI_VERSION
    d.num_person, d.num_item, d.ability_dim, d.irt_model, d.want_grad = 100, 64, 2, 2, 1
    d.mask_dtype, d.response_row_stride, d.mask_row_stride = _lib.MASK_U8, 64, 64
    d.flags = _lib.FLAG_KERNEL_VALU                                             # (the VALU kernel takes explicit noise)
    assert lib.vibo_train_step_supported(ctypes.byref(d)) & 1
    assert lib.vibo_train_step_draws_noise(ctypes.byref(d)) == 0
    d.flags = _lib.FLAG_KERNEL_MATRIX
    assert lib.vibo_train_step_draws_noise(ctypes.byref(d)) == 1
    d.posterior = _lib.POSTERIOR_CONDITIONAL                                    # (not a folded step at all)
    assert lib.vibo_train_step_draws_noise(ctypes.byref(d)) == 0
