#!/usr/bin/env python3
"""Train-step time of the module path (elbo_step + backward + Adam) eager vs replayed from a hipGraph
(vibo_amd.torch_core.vibo.GraphedModuleStep), for the configurations FusedTrainer does not cover.
   python tools/step_time.py [--irt 3] [--items 1000] [--ability-dim 1] [--batch 16] [--cond] [--flows 4] [--merge product]
With --generative-model link | deep | residual: the module step (eager) against FusedDecoderTrainer's native step, eager and
replayed from a hipGraph, A/B interleaved on one box in --blocks blocks of --steps steps; medians and ranges per leg:
   python tools/step_time.py --generative-model deep --irt 2 --items 100 --batch 16 --persons 20000 --blocks 5
With --method vi | mle: the un-amortized methods -- the module step as vi.py / mle.py run it (autograd + torch.optim.Adam on the
dense embeddings) against FusedVITrainer / FusedMLETrainer, eager and replayed, the same interleaved blocks (rows as 1-byte cell
codes, the CLIs' default on the GPU):
   python tools/step_time.py --method vi --irt 2 --persons 1000000 --items 1000 --batch 16 --ability-dim 8 --blocks 5 --steps 50
With --table-update: the person-table update alone (vibo_person_table_adam, HIP events around the call) at --persons x --ability-dim
entries per table, as a fraction of 24 B per entry at the 6.29 TB/s copy ceiling:
   python tools/step_time.py --method vi --table-update --persons 1000000 --ability-dim 8
With --whole-matrix: the native trainer's step on the WHOLE resident matrix (no row_index: --batch is not read), replayed from a
hipGraph, with ops.TILE_ROWS_GIVEN off (the VIBO_POSTERIOR_GIVEN launch on the rows) against on (on the matrix' tile image),
interleaved blocks on one box; step = wall clock per replay, kernel = the GIVEN launch's own stamps (ops.InsituTimer).  For
--merge mean (FusedMeanTrainer) and --method vi | mle (fp32 rows with a mask; --codes: 1-byte cell codes):
   python tools/step_time.py --whole-matrix --merge mean --irt 2 --persons 1000000 --items 1000 --ability-dim 8 --blocks 5 --steps 50"""
import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
for p in (ROOT, os.path.join(ROOT, 'variational-item-response-theory-public_amd')):
    sys.path.insert(0, p)
import torch
from vibo_amd.torch_core import models as M
from vibo_amd.torch_core.vibo import GraphedModuleStep

ap = argparse.ArgumentParser()
ap.add_argument('--persons', type=int, default=20000)
ap.add_argument('--items', type=int, default=1000)
ap.add_argument('--ability-dim', type=int, default=1)
ap.add_argument('--irt', type=int, default=3)
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--cond', action='store_true')
ap.add_argument('--flows', type=int, default=0)
ap.add_argument('--merge', default='product')
ap.add_argument('--generative-model', default='irt', choices=['irt', 'link', 'deep', 'residual'])
ap.add_argument('--hidden-dim', type=int, default=64)
ap.add_argument('--blocks', type=int, default=5, help='MLP decoders: interleaved timing blocks per leg')
ap.add_argument('--steps', type=int, default=200, help='MLP decoders: steps per block')
ap.add_argument('--method', default='vibo', choices=['vibo', 'vi', 'mle'], help='vi | mle: the un-amortized methods (per-person tables)')
ap.add_argument('--table-update', action='store_true', help='--method vi | mle: time vibo_person_table_adam alone')
ap.add_argument('--whole-matrix', action='store_true', help='--merge mean / --method vi | mle: the whole-matrix step, tile image off vs on')
ap.add_argument('--codes', action='store_true', help='--whole-matrix: rows as 1-byte cell codes')
a = ap.parse_args()
d = torch.device('cuda:0')
g = torch.Generator(device=d).manual_seed(0)
P, I, A, B = a.persons, a.items, a.ability_dim, a.batch


class Data:
    pass


data = Data()
if not a.table_update:
    data.response = (torch.rand(P, I, device=d, generator=g) < 0.5).float()
    data.mask = torch.rand(P, I, device=d, generator=g) >= 0.1
data.device = d
cls = {1: M.VIBO_1PL, 2: M.VIBO_2PL, 3: M.VIBO_3PL}[a.irt]


def decoder_legs():
    """Module step (eager; its captured form is not replayed here: DESIGN.md 4) vs the native step, eager and replayed."""
    import statistics
    from vibo_amd.trainer import FusedTrainer, fused_decoder_trainer_covers
    kw = dict(hidden_dim=a.hidden_dim, ability_merge=a.merge, conditional_posterior=a.cond, n_norm_flows=a.flows,
              generative_model=a.generative_model)
    rows = [torch.randperm(P, device=d)[:B].contiguous() for _ in range(8)]
    rbuf = torch.zeros(B, dtype=torch.int64, device=d)
    torch.manual_seed(0)
    m_mod = cls(A, I, **kw).to(d)
    opt = torch.optim.Adam(m_mod.parameters(), lr=5e-3, fused=True)      # (as the CLI builds it)

    def module_step(k):                   # train_epoch's own eager loop, on the current stream
        opt.zero_grad(set_to_none=True)
        loss = m_mod.elbo_step(data.response, data.mask, annealing_factor=1.0, row_index=rows[k % 8])
        loss.backward()
        opt.step()
        return loss.detach()
    legs = {'module eager': module_step}
    if fused_decoder_trainer_covers(m_mod):
        torch.manual_seed(0)
        tr_e = FusedTrainer(cls(A, I, **kw).to(d), lr=5e-3, rng='native', seed=3)
        legs['native eager'] = lambda k: tr_e.step(data.response, data.mask, row_index=rows[k % 8])
        torch.manual_seed(0)
        tr_g = FusedTrainer(cls(A, I, **kw).to(d), lr=5e-3, rng='native', seed=3)
        for k in range(4):
            rbuf.copy_(rows[k]); tr_g.step(data.response, data.mask, row_index=rbuf)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            loss_g = tr_g.step(data.response, data.mask, row_index=rbuf)

        def replay(k):
            rbuf.copy_(rows[k % 8]); gr.replay()
            return loss_g
        legs['native graph'] = replay
    time_legs(legs, f'{a.generative_model} irt={a.irt} I={I} A={A} B={B} H={a.hidden_dim}')


def time_legs(legs, label):
    """A/B interleaved: --blocks blocks of --steps steps per leg; medians and ranges."""
    import statistics
    for fn in legs.values():
        for k in range(4):
            fn(k)
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for blk in range(a.blocks):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.steps):
                loss = fn(k)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e6)
            print(f'  block {blk} {name:13s}: {times[name][-1]:10.1f} us/step  loss {float(loss):.4f}', flush=True)
    for name, t in times.items():
        print(f'{label} {name:13s}: median {statistics.median(t):10.1f} us/step  '
              f'range {min(t):.1f} .. {max(t):.1f}  ({a.blocks} blocks x {a.steps} steps)', flush=True)


def person_table_legs():
    """vi.py / mle.py's own train step (module + autograd + torch.optim.Adam over the dense embeddings) vs the native step, eager and
    replayed.  Person = row of the resident split, minibatches are row-index vectors."""
    from vibo_amd import ops
    from vibo_amd.torch_core.vi import ResidentVI
    from vibo_amd.trainer import FusedTrainer
    mcls = {'vi': {1: M.VI_1PL, 2: M.VI_2PL, 3: M.VI_3PL}, 'mle': {1: M.MLE_1PL, 2: M.MLE_2PL, 3: M.MLE_3PL}}[a.method][a.irt]
    response, mask = ops.pack_cell_codes(data.response, data.mask), None
    del data.response, data.mask
    rows = [torch.randperm(P, device=d)[:B].contiguous() for _ in range(8)]
    rbuf = torch.zeros(B, dtype=torch.int64, device=d)

    def build():
        torch.manual_seed(0)
        return mcls(A, P, I).to(d)
    m_mod = build()
    opt = torch.optim.Adam(m_mod.parameters(), lr=5e-3)                   # (as vi.py / mle.py build it)
    face = ResidentVI(m_mod) if a.method == 'vi' else None

    def module_step(k):
        opt.zero_grad(set_to_none=True)
        if face is not None:
            loss = face.elbo_step(response, mask, annealing_factor=1.0, row_index=rows[k % 8])
        else:
            loss = m_mod.nll_step(rows[k % 8], response, mask, row_index=rows[k % 8])
        loss.backward()
        opt.step()
        return loss.detach()
    tr_e = FusedTrainer(build(), lr=5e-3, rng='native', seed=3)
    tr_g = FusedTrainer(build(), lr=5e-3, rng='native', seed=3)
    for k in range(4):
        rbuf.copy_(rows[k]); tr_g.step(response, mask, row_index=rbuf)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        loss_g = tr_g.step(response, mask, row_index=rbuf)

    def replay(k):
        rbuf.copy_(rows[k % 8]); gr.replay()
        return loss_g
    legs = {'module eager': module_step, 'native eager': lambda k: tr_e.step(response, mask, row_index=rows[k % 8]), 'native graph': replay}
    time_legs(legs, f'{a.method} irt={a.irt} P={P} I={I} A={A} B={B}')


def table_update_time():
    """vibo_person_table_adam alone, HIP events around each call (claims + update + reset: the export's three launches)."""
    import ctypes
    import statistics
    from vibo_amd import _lib, ops
    T = 2 if a.method == 'vi' else 1
    n = P * A
    stride = (n + 3) // 4 * 4
    tabs = [torch.randn(P, A, device=d) for _ in range(T)]
    m, v = torch.zeros(T, stride, device=d), torch.zeros(T, stride, device=d)
    slot = torch.full((P,), -1, dtype=torch.int32, device=d)
    bad = torch.zeros(1, dtype=torch.int32, device=d)
    idx = torch.randperm(P, device=d)[:B].contiguous()
    grows = torch.randn(2, B, 2 * A, device=d)
    steps = torch.tensor([1, 0], dtype=torch.int32, device=d)
    scal = torch.tensor([1.0, 5e-3], device=d)
    dsc = ops._make_desc(ops.ElboSpec(irt_model=a.irt, ability_dim=A, given=True), B, I, _lib.MASK_U8, _lib.REG_KL, True, I, I)
    p = ops._ptr

    def call():
        ops._call('vibo_person_table_adam', ctypes.byref(dsc), _lib.PTRAIN_VI if T == 2 else _lib.PTRAIN_MLE, P, p(idx), p(grows), p(scal[0:1]),
                  p(scal[1:2]), p(steps), p(tabs[0]), p(tabs[1]) if T > 1 else None, p(m), p(v), stride, p(slot), p(bad), ops._stream(d))
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    floor = T * n * 24 / 6.29e12 * 1e6
    med = statistics.median(us)
    print(f'table update {a.method} P={P} A={A} ({T} x {n} entries, B={B}): median {med:.1f} us  range {min(us):.1f} .. {max(us):.1f} '
          f'({a.steps} calls); 24 B/entry at 6.29 TB/s = {floor:.1f} us -> {floor / med:.2f} of the copy ceiling', flush=True)


def whole_matrix_legs():
    """The whole-matrix step of the trainers whose ELBO launch reads a caller-supplied posterior, replayed from a hipGraph: the launch
    on the rows (ops.TILE_ROWS_GIVEN off) against the launch on the matrix' tile image (on).  One trainer and one graph per leg, from
    the same seed, on the same matrix; the legs alternate block by block."""
    import statistics
    from vibo_amd import ops
    from vibo_amd.trainer import FusedTrainer
    if a.method == 'vibo':
        def build():
            torch.manual_seed(0)
            return cls(A, I, ability_merge=a.merge).to(d)
    else:
        mcls = {'vi': {1: M.VI_1PL, 2: M.VI_2PL, 3: M.VI_3PL}, 'mle': {1: M.MLE_1PL, 2: M.MLE_2PL, 3: M.MLE_3PL}}[a.method][a.irt]

        def build():
            torch.manual_seed(0)
            return mcls(A, P, I).to(d)
    response, mask = (ops.pack_cell_codes(data.response, data.mask), None) if a.codes else (data.response, data.mask)
    legs, names = {}, []
    real_call = ops._call

    def logging_call(name, *args):
        if name.startswith('vibo_elbo_fwd_bwd'):
            names.append(name)
        return real_call(name, *args)
    ops._call = logging_call
    for leg, on in (('rows', False), ('tile image', True)):
        ops.TILE_ROWS_GIVEN = on
        tr = FusedTrainer(build(), lr=5e-3, rng='native', seed=3)
        timer = ops.InsituTimer(d)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                tr.step(response, mask)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        del names[:]
        gr = torch.cuda.CUDAGraph()
        with timer:
            with torch.cuda.graph(gr):
                loss = tr.step(response, mask)
        legs[leg] = (tr, gr, loss, timer, list(names))
        for _ in range(5):
            gr.replay()
        torch.cuda.synchronize()
    ops._call = real_call
    label = f'{type(legs["rows"][0]).__name__} irt={a.irt} P={P} I={I} A={A} {"cell codes" if a.codes else "fp32 + mask"}'
    for leg, (_, _, _, _, sent) in legs.items():
        print(f'{label} {leg:10s}: captured ELBO entry point {sent}', flush=True)
    step_us, kern_us = {leg: [] for leg in legs}, {leg: [] for leg in legs}
    for blk in range(a.blocks):
        for leg, (_, gr, loss, timer, _) in legs.items():
            timer.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                gr.replay()
            torch.cuda.synchronize()
            step_us[leg].append((time.perf_counter() - t0) / a.steps * 1e6)
            k = timer.read()
            kern_us[leg].append(k.get('mean_ms', 0.0) * 1e3)
            print(f'  block {blk} {leg:10s}: step {step_us[leg][-1]:9.1f} us  kernel {kern_us[leg][-1]:9.1f} us (min {k.get("min_ms", 0.0) * 1e3:.1f}, '
                  f'{k.get("launches", 0)} launches)  loss {float(loss):.6g}', flush=True)
    for leg in legs:
        s, k = step_us[leg], kern_us[leg]
        print(f'{label} {leg:10s}: step median {statistics.median(s):9.1f} us  range {min(s):.1f} .. {max(s):.1f} | kernel median '
              f'{statistics.median(k):9.1f} us  range {min(k):.1f} .. {max(k):.1f}  ({a.blocks} blocks x {a.steps} steps)', flush=True)


if a.whole_matrix:
    whole_matrix_legs()
    sys.exit(0)
if a.method != 'vibo':
    table_update_time() if a.table_update else person_table_legs()
    sys.exit(0)


if a.generative_model != 'irt':
    decoder_legs()
    sys.exit(0)
for mode in ('eager', 'graph'):
    torch.manual_seed(0)
    model = cls(A, I, ability_merge=a.merge, conditional_posterior=a.cond, n_norm_flows=a.flows).to(d)
    opt = torch.optim.Adam(model.parameters(), lr=5e-3, capturable=mode == 'graph', fused=True)      # (as the CLI builds it)
    step = GraphedModuleStep(model, opt, data, B)
    if mode == 'eager':
        step.WARMUP = 1 << 30
    rows = [torch.randperm(P, device=d)[:B].contiguous() for _ in range(8)]
    for k in range(6):
        step(rows[k % 8], 1.0)
    torch.cuda.synchronize()
    n = 200
    t0 = time.perf_counter()
    for k in range(n):
        loss = step(rows[k % 8], 1.0)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    print(f'irt={a.irt} I={I} A={A} B={B} cond={a.cond} flows={a.flows} merge={a.merge} {mode:6s}: {dt * 1e6:9.1f} us/step  loss {float(loss):.1f}')

# the same configuration through the fused trainer (FusedTrainer / FusedCondFlowTrainer), eager and replayed
from vibo_amd.trainer import FusedTrainer, fused_trainer_covers
torch.manual_seed(0)
model = cls(A, I, ability_merge=a.merge, conditional_posterior=a.cond, n_norm_flows=a.flows).to(d)
if fused_trainer_covers(model):
    tr = FusedTrainer(model, lr=5e-3, rng='native', seed=3)
    rbuf = torch.zeros(B, dtype=torch.int64, device=d)
    rows = [torch.randperm(P, device=d)[:B].contiguous() for _ in range(8)]
    for k in range(4):
        rbuf.copy_(rows[k]); tr.step(data.response, data.mask, row_index=rbuf)
    torch.cuda.synchronize()
    n = 200
    t0 = time.perf_counter()
    for k in range(n):
        rbuf.copy_(rows[k % 8]); loss = tr.step(data.response, data.mask, row_index=rbuf)
    torch.cuda.synchronize()
    print(f'fused trainer ({type(tr).__name__}) eager : {(time.perf_counter() - t0) / n * 1e6:9.1f} us/step  loss {float(loss):.1f}')
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        loss = tr.step(data.response, data.mask, row_index=rbuf)
    for k in range(5):
        gr.replay()
    torch.cuda.synchronize()
    n = 1000
    t0 = time.perf_counter()
    for k in range(n):
        rbuf.copy_(rows[k % 8]); gr.replay()
    torch.cuda.synchronize()
    print(f'fused trainer ({type(tr).__name__}) graph : {(time.perf_counter() - t0) / n * 1e6:9.1f} us/step  loss {float(loss):.1f}')
