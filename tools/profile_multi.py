#!/usr/bin/env python3
"""Multi-sample forward (log_marginal's loop body) vs one forward launch per sample.
   python tools/profile_multi.py [--persons P] [--items I] [--ability-dim A] [--samples S] [--given [--per-sample] | --cond]
--given: a caller-supplied posterior (VIBO_POSTERIOR_GIVEN: --ability-merge mean, VI_*PL) through vibo_elbo_multi_forward_given,
one [P, 2A] posterior for all samples, or with --per-sample one per sample ([S, P, 2A]: mean merge x conditional posterior); the
singles leg is then one GIVEN forward launch (want_grad = 0) per sample.
--cond: the product of experts of the conditional posterior through vibo_elbo_multi_forward_cond, one encoder table per sample
([S, 2, I, 2A]); the singles leg is one conditional forward launch per sample.
--log-marginal: the module instead of the kernel legs -- VIBO_*PL(...).log_marginal of this checkout's package on the same rows
(with --minibatch N: summed over minibatches of N persons, as the reference's evaluation pass), torch.manual_seed(7) in front of
every call; prints `log_marginal <ms median> <min> <max> <value>`.  Run from two checkouts for a parent / new comparison.
--generative-model link | deep | residual: the MLP-decoder model instead (with --log-marginal; with --predictive:
vibo.posterior_predictive's mean over --samples draws in minibatches of --minibatch, prints `posterior_predictive <ms ...> <sum>`).
These decoder legs warm up on the first and the last minibatch only (every shape of the timed pass); the IRT legs on a whole pass.
--decoder-kernel deep | link | residual: the kernel legs of the decoder -- vibo_decoder_multi_forward on --samples stacked samples
against one vibo_decoder_fwd_bwd forward launch per sample."""
import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
for p in (ROOT, os.path.join(ROOT, 'variational-item-response-theory-public_amd')):
    sys.path.insert(0, p)
import torch
from vibo_amd import _lib, ops
from vibo_amd.ops import ElboSpec

ap = argparse.ArgumentParser()
ap.add_argument('--persons', type=int, default=1_000_000)
ap.add_argument('--items', type=int, default=1000)
ap.add_argument('--ability-dim', type=int, default=1)
ap.add_argument('--samples', type=int, default=16)
ap.add_argument('--irt', type=int, default=2)
ap.add_argument('--codes', action='store_true', help='rows as 1-byte cell codes (VIBO_MASK_CODES)')
ap.add_argument('--gather', action='store_true')
ap.add_argument('--given', action='store_true', help='caller-supplied posterior, shared by the samples')
ap.add_argument('--per-sample', action='store_true', help='with --given: one posterior per sample')
ap.add_argument('--cond', action='store_true', help='product of experts x conditional posterior: one encoder table per sample')
ap.add_argument('--log-marginal', action='store_true', help='time model.log_marginal instead of the kernel legs')
ap.add_argument('--minibatch', type=int, default=0, help='with --log-marginal: persons per call (0: all)')
ap.add_argument('--generative-model', default='irt', choices=['irt', 'link', 'deep', 'residual'])
ap.add_argument('--predictive', action='store_true', help='time vibo.posterior_predictive (mean over the draws) instead')
ap.add_argument('--decoder-kernel', default=None, choices=['link', 'deep', 'residual'], help='decoder kernel legs: stacked vs one launch per sample')
ap.add_argument('--reps', type=int, default=3)
a = ap.parse_args()
d = torch.device('cuda:0')
g = torch.Generator(device=d).manual_seed(0)
P, I, A, S = a.persons, a.items, a.ability_dim, a.samples
spec = ElboSpec(irt_model=a.irt, ability_dim=A, given=a.given, conditional=a.cond)
resp = (torch.rand(P, I, device=d, generator=g) < 0.5).float()
mask = torch.rand(P, I, device=d, generator=g) >= 0.1

if a.log_marginal or a.predictive:
    import types
    from vibo_amd.torch_core import models, vibo
    torch.manual_seed(3)
    model = {1: models.VIBO_1PL, 2: models.VIBO_2PL, 3: models.VIBO_3PL}[a.irt](
        A, I, ability_merge='mean' if a.given else 'product', conditional_posterior=a.cond or a.per_sample,
        **({} if a.generative_model == 'irt' else {'generative_model': a.generative_model})).to(d)
    rows = ops.pack_cell_codes(resp, mask) if a.codes else resp
    step = a.minibatch or P
    starts = list(range(0, P, step))

    def log_marginal_pass(starts):
        torch.manual_seed(7)
        total = 0.0
        for p0 in starts:
            r = rows.rows(torch.arange(p0, min(P, p0 + step), device=d)) if a.codes else rows[p0:p0 + step]
            total += float(model.log_marginal(r, None if a.codes else mask[p0:p0 + step], num_samples=S))      # (float() synchronises)
        return total

    class Rows:      # the slice of vibo.py's dataset that posterior_predictive reads
        def __init__(self, starts):
            self.response, self.mask, self.starts = resp.unsqueeze(2), mask.unsqueeze(2), starts

        def batches(self, batch_size, shuffle=False):
            return [torch.arange(p0, min(P, p0 + step), device=d) for p0 in self.starts]

    def predictive_pass(starts):
        torch.manual_seed(7)
        out = vibo.posterior_predictive(model, Rows(starts), types.SimpleNamespace(num_posterior_samples=S), step, False)
        return float(out['response'].double().sum())          # (the result is on the host: the pass has synchronised)

    one_pass = predictive_pass if a.predictive else log_marginal_pass
    # warm-up: a whole pass; the decoder legs' loop side takes tens of seconds per pass, so they warm the first and the last minibatch
    # only (every shape of the timed pass)
    one_pass(starts if a.generative_model == 'irt' and not a.predictive else sorted({starts[0], starts[-1]}))
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        value = one_pass(starts)
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    print(f'{"posterior_predictive" if a.predictive else "log_marginal"} {times[len(times) // 2]:.3f} {times[0]:.3f} {times[-1]:.3f} {value!r}')
    sys.exit(0)

if a.decoder_kernel:
    from vibo_amd import decoder as D
    kind, Hd = a.decoder_kernel, D.HIDDEN
    rn = lambda *shape, sc=1.0: torch.randn(*shape, device=d, generator=g) * sc
    m8 = ops.prepare_mask(mask)[0]
    U = None if kind == 'link' else rn(S, I, Hd, sc=0.7)
    V, L = rn(S, P, Hd, sc=0.7), (None if kind == 'deep' else rn(S, P, I, sc=1.5))
    w1 = rn(Hd, sc=0.5) if kind == 'link' else None
    W2, b2, w3, b3 = rn(Hd, Hd, sc=0.18), rn(Hd, sc=0.1), rn(Hd, sc=0.25), rn(1, sc=0.1)
    resid = 1.0 if kind == 'residual' else 0.0
    at = lambda t, s: None if t is None else t[s]
    legs = (('stacked launch', lambda: D._launch_multi(resp, m8, U, V, L, None, w1, W2, b2, w3, b3, resid)['ll_part'].sum(1)),
            ('one launch per sample', lambda: torch.stack([D._launch(resp, m8, at(U, s), V[s], at(L, s), None, w1, W2, b2, w3, b3, resid,
                                                                     False)['ll_part'].sum() for s in range(S)])))
    for name, f in legs:
        value = f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            f()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.reps
        print(f'decoder {kind} P={P} I={I} S={S} {name:24s}: {dt * 1e3:8.3f} ms = {dt * 1e3 / S:6.3f} ms per sample, '
              f'{P * I * S / dt / 1e12:.3f} T sample-terms/s, ll[0]={float(value[0])!r}')
    sys.exit(0)

table = torch.randn(2, 2 * A, device=d, generator=g) * 0.5
if a.given:      # mu = 0.5 randn | logvar = -1 + 0.5 randn
    shape = (S, P, A) if a.per_sample else (P, A)
    table = torch.cat([0.5 * torch.randn(shape, device=d, generator=g), -1.0 + 0.5 * torch.randn(shape, device=d, generator=g)], dim=-1)
if a.cond:
    table = torch.randn(S, 2, I, 2 * A, device=d, generator=g) * 0.5
items = torch.randn(S, I, spec.item_dim, device=d, generator=g)
eps = torch.randn(S, P, A, device=d, generator=g)
m, code = ops.prepare_mask(mask)
if a.codes:
    resp, m, code = ops.prepare_rows(ops.pack_cell_codes(resp, mask), None)
ridx = torch.randperm(P, device=d) if a.gather else None
per_sample_table = a.cond or (a.given and a.per_sample)


def multi():
    return ops._hip_multi_forward(spec, resp, m, code, ridx, table, items, eps, None, _lib.REG_SAMPLED, P)


def singles():
    return [ops._hip_launch_elbo(spec, resp, m, code, ridx, table[s] if per_sample_table else table, items[s], eps[s], None,
                                 _lib.REG_SAMPLED, False, P).scalars for s in range(S)]


for name, f in (('multi-sample kernel', multi), ('one launch per sample', singles)):
    if f() is None:
        print(f'{name}: this library does not cover the configuration')
        continue
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        f()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.reps
    print(f'P={P} I={I} A={A} S={S} codes={a.codes} gather={a.gather} given={a.given} per_sample={a.per_sample} cond={a.cond} {name:24s}: {dt * 1e3:8.3f} ms = {dt * 1e3 / S:6.3f} ms per sample, '
          f'{P * I * S / dt / 1e12:.3f} T sample-terms/s')
