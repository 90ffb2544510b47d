"""What tests/test_gpu_decoder_cells.py shares: the launch of vibo_decoder_fwd_bwd with a descriptor of the test's own (so that
person_chunks is the test's choice, not vibo_decoder_person_chunks'), every output on the host in the names of
oracle/decoder_model.py's Layout.shapes, and the comparison of a launch with the model's bounds.  A plain module."""
import ctypes

import numpy as np
import torch

from gpu_common import dev, record
from oracle import decoder_model as D
from vibo_amd import _lib, ops
from vibo_amd import decoder as DEC

MODES = dict(deep=dict(), link=dict(has_U=False, has_w1=True), resid=dict(resid=1.0), guess=dict(has_guess=True),
             logits=dict(force_L=True), all=dict(has_w1=True, resid=1.0, has_guess=True))
NAN = float('nan')


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def device_rows(case, pad=0):
    """-> (response, mask) device views [B, I] with a row stride of I + pad; the padding holds NaN responses under mask bytes 1."""
    resp, mask = case['resp'], case['mask']
    B, I = resp.shape
    rbuf = torch.full((B, I + pad), NAN)
    rbuf[:, :I] = torch.from_numpy(resp)
    mbuf = None
    if mask is not None:
        mbuf = torch.ones((B, I + pad), dtype=torch.uint8)
        mbuf[:, :I] = torch.from_numpy(np.asarray(mask, np.uint8))
        mbuf = mbuf.to(dev())[:, :I]
    return rbuf.to(dev())[:, :I], mbuf


def device_args(case):
    return dict(U=_t(case['U']), V=_t(case['V']), L=_t(case['L']), guess=_t(case['guess']), w1=_t(case['w1']), W2=_t(case['W2']),
                b2=_t(case['b2']), w3=_t(case['w3']), b3=torch.tensor([case['b3']], dtype=torch.float32, device=dev()))


def launch(case, chunks, want_grad=True, pad=0):
    """vibo_decoder_fwd_bwd on `case` with `chunks` person chunks -> dict of numpy arrays (Layout.shapes' names and 'prob'); the
    buffers start as NaN, so an entry the kernel does not write shows.  Every buffer has exactly the size the layout states."""
    resp, mask = device_rows(case, pad)
    B, I = resp.shape
    lay = D.layout(B, I, chunks)
    a = device_args(case)
    d = _lib.ViboDecoderDesc(B, I, DEC.HIDDEN, int(want_grad), chunks, float(case['resid']), resp.stride(0), mask.stride(0) if mask is not None else 0)
    new = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=dev())
    out = {'ll_part': new(*lay.shapes['ll_part']), 'prob': new(B, I)}
    if want_grad:
        for k in ('dW2_part', 'dvec_part', 'dV_part'):
            out[k] = new(*lay.shapes[k])
        if a['U'] is not None:
            out['dU_part'] = new(*lay.shapes['dU_part'])
        if a['L'] is not None:
            out['dL'] = new(B, I)
        if a['guess'] is not None:
            out['dguess_part'] = new(*lay.shapes['dguess_part'])
    p = ops._ptr
    ops._call('vibo_decoder_fwd_bwd', ctypes.byref(d), p(resp), p(mask), p(a['U']), p(a['V']), p(a['L']), p(a['guess']), p(a['w1']), p(a['W2']),
              p(a['b2']), p(a['w3']), p(a['b3']), p(out['ll_part']), p(out.get('dU_part')), p(out.get('dV_part')), p(out.get('dL')),
              p(out.get('dguess_part')), p(out.get('dW2_part')), p(out.get('dvec_part')), p(out['prob']), ops._stream(dev()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def launch_multi(case, chunks, S=2):
    """decoder._launch_multi on S copies of the case's sample -> ll_part [S, n_wave] (numpy)."""
    resp, mask = device_rows(case)
    a = device_args(case)
    st = lambda t: None if t is None else t.unsqueeze(0).expand(S, *t.shape).contiguous()
    out = DEC._launch_multi(resp, mask, st(a['U']), st(a['V']), st(a['L']), st(a['guess']), a['w1'], a['W2'], a['b2'], a['w3'], a['b3'],
                            float(case['resid']), person_chunks=chunks)
    torch.cuda.synchronize()
    return out['ll_part'].cpu().numpy()


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


def given_dz2(got, case, lay):
    """`single` layout: the one observed term of each wave has its dz2 in dvec_part row 0, bit for bit (the other terms add zeros)."""
    B, I = lay.B, lay.I
    dz = np.zeros((B, I, D.H))
    for p, i in np.argwhere(np.asarray(case['mask']) != 0):
        dz[p, i] = got['dvec_part'][lay.wave_id(lay.chunk_of(p), i // 64, (i % 64) // 16), 0]
    return dz


def model_of(case, chunks):
    """The exact reference and the bounds of one case, computed once: (X, exact records, bounds, per-term bounds, layout)."""
    X, exact, lay = D.run(case, chunks, scheme=False)
    bnd, E = D.record_bounds(case, X, lay)
    return X, exact, bnd, E, lay


def ratios_of(got, case, model, kind):
    """Worst error / bound per observable of one launch; `single`: also the backward half on the kernel's own dz2 ('x|dz2')."""
    X, exact, bnd, E, lay = model
    r = D.ratios(got, exact, bnd, X)
    if kind == 'single' and 'dvec_part' in got:
        Y = D.condition(case, X, given_dz2(got, case, lay))
        bg, _ = D.record_bounds(case, Y, lay, given=True)
        r.update({k + '|dz2': v for k, v in D.ratios(got, D.records(Y, lay, scheme=False), bg, None, names=D.GIVEN).items()})
    return r


def explain_dw2_given(got, case, model):
    """The worst dW2|dz2 entry of a `single` launch with the parts of its bound (what a failure message shows)."""
    X, _, _, _, lay = model
    Y = D.condition(case, X, given_dz2(got, case, lay))
    bg, E = D.record_bounds(case, Y, lay, given=True)
    ref = D.records(Y, lay, scheme=False)['dW2_part']
    err = np.abs(got['dW2_part'].astype(np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bg['dW2_part'] > 0, err / bg['dW2_part'], 0.0)
    wid, n, k = (int(v) for v in np.unravel_index(np.argmax(r), r.shape))
    p, i = next((int(p), int(i)) for p, i in np.argwhere(np.asarray(case['mask']) != 0)
                if lay.wave_id(lay.chunk_of(p), i // 64, (i % 64) // 16) == wid)
    dz, h = Y['dz2'][p, i, n], X['h1'][p, i, k]
    return dict(wave=wid, n=n, k=k, p=p, i=i, ratio=float(r[wid, n, k]), err=float(err[wid, n, k]), bound=float(bg['dW2_part'][wid, n, k]),
                got=float(got['dW2_part'][wid, n, k]), ref=float(ref[wid, n, k]), dz2=float(dz), h1=float(h), z1=float(X['z1'][p, i, k]),
                rep_dz=float(E['rep_dz'][p, i, n]), E_h1=float(E['h1'][p, i, k]), rep_h=float(E['rep_h'][p, i, k]),
                dzl=float(E['dzl'][p, i, n]), hl=float(E['hl'][p, i, k]), product_in_u=float(abs(dz * h) / D.U_),
                err_in_u_of_product=float(err[wid, n, k] / max(abs(dz * h) * D.U_, 1e-300)))


def worse(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def report(part, cls, worst, grade=None, **extra):
    """gpu_common.record, kind 'decoder_cells': per observable the worst error / bound; per contraction the bound over the plain fp32
    bound (median, 95th percentile: decoder_model.fp32_grade) where `grade` is given."""
    for k, v in sorted(worst.items()):
        record('decoder_cells', v, 1.0, part=part, **{'class': cls}, observable=k, ratio=v, **extra)
    for k, (med, p95) in sorted((grade or {}).items()):
        record('decoder_cells', p95, part=part, **{'class': cls}, observable='bound/fp32 ' + k, median=med, p95=p95, **extra)
    print(part, cls, {k: float(f'{v:.3g}') for k, v in worst.items()}, {k: (float(f'{a:.3g}'), float(f'{b:.3g}')) for k, (a, b) in (grade or {}).items()})
