"""What the GPU tests share, once each: the device, the seeded random ELBO problems, the one launch of the ELBO kernel, the
comparison with the fp64 table oracle and its tolerances, the VIBO_TOL_RECORD writer, the kernel-pin fixture, twin trainers, the
native noise at a counter of the test's own, and the float64 statement of the MLP decoder.  A plain module (tools/ import it too), importable without a GPU: only calling dev() needs one."""
import copy
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import vibo_oracle as O
from vibo_amd import _lib, ops
from vibo_amd.torch_core.models import VIBO_1PL, VIBO_2PL, VIBO_3PL
from vibo_amd.trainer import FusedTrainer

CLS = {1: VIBO_1PL, 2: VIBO_2PL, 3: VIBO_3PL}

# Tolerances (fp32).  ELBO: <= 1e-4 relative (north_star).  Gradients: fractions of the tensor's max-abs against
# the fp64 analytic oracle; section 8c asks for <= 1e-4, TOL_GRAD is that bound and the default everywhere.  Named wider bands exist only
# where the fp64 oracle cannot arbitrate to 1e-4, each with the reason and the maximum measured on the GPU beside it (VIBO_TOL_RECORD=path
# appends every observed error to a JSON-lines file: record() below).
TOL_ELBO = 1e-4
TOL_GRAD = 1e-4


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


# ---------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------
def simulated(irt, P, I, A, missing, seed):
    """-> (resp, mask, g): O.simulate_responses from a host generator seeded with `seed`; the caller's own draws go on from `g`."""
    g = torch.Generator().manual_seed(seed)
    resp, mask = O.simulate_responses(irt, P, I, A, generator=g, missing_frac=missing)
    return resp, mask, g


def random_problem(irt, A, B, I, missing, seed, cond=False, scale=1.0, table_scale=0.7, n_flows=None):
    """Host tensors (resp, mask, table, item, eps), drawn in this order from one generator.  With n_flows given (0 included) a sixth
    entry follows: the planar-flow parameters drawn after eps, None without flows."""
    resp, mask, g = simulated(irt, B, I, A, missing, seed)
    D = O.item_feat_dim(irt, A)
    table = torch.randn((2, I, 2 * A) if cond else (2, 2 * A), generator=g) * table_scale
    item = torch.randn(I, D, generator=g) * scale
    eps = torch.randn(B, A, generator=g)
    if n_flows is None:
        return resp, mask, table, item, eps
    return resp, mask, table, item, eps, (torch.randn(n_flows, 2 * A + 1, generator=g) * 0.5 if n_flows else None)


def device_problem(irt, A, P, I, missing, seed, cond):
    """A simulated response matrix built on the GPU in person slices (the full-size cases do not fit the host-side helper's
    temporaries): responses from the model's own link (models.py:729-766), `missing` of the cells unobserved."""
    d = dev()
    g = torch.Generator(device=d).manual_seed(seed)
    D = O.item_feat_dim(irt, A)
    theta = torch.randn(P, A, device=d, generator=g)
    item_true = torch.randn(I, D, device=d, generator=g)
    resp = torch.empty(P, I, device=d)
    mask = torch.empty(P, I, dtype=torch.bool, device=d)
    step = max(1, 100_000_000 // I)
    for s0 in range(0, P, step):
        sl = slice(s0, min(P, s0 + step))
        if irt == 1:
            logit = theta[sl].sum(1, keepdim=True) + item_true[:, 0]
        else:
            logit = -(theta[sl] @ item_true[:, :A].t()) + item_true[:, A]
        probs = torch.sigmoid(logit)
        if irt == 3:
            gs = torch.sigmoid(item_true[:, A + 1])
            probs = gs + (1 - gs) * probs
        resp[sl] = torch.bernoulli(probs, generator=g)
        mask[sl] = torch.rand(probs.shape, device=d, generator=g) >= missing
        del logit, probs
    table = (torch.randn((2, I, 2 * A) if cond else (2, 2 * A), device=d, generator=g) * 0.5).contiguous()
    item = torch.randn(I, D, device=d, generator=g)
    eps = torch.randn(P, A, device=d, generator=g)
    return resp, mask, table, item, eps


def coin_flip_rows(P, I, A, seed):
    """Rows that need no link, drawn on the GPU: fair-coin responses, 10 % missing, an unconditional 2PL table and items.
    -> (spec, resp, mask, table, item, g); the caller's own draws (noise, a row permutation) go on from `g`."""
    d = dev()
    g = torch.Generator(device=d).manual_seed(seed)
    resp = (torch.rand(P, I, device=d, generator=g) < 0.5).float()
    mask = torch.rand(P, I, device=d, generator=g) >= 0.1
    table = torch.randn(2, 2 * A, device=d, generator=g) * 0.5
    item = torch.randn(I, A + 1, device=d, generator=g)
    return ops.ElboSpec(irt_model=2, ability_dim=A), resp, mask, table, item, g


def scattered_rows(resp, mask, n_total):
    """The minibatch (host tensors) at random places of a resident matrix of n_total rows, decoys around it.
    -> (big_resp, big_mask, where): host tensors; the generator is seeded with the minibatch's cell count."""
    B, I = resp.shape
    g = torch.Generator().manual_seed(B * I)
    big_r = (torch.rand(n_total, I, generator=g) < 0.5).float()
    big_m = torch.rand(n_total, I, generator=g) < 0.8
    where = torch.randperm(n_total, generator=g)[:B]
    big_r[where], big_m[where] = resp, mask.bool()
    return big_r, big_m, where


# ---------------------------------------------------------------------------
# the launch
# ---------------------------------------------------------------------------
def launch_elbo(spec, resp, mask, table, item, eps, *, reg_mode=_lib.REG_KL, mask_dtype=torch.bool, row_index=None, want_grad=True,
                keep_int64=False, pad=False, codes=False, flow=None, kernel=None):
    """The one way a test calls the ELBO kernel on tensors of its own (host or device): ops._hip_launch_elbo, then
    torch.cuda.synchronize().  Rows as they are (the mask as `mask_dtype`; keep_int64: ops.prepare_mask), with `pad` their strides
    padded to 16 bytes as the CLI's resident splits are (ops.pad_rows), with `codes` as 1-byte cell codes.  `kernel`: the name the
    planner has to give this call (ops.plan_kernel), asserted before the launch."""
    d = dev()
    r, m = resp.to(d), (mask.to(d).to(mask_dtype) if mask is not None else None)
    if pad:
        r, m = ops.pad_rows(r, m)
    if codes:
        r, m = ops.pack_cell_codes(r, m), None
    r, m, code = ops.prepare_rows(r, m, keep_int64=keep_int64)
    ri = row_index.to(d) if row_index is not None else None
    B = int(ri.numel()) if ri is not None else r.shape[0]
    if kernel is not None:
        assert ops.plan_kernel(spec, B, r.shape[1], code, want_grad) == kernel, 'the planner did not pick ' + kernel
    raw = ops._hip_launch_elbo(spec, r, m, code, ri, table.to(d).contiguous(), item.to(d).contiguous(), eps.to(d).contiguous(),
                               flow.to(d).contiguous() if flow is not None else None, reg_mode, want_grad, B)
    torch.cuda.synchronize()
    return raw


# ---------------------------------------------------------------------------
# the record of observed errors, and the comparison with the fp64 table oracle
# ---------------------------------------------------------------------------
def recording():
    return bool(os.environ.get('VIBO_TOL_RECORD'))


def record(kind, err, tol=None, **extra):
    """VIBO_TOL_RECORD=path: append {'kind', 'err', 'tol' (where given), **extra, 'test'} to that file as one JSON line.  The only
    reader of the variable and the only writer of the file; it always returns, so no caller's assert depends on it."""
    if recording():
        entry = {'kind': kind, 'err': float(err), **({} if tol is None else {'tol': float(tol)}), **extra,
                 'test': os.environ.get('PYTEST_CURRENT_TEST', '')}
        with open(os.environ['VIBO_TOL_RECORD'], 'a') as f:
            f.write(json.dumps(entry) + '\n')


def check(kind, err, tol):
    record(kind, err, tol)
    # record, then assert
    assert err < tol, (kind, err, tol)


def compare_raw(raw, ref, item_shape, want_grad=True, tol=TOL_GRAD):
    sc = raw.scalars.cpu()
    assert rel_err(sc[_lib.S_LL], ref['ll']) < 2e-5
    assert abs(float(sc[_lib.S_REG]) - float(ref['reg'])) < 2e-5 * max(1.0, abs(float(ref['reg'])))
    assert abs(float(sc[_lib.S_KL]) - float(ref['kl_ability'])) < 2e-5 * max(1.0, abs(float(ref['kl_ability'])))
    assert abs(float(sc[_lib.S_LOGQ0]) - float(ref['logq0'])) < 2e-5 * max(1.0, abs(float(ref['logq0'])))
    assert abs(float(sc[_lib.S_LOGP]) - float(ref['logp'])) < 2e-5 * max(1.0, abs(float(ref['logp'])))
    for k, t in (('ability_mu', raw.ability_mu), ('ability_logvar', raw.ability_logvar), ('ability', raw.ability)):
        assert (t.cpu() - ref[k].float()).abs().max() < 2e-5 * max(1.0, float(ref[k].abs().max())), k
    if want_grad:
        for s in range(2):
            scale = float(ref['g_table'][s].abs().max())
            if scale > 0:
                check(f'g_table[{s}]', rel_err(raw.grad_table(s).cpu(), ref['g_table'][s]), tol)
            else:
                assert float(raw.grad_table(s).abs().max()) < 1e-6
        check('g_item', rel_err(raw.grad_item(item_shape).cpu(), ref['g_item']), tol)


# ---------------------------------------------------------------------------
# the kernel pin
# ---------------------------------------------------------------------------
def about_the_conditional_posterior(request):
    cs = getattr(request.node, 'callspec', None)
    params = cs.params if cs is not None else {}
    return 'cond' in request.node.name.lower() or bool(params.get('cond')) or 'cond' in str(params.get('golden', ''))


def kernel_choice_fixture(pins, ids, about_cond=about_the_conditional_posterior):
    """-> an autouse fixture that runs every test of the module that binds it once per entry of `pins` (vibo_desc.flags, through
    ops.DESC_FLAGS: the library reads no environment variable).  A pin with VIBO_FLAG_COND_THREE_PASS only differs for the
    conditional posterior: tests that are not `about_cond(request)` skip it."""
    @pytest.fixture(autouse=True, params=pins, ids=ids)
    def row_split_kernel_choice(request, monkeypatch):
        if request.param & _lib.FLAG_COND_THREE_PASS and not about_cond(request):
            pytest.skip('the three-pass pin only differs for the conditional posterior')
        monkeypatch.setattr(ops, 'DESC_FLAGS', request.param)
    return row_split_kernel_choice


# ---------------------------------------------------------------------------
# twin trainers
# ---------------------------------------------------------------------------
def twin_trainers(cls, A, I, model_seed, kw_a, kw_b=None, **model_kw):
    """-> (m_a, m_b, t_a, t_b): a model built under torch.manual_seed(model_seed) on the GPU, its deep copy, and a FusedTrainer
    at lr 5e-3 on each (kw_b: the second trainer's keywords where they differ from the first's)."""
    torch.manual_seed(model_seed)
    m_a = cls(A, I, **{'ability_merge': 'product', **model_kw}).to(dev())
    m_b = copy.deepcopy(m_a)
    return m_a, m_b, FusedTrainer(m_a, lr=5e-3, **kw_a), FusedTrainer(m_b, lr=5e-3, **(kw_a if kw_b is None else kw_b))


def assert_same_parameters(m_a, m_b):
    for (k, a), (_, b) in zip(m_a.state_dict().items(), m_b.state_dict().items()):
        assert torch.equal(a, b), (k, float((a - b).abs().max()))


# ---------------------------------------------------------------------------
# the native noise at a counter of the test's own (test_gpu_noise.py)
# ---------------------------------------------------------------------------
def noise_counter(step):
    """The int32 device word vibo_fill_normal reads its step from, holding `step` (as uint32 bits: 2^31 ... 2^32 - 1 wrap)."""
    step = int(step) & 0xFFFFFFFF
    return torch.tensor([step - (1 << 32) if step >= 1 << 31 else step], dtype=torch.int32, device=dev())


def fill_normal(n, seed, counter, stream_id, out=None):
    """vibo_fill_normal(out, n, seed, counter, stream_id) on torch's current stream -> out: a fresh float32 tensor [n], or the
    caller's (a contiguous float32 view of at least n entries, wherever it starts)."""
    if out is None:
        out = torch.empty(n, device=counter.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n and counter.dtype == torch.int32
    ops._call('vibo_fill_normal', ops._ptr(out), n, int(seed), ops._ptr(counter), int(stream_id), ops._stream(counter.device))
    return out


# ---------------------------------------------------------------------------
# the MLP decoder in float64 (test_gpu_decoder.py, tools/fuzz_decoder.py)
# ---------------------------------------------------------------------------
EPS32 = 1.1920928955078125e-07


def torch_reference(resp, mask, U, V, W2, b2, w3, b3, logit, w1, guess, resid):
    """[B, I, 64] the slow way (float64)."""
    z1 = V.unsqueeze(1) + (U.unsqueeze(0) if U is not None else 0.0)
    if w1 is not None:
        z1 = z1 + logit.unsqueeze(2) * w1
    h2 = F.elu(F.elu(z1) @ W2.t() + b2)
    o = h2 @ w3 + b3
    if resid:
        o = o + resid * logit
    p = torch.sigmoid(o)
    if guess is not None:
        p = guess + (1 - guess) * p
    pc = p.clamp(EPS32, 1 - EPS32)                       # torch.distributions.Bernoulli(probs=...) clamp (utils.py:46-49)
    ll = torch.where(resp > 0.5, pc.log(), torch.log1p(-pc))
    if mask is not None:
        ll = ll * mask
    return ll.sum(), p


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
