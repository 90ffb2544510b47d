"""Planar flows inside the two row-split ELBO kernels, past one batch per workgroup: the case table of tests/test_gpu_flow_batches.py, the
restatement of the planner's grids it is built on, the seeded problems with their person-sliced fp64 oracle (cached: the CPU admission
test and the GPU file ask for the same ones), and the admission figures.  A plain module, importable without a GPU.

Both kernels hand batch bt to workgroup bt % G (vibo_msplit_kernel.hpp `for (; bt < n_batches; bt += G, par ^= 1)`,
vibo_split_kernel.hpp `bt += gridDim.x`): a launch of a G + b full batches and one partial batch gives workgroup 0 a + 1 batches.
The flow state carried over that loop (matrix kernel: tps / facc / lacc by batch parity; VALU kernel: SplitFlowAcc and the per-wave
log-det sum) is what the cases are about."""
import functools

import torch

from conftest import rel_err
from gpu_common import TOL_GRAD, random_problem, scattered_rows, simulated
from oracle import vibo_oracle as O
from oracle import vibo_table_ref as T
from vibo_amd import _lib

ROWS = {'matrix': 32, 'valu': 8}            # rows per batch: kMsRows, kSplitRows
TAIL = {'matrix': 19, 'valu': 7}            # the partial last batch (19: both halves of the matrix kernel's 32-row slot map)
KERNEL = {'matrix': _lib.KERNEL_NAMES[1], 'valu': _lib.KERNEL_NAMES[2]}
WATCH_FACTOR = 10.0                         # a watched batch's contribution >= WATCH_FACTOR * TOL_GRAD of the set's maximum
F32_SHARE = 0.25                            # the float32 oracle stays within this share of every bound (trainer_gradient_common's rule)
PSI_NEGATIVE_SHARE, PSI_FLOOR = 0.01, 0.05  # raw flow parameters: psi < 0 on this share of the (person, flow) pairs, min |psi|

# the bounds of the GPU file (gpu_common.compare_raw and test_general_kernel_vs_oracle), restated for the float32-oracle rule
TOL_SCALAR = 2e-5                           # S_LL: relative; S_REG, S_KL, S_LOGQ0, S_LOGP: of max(1, |ref|)
TOL_PERSON = 2e-5                           # ability_mu, ability_logvar, ability: of max(1, max|ref|)
TOL_FLOW_PERSON = 5e-5                      # ability_k, ability_ladj: absolute
TOL_LADJ_SUM = 1e-4                         # S_LADJ: of max(1, |ref|)


# ---------------------------------------------------------------------------
# the planner's grids, restated (vibo_planner.hip: msplit_blocks, plan_row_split, plan_panel_grids; vibo_planner.hpp: clamp_grid)
# ---------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def matrix_grid(cus, I, B):
    """Workgroups per panel of the matrix kernel's launch."""
    panels, width = ceil_div(I, 1024), min(I, 1024)
    g = min(cus * max(1, 8 // ceil_div(width, 128)), ceil_div(B, 32))
    return min(g, max(1, cus // panels)) if panels > 1 else g


def valu_grid(cus, I, B, irt, A, want_grad, codes, hooks):
    """Workgroups of a VALU-kernel launch.  hooks: the conditional and caller-supplied posteriors (planned at 4 waves, as the panels
    of more than 1024 items are)."""
    at = 2 if A <= 2 else 4 if A <= 4 else 8
    three_waves = codes and (at <= 2 or (at == 4 and irt <= 2))
    nq = 4 if hooks or I > 1024 else ceil_div(I, 256)
    return min(cus * ((8 if want_grad and not three_waves else 12) // nq), ceil_div(B, 8))


def grid_of(c, cus, B=1 << 30):
    if c['engine'] == 'matrix':
        return matrix_grid(cus, c['I'], B)
    return valu_grid(cus, c['I'], B, c['irt'], c['A'], c['want_grad'], c['rows'] == 'codes', c['post'] != 'uncond')


def persons(c, cus):
    """B = (a G + b) R + tail at the grid G of a full chip: a G + b full batches and the partial one."""
    a, b = c['pattern']
    return (a * grid_of(c, cus) + b) * ROWS[c['engine']] + TAIL[c['engine']]


def batches_of(B, G, R, wg=0):
    """The batches workgroup `wg` of G takes, in its order."""
    return list(range(wg, ceil_div(B, R), G))


def watched_batches(B, G, R):
    """Workgroup 0's second and third batch (where it has them), one batch of the first sweep, the partial last batch."""
    return sorted(set(batches_of(B, G, R)[1:3] + [min(5, G - 1), ceil_div(B, R) - 1]))


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def case(name, engine, irt, A, I, flows, pattern, seed, rows='fp32', post='uncond', drop=False, want_grad=True, raw_flows=None,
         missing=0.1, cond_flag=0):
    """pattern (a, b): see persons().  rows: 'fp32' | 'codes' | 'gathered'.  post: 'uncond' | 'cond' | 'given'.  raw_flows: the seed of
    flow parameters drawn raw (no flow_uhat), None: uhat built with T.flow_uhat."""
    pin = (_lib.FLAG_KERNEL_MATRIX if engine == 'matrix' else _lib.FLAG_KERNEL_VALU) | cond_flag
    return dict(name=name, engine=engine, irt=irt, A=A, I=I, flows=flows, pattern=pattern, seed=seed, rows=rows, post=post, drop=drop,
                want_grad=want_grad, raw_flows=raw_flows, missing=missing, pin=pin)


def forward_only(c, name):
    return dict(c, name=name, want_grad=False)


# G + 1 full batches and the partial one (workgroups 0 and 1 take two batches, the others one), 2 G + 1 (three and two), and
# 2 G - 2 (2 G - 1 batches in all: workgroup G - 1 has no second batch, workgroup G - 2 ends on the partial one)
G1, G2, G2M1 = (1, 1), (2, 1), (2, -2)
# Raw flow parameters (randn * 0.5, no flow_uhat, as test_general_kernel_vs_oracle draws them): the seeds at which one flow has
# w.u < -1 with every person's psi below zero and clear of it -- with thousands of persons a flow whose psi changes sign between
# persons also has persons next to the zero.  The first seeds from 1 upwards that meet both conditions of the CPU test on the fp64
# oracle (M1: psi < 0 on one flow of two, min |psi| 0.30; V3: on one flow of eight, 0.13)
RAW_SEED_M1, RAW_SEED_V3 = 135, 97
M1 = case('M1-matrix-8-waves-2pl-a8-1000-raw-flows', 'matrix', 2, 8, 1000, 2, G2, seed=1, raw_flows=RAW_SEED_M1)
M2 = case('M2-matrix-pinned-flow-addr-3pl-a2-1000', 'matrix', 3, 2, 1000, 4, G1, seed=2)
V1 = case('V1-valu-nq4-2pl-a3-1000', 'valu', 2, 3, 1000, 4, G1, seed=11)
CASES = [
    M1, M2,
    case('M3-matrix-5-waves-1pl-a4-600-codes', 'matrix', 1, 4, 600, 8, G1, seed=3, rows='codes', missing=0.0),
    case('M4-matrix-gathered-2pl-a3-896', 'matrix', 2, 3, 896, 2, G2M1, seed=4, rows='gathered'),
    case('M5-matrix-two-panels-2pl-a1-2048', 'matrix', 2, 1, 2048, 4, G1, seed=5, missing=0.2),
    case('M6-matrix-given-2pl-a4-1000', 'matrix', 2, 4, 1000, 2, G1, seed=6, post='given'),
    case('M7-matrix-cond-3pl-a1-1000', 'matrix', 3, 1, 1000, 2, G1, seed=7, post='cond', cond_flag=_lib.FLAG_COND_MATRIX),
    case('M8-matrix-drop-missing-2pl-a5-772', 'matrix', 2, 5, 772, 3, G1, seed=8, drop=True, missing=0.2),
    forward_only(M1, 'M9-matrix-forward-only-of-M1'), forward_only(M2, 'M9-matrix-forward-only-of-M2'),
    V1,
    # (forward only: with 3 072 workgroups an 8-row batch is 3e-4 of the flow gradients -- 2.8 x TOL_GRAD where admission asks for 10 --
    #  and no one-launch VALU shape under 513 items has fewer than 1 024: the gradients at nq 1 and 2 stay to the one-batch tests)
    case('V2-valu-nq1-3pl-a1-256-codes-forward-only', 'valu', 3, 1, 256, 2, G1, seed=12, rows='codes', want_grad=False),
    case('V3-valu-nq3-1pl-a8-516-gathered-raw-flows', 'valu', 1, 8, 516, 8, G1, seed=13, rows='gathered', raw_flows=RAW_SEED_V3),
    case('V4-valu-three-panels-2pl-a2-2500', 'valu', 2, 2, 2500, 2, G1, seed=14, missing=0.2),
    case('V5-valu-given-3pl-a2-600', 'valu', 3, 2, 600, 3, G1, seed=15, post='given'),
    case('V6-valu-cond-2pl-a4-600', 'valu', 2, 4, 600, 2, G1, seed=16, post='cond', cond_flag=_lib.FLAG_COND_VALU),
    forward_only(V1, 'V7-valu-forward-only-of-V1'),
]


def case_id(c):
    return c['name']


# ---------------------------------------------------------------------------
# problems and their oracle (cached per distinct problem: a forward-only case shares its training case's where the grids agree)
# ---------------------------------------------------------------------------
def flow_parameters(c):
    """[n_flows, 2A+1] float32 rows uhat | w | b."""
    A = c['A']
    if c['raw_flows'] is not None:
        return torch.randn(c['flows'], 2 * A + 1, generator=torch.Generator().manual_seed(c['raw_flows'])) * 0.5
    raw = torch.randn(c['flows'], 2 * A + 1, generator=torch.Generator().manual_seed(1000 + c['seed'])) * 0.7
    wv = raw[:, A:2 * A]
    raw[:, A:2 * A] = torch.sign(wv) * (0.4 + wv.abs()) / (A ** 0.5)        # (flow_uhat divides by |w|^2)
    return torch.stack([torch.cat([T.flow_uhat(f[:A], f[A:2 * A]), f[A:]]) for f in raw])


def oracle_kwargs(c):
    return dict(irt_model=c['irt'], ability_dim=c['A'], conditional_posterior=c['post'] == 'cond', replace_missing_with_prior=not c['drop'],
                mode='sampled', given_posterior=c['post'] == 'given')


def flows_of(flow, dtype):
    A = (flow.shape[1] - 1) // 2
    return [(f[:A].to(dtype), f[A:2 * A].to(dtype), f[2 * A:].to(dtype)) for f in flow]


def sliced_oracle(p, dtype):
    """The table oracle in `dtype` over the problem's persons in slices of one batch each: slice j of 'g_flow_slices' is batch j's own
    contribution."""
    c = p['case']
    return T.fused_elbo_ref_sliced(p['table'].to(dtype), p['item'].to(dtype), p['resp'].to(dtype), p['mask'], p['eps'].to(dtype),
                                   ROWS[c['engine']], flow_uhat_w_b=flows_of(p['flow'], dtype), want_grad=c['grads'], **oracle_kwargs(c))


def _base_key(c, cus):
    return tuple(c[k] for k in ('engine', 'irt', 'A', 'I', 'flows', 'seed', 'rows', 'post', 'drop', 'raw_flows', 'missing')) + (persons(c, cus),)


def problem_key(c, cus):
    """... and whether a training case asks for this problem (else its oracle stops after the forward)."""
    return _base_key(c, cus) + (any(o['want_grad'] and _base_key(o, cus) == _base_key(c, cus) for o in CASES),)


@functools.lru_cache(maxsize=None)
def _problem(key):
    engine, irt, A, I, flows, seed, rows, post, drop, raw_flows, missing, B, grads = key
    c = dict(engine=engine, irt=irt, A=A, I=I, flows=flows, seed=seed, rows=rows, post=post, drop=drop, raw_flows=raw_flows, grads=grads)
    if post == 'given':
        resp, mask, g = simulated(irt, B, I, A, missing, seed)
        table = torch.cat([torch.randn(B, A, generator=g) * 0.8, torch.randn(B, A, generator=g) * 0.5 - 1.0], dim=1)
        item = torch.randn(I, O.item_feat_dim(irt, A), generator=g) * 0.6
        eps = torch.randn(B, A, generator=g)
    else:
        resp, mask, table, item, eps = random_problem(irt, A, B, I, missing, seed, cond=post == 'cond')
    if drop:                                             # every row keeps an observation
        mask[:, 0] = 1
        resp[:, 0] = resp[:, 0].clamp(min=0)
    p = dict(case=c, B=B, resp=resp, mask=mask, table=table, item=item, eps=eps, flow=flow_parameters(c))
    if rows == 'gathered':
        p['big_resp'], p['big_mask'], p['where'] = scattered_rows(resp, mask, B + 997)
    p['ref'] = sliced_oracle(p, torch.float64)
    return p


def problem(c, cus):
    """Host tensors of the case at a chip of `cus` compute units, with 'ref': the float64 oracle in one-batch slices.  Never written."""
    return _problem(problem_key(c, cus))


def psi_of(p):
    """[B, n_flows] float64: 1 + (1 - tanh^2) w.uhat of every person and flow, from the oracle's sample."""
    z, out = p['ref']['ability'], []
    for uhat, w, b in flows_of(p['flow'], torch.float64):
        t = torch.tanh(z @ w + b)
        out.append(1.0 + (1.0 - t * t) * torch.dot(w, uhat))
        z = z + uhat.unsqueeze(0) * t.unsqueeze(1)
    return torch.stack(out, dim=1)


def flow_blocks(A):
    """The (name, slice) blocks of one flow's 2A+1 gradient entries."""
    return (('uhat', slice(0, A)), ('w', slice(A, 2 * A)), ('b', slice(2 * A, 2 * A + 1)))


def block_norms(ref, A):
    """[2, n_flows, 3]: per (set, flow, uhat | w | b) block, max over its entries of the sum over batches of |batch contribution|."""
    mass = ref['g_flow_slices'].abs().sum(0)                                   # [2, F, 2A+1]
    return torch.stack([mass[:, :, sl].amax(dim=2) for _, sl in flow_blocks(A)], dim=2)


def block_errors(got, ref, A):
    """[2, n_flows, 3]: max |got - ref| per block over the block's norm.  got: [2, n_flows, 2A+1]."""
    d = (got.double() - ref['g_flow_slices'].sum(0)).abs()
    return torch.stack([d[:, :, sl].amax(dim=2) for _, sl in flow_blocks(A)], dim=2) / block_norms(ref, A)


def flat_flow(ref):
    return T.flat_flow_grads(ref['g_flow'])


def float32_shares(p):
    """{quantity: distance of the float32 oracle from the float64 one / the GPU file's bound on that quantity}."""
    c, r64 = p['case'], p['ref']
    r32 = sliced_oracle(p, torch.float32)
    one = lambda k: max(1.0, abs(float(r64[k])))
    s = {'ll': rel_err(r32['ll'], r64['ll']) / TOL_SCALAR}
    for k in ('reg', 'kl_ability', 'logq0', 'logp'):
        s[k] = abs(float(r32[k]) - float(r64[k])) / one(k) / TOL_SCALAR
    s['ladj_sum'] = abs(float(r32['ladj_sum']) - float(r64['ladj_sum'])) / one('ladj_sum') / TOL_LADJ_SUM
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        s[k] = float((r32[k].double() - r64[k]).abs().max()) / max(1.0, float(r64[k].abs().max())) / TOL_PERSON
    for k in ('ability_k', 'ladj'):
        s[k] = float((r32[k].double() - r64[k]).abs().max()) / TOL_FLOW_PERSON
    if not c['grads']:
        return s
    for st in range(2):
        if float(r64['g_table'][st].abs().max()) > 0:
            s[f'g_table[{st}]'] = rel_err(r32['g_table'][st], r64['g_table'][st]) / TOL_GRAD
        s[f'g_flow[{st}]'] = rel_err(flat_flow(r32)[st], flat_flow(r64)[st]) / TOL_GRAD
    s['g_item'] = rel_err(r32['g_item'], r64['g_item']) / TOL_GRAD
    s['g_flow blocks'] = float(block_errors(flat_flow(r32), r64, c['A']).max()) / TOL_GRAD
    return s


def watched_shares(p, G):
    """{(batch, set): largest entry of the batch's own contribution to g_flow[set] / max |g_flow[set]|}, and the same with every block
    over its own norm (the largest block share of the batch)."""
    c, ref = p['case'], p['ref']
    total, norms = flat_flow(ref).abs(), block_norms(ref, c['A'])
    whole, blocks = {}, {}
    for bt in watched_batches(p['B'], G, ROWS[c['engine']]):
        part = ref['g_flow_slices'][bt].abs()
        for st in range(2):
            whole[(bt, st)] = float(part[st].max() / total[st].max())
            blocks[(bt, st)] = float(max((part[st][:, sl].amax(dim=1) / norms[st, :, k]).max() for k, (_, sl) in enumerate(flow_blocks(c['A']))))
    return whole, blocks
