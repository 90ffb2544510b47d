"""CPU side of tests/test_gpu_flow_batches.py: the person-sliced table oracle equals the unsliced one; the restated planner grids give
the figures worked out by hand from vibo_planner.hip at 256 compute units; every case of the table is admitted -- the oracle in
float32 stays within a quarter of each bound of the GPU file, and every watched batch's own contribution to the flow gradients is at
least ten times the tolerance that has to notice its loss."""
import pytest
import torch

import flow_batches_common as Fb
from gpu_common import TOL_GRAD, random_problem
from oracle import vibo_table_ref as T

CUS = 256


def distinct_problems():
    seen, out = set(), []
    for c in Fb.CASES:
        k = Fb.problem_key(c, CUS)
        if k not in seen:
            seen.add(k)
            # (the training case of a problem stands for it where there is one: CASES lists it before its forward-only twin)
            out.append(c)
    return out


def close(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize('rows_per_slice', [6, 12, 7, 10, 1, 36, 50])          # 6, 12, 1, 36 divide B; 7, 10 do not; 50: one slice
@pytest.mark.parametrize('kind', ['uncond', 'cond', 'given'])
def test_sliced_oracle_equals_the_unsliced_one(kind, rows_per_slice):
    irt, A, B, I = 3, 3, 36, 40
    resp, mask, table, item, eps = random_problem(irt, A, B, I, 0.2, seed=5, cond=kind == 'cond')
    g = torch.Generator().manual_seed(9)
    if kind == 'given':
        table = torch.cat([torch.randn(B, A, generator=g) * 0.8, torch.randn(B, A, generator=g) * 0.5 - 1.0], dim=1)
    flows = Fb.flows_of(torch.randn(2, 2 * A + 1, generator=g) * 0.5, torch.float64)
    args = (table.double(), item.double(), resp.double(), mask, eps.double())
    kw = dict(irt_model=irt, ability_dim=A, conditional_posterior=kind == 'cond', mode='sampled', flow_uhat_w_b=flows,
              given_posterior=kind == 'given')
    whole = T.fused_elbo_ref(*args, **kw)
    cut = T.fused_elbo_ref_sliced(*args, rows_per_slice, keep_logit=True, **kw)
    assert set(cut) == set(whole) | {'g_flow_slices'}
    for k in whole:
        if k == 'g_table':
            assert cut[k][0].shape == ((B, 2 * A) if kind == 'given' else table.shape)
            for s in range(2):
                close(cut[k][s], whole[k][s])
        elif k == 'g_flow':
            close(T.flat_flow_grads(cut[k]), T.flat_flow_grads(whole[k]))
        else:
            close(cut[k], whole[k])
    n = -(-B // rows_per_slice)
    assert cut['g_flow_slices'].shape == (n, 2, 2, 2 * A + 1)
    close(cut['g_flow_slices'].sum(0), T.flat_flow_grads(whole['g_flow']))
    # a slice's entry is that slice's own gradient
    own = T.fused_elbo_ref(table.double()[:rows_per_slice] if kind == 'given' else args[0], args[1], args[2][:rows_per_slice],
                           mask[:rows_per_slice], args[4][:rows_per_slice], **kw)
    close(cut['g_flow_slices'][0], T.flat_flow_grads(own['g_flow']))
    forward = T.fused_elbo_ref_sliced(*args, rows_per_slice, want_grad=False, **kw)
    assert 'g_item' not in forward and 'logit' not in forward
    close(forward['reg'], whole['reg'])


def test_restated_grids_at_256_compute_units():
    """Against figures worked out by hand from the planner's source (msplit_blocks: CUs x max(1, 8 / waves), waves = ceil(width / 128),
    at most CUs / panels per panel; plan_row_split: clamp_grid(CUs, (8 or 12) / nq, B, 8) in integer division)."""
    assert Fb.matrix_grid(CUS, 1000, 1 << 20) == 256 and Fb.matrix_grid(CUS, 600, 1 << 20) == 256          # 8 and 5 waves: one per CU
    assert Fb.matrix_grid(CUS, 896, 1 << 20) == 256                                                          # 7 waves
    assert Fb.matrix_grid(CUS, 512, 1 << 20) == 512 and Fb.matrix_grid(CUS, 384, 1 << 20) == 512            # 4 and 3 waves: 8 / 3 = 2
    assert Fb.matrix_grid(CUS, 128, 1 << 20) == 2048
    assert Fb.matrix_grid(CUS, 2048, 1 << 20) == 128 and Fb.matrix_grid(CUS, 2500, 1 << 20) == 85           # 256 / 2, 256 / 3
    assert Fb.matrix_grid(CUS, 1000, 100) == 4                                                               # ceil(100 / 32)
    assert Fb.valu_grid(CUS, 1000, 1 << 20, 2, 3, True, False, False) == 512                                 # nq 4: 8 / 4 = 2 per CU
    assert Fb.valu_grid(CUS, 1000, 1 << 20, 2, 3, False, False, False) == 768                                # forward only: 12 / 4 = 3
    assert Fb.valu_grid(CUS, 516, 1 << 20, 1, 8, True, False, False) == 512                                  # nq 3: 8 / 3 = 2
    assert Fb.valu_grid(CUS, 512, 1 << 20, 2, 8, True, False, False) == 1024                                 # nq 2
    assert Fb.valu_grid(CUS, 256, 1 << 20, 3, 1, True, False, False) == 2048                                 # nq 1
    assert Fb.valu_grid(CUS, 256, 1 << 20, 3, 1, True, True, False) == 3072                                  # cell codes at width 2: 12
    assert Fb.valu_grid(CUS, 256, 1 << 20, 3, 4, True, True, False) == 2048                                  # ... not 3PL at width 4
    assert Fb.valu_grid(CUS, 256, 1 << 20, 2, 4, True, True, False) == 3072
    assert Fb.valu_grid(CUS, 256, 1 << 20, 2, 5, True, True, False) == 2048                                  # ... nor width 8
    assert Fb.valu_grid(CUS, 600, 1 << 20, 3, 2, True, False, True) == 512                                   # hooks: planned at nq 4
    assert Fb.valu_grid(CUS, 2500, 1 << 20, 2, 2, True, False, False) == 512                                 # panels: nq 4
    assert Fb.valu_grid(CUS, 1000, 100, 2, 3, True, False, False) == 13                                      # ceil(100 / 8)
    by_hand = {                                     # name: (G, persons)
        'M1': (256, 513 * 32 + 19), 'M2': (256, 257 * 32 + 19), 'M3': (256, 8243), 'M4': (256, 510 * 32 + 19), 'M5': (128, 129 * 32 + 19),
        'M6': (256, 8243), 'M7': (256, 8243), 'M8': (256, 8243), 'M9': (256, None), 'V1': (512, 513 * 8 + 7), 'V2': (3072, 3073 * 8 + 7),
        'V3': (512, 4111), 'V4': (512, 4111), 'V5': (512, 4111), 'V6': (512, 4111), 'V7': (768, 769 * 8 + 7)}
    assert by_hand['M1'][1] == 16435 and by_hand['M5'][1] == 4147 and by_hand['V2'][1] == 24591 and by_hand['V7'][1] == 6159
    for c in Fb.CASES:
        G, B = by_hand[c['name'][:2]]
        assert Fb.grid_of(c, CUS) == G, c['name']
        assert B is None or Fb.persons(c, CUS) == B, c['name']
        # the launch's own grid (clamped by the persons) is the full chip's: every case has more batches than workgroups
        assert Fb.grid_of(c, CUS, Fb.persons(c, CUS)) == G


def test_batch_patterns():
    """Every case gives workgroup 0 a second batch and ends on a partial one; M1 a third; M4 leaves its last workgroup with one."""
    for c in Fb.CASES:
        G, B, R = Fb.grid_of(c, CUS), Fb.persons(c, CUS), Fb.ROWS[c['engine']]
        n = Fb.ceil_div(B, R)
        assert B % R == Fb.TAIL[c['engine']] and len(Fb.batches_of(B, G, R)) >= 2, c['name']
        a, b = c['pattern']
        assert n == a * G + b + 1
        assert len(Fb.batches_of(B, G, R)) == (3 if a == 2 and b > 0 else 2)
        watched = Fb.watched_batches(B, G, R)
        assert G in watched and n - 1 in watched and 5 in watched and (2 * G in watched) == (n > 2 * G)
    m1, m4 = Fb.CASES[0], Fb.CASES[3]
    assert m1['name'].startswith('M1') and Fb.batches_of(16435, 256, 32) == [0, 256, 512] and Fb.batches_of(16435, 256, 32, 1) == [1, 257, 513]
    assert Fb.batches_of(16435, 256, 32, 2) == [2, 258]                      # three, three (the last one partial) and two
    assert m4['name'].startswith('M4') and Fb.batches_of(16339, 256, 32, 255) == [255] and Fb.batches_of(16339, 256, 32, 254) == [254, 510]
    # odd and even parity of the last batch among the workgroups of one launch
    assert {len(Fb.batches_of(8243, 256, 32, wg)) for wg in range(256)} == {1, 2}


@pytest.mark.parametrize('c', distinct_problems(), ids=Fb.case_id)
def test_case_is_admitted(c):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    p = Fb.problem(c, CUS)
    shares = Fb.float32_shares(p)
    assert max(shares.values()) <= Fb.F32_SHARE, {k: v for k, v in shares.items() if v > Fb.F32_SHARE}
    if c['want_grad']:
        whole, blocks = Fb.watched_shares(p, Fb.grid_of(c, CUS))
        assert len(whole) == 2 * len(Fb.watched_batches(p['B'], Fb.grid_of(c, CUS), Fb.ROWS[c['engine']]))
        assert min(whole.values()) >= Fb.WATCH_FACTOR * TOL_GRAD, whole
        assert min(blocks.values()) >= Fb.WATCH_FACTOR * TOL_GRAD, blocks          # ... and under the per-block normalisation
    if c['raw_flows'] is not None:
        psi = Fb.psi_of(p)
        assert float((psi < 0).double().mean()) >= Fb.PSI_NEGATIVE_SHARE and float(psi.abs().min()) >= Fb.PSI_FLOOR
    else:
        assert float(Fb.psi_of(p).min()) > 0                                      # flow_uhat keeps w.uhat >= -1
