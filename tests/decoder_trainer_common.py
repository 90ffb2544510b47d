"""What the FusedDecoderTrainer tests share (test_gpu_decoder_trainer.py, test_decoder_trainer[_cond]_host.py): the problems and models of
either posterior, the fp64 oracle trajectory with its exclusion rule, the trainer-state comparison, and the code-object notes of an
in-tree object (test_capi_symbols.py reads them too)."""
import glob
import os
import re
import subprocess
import tempfile

import pytest
import torch

from gpu_common import CLS, dev, simulated          # (CLS: the host-side tests import it from here)
from oracle import vibo_oracle as O
from vibo_amd import _lib, ops
from vibo_amd.torch_core import vibo as cli

TOL_ADAM1, TOL_ADAM3 = 2e-4, 5e-4                       # with gpu_common.TOL_ELBO: test_golden_adam_trajectory_through_the_fused_trainers' bounds
# Adam normalises the step, so an entry whose gradient is at rounding level moves by a full +-lr either way: entries whose gradient
# is below EXCLUDE_BELOW of the tensor's max-abs in any step are left out of a comparison, at most EXCLUDE_CAP of any tensor.
EXCLUDE_BELOW, EXCLUDE_CAP = 1e-4, 0.02


# ---------------------------------------------------------------------------
# problems and the fp64 oracle
# ---------------------------------------------------------------------------
# The unconditional posterior.  (decoder, IRT, A, B, I, missing, hidden, drop_missing, seed).  The seeds were picked on the CPU with oracle_trajectory() below
# (`python tests/test_gpu_decoder_trainer.py` prints the figures): seeds 1, 2, ... were tried per case until the float64
# gradients left at most 1.5 % of any tensor under the exclusion threshold over the three steps -- inside the 2 % cap with room
# for the fp32 gradients of the module-step test, which applies the same rule to the same problems.  Largest excluded share of
# any tensor with the seeds below: 1.0 %, 1.3 %, 1.1 %, 1.5 %, 1.3 %.
ORACLE_CASES = [('link', 3, 1, 33, 95, 0.3, 64, False, 1),
                ('deep', 2, 8, 300, 130, 0.1, 64, False, 2),
                ('residual', 1, 3, 77, 200, 0.2, 64, True, 8),
                ('deep', 2, 2, 64, 64, 0.0, 32, False, 5),
                ('residual', 3, 12, 40, 260, 0.1, 48, False, 9)]
# The conditional posterior.  (decoder, IRT, A, B, I, missing, hidden, drop_missing, seed).  The inputs were picked on the CPU with oracle_trajectory() below
# (`python tests/test_gpu_decoder_trainer.py` prints the figures) so that the float64 gradients leave at most 1.5 % of any
# tensor under the exclusion threshold over the three steps -- inside the 2 % cap with room for the fp32 gradients of the
# module-step test, which applies the same rule to the same problems.  The conditional table's wide last layer and the item
# log-variances have many near-zero gradients at 8 and more ability dimensions: the unconditional file's shapes at A = 8 / 12
# (130 / 260 items) left 3.5-50 % out with seeds 1-12, with 300-600 persons and missing fractions 0-0.1 still 3.5-51 %; at 30
# items (not a multiple of 4; 60 table rows: four tiles, the last one ragged) and 100 persons (seven person tiles, the last one
# ragged) seeds 1, 2, ... reached the bound at seed 6 (A = 8) and seed 15 (A = 12).  Largest excluded share of any tensor with
# the inputs below: 0.70 %, 1.40 %, 1.04 %, 1.39 %, 0.87 %.
COND_ORACLE_CASES = [('link', 3, 1, 33, 95, 0.3, 64, False, 10),
                     ('residual', 1, 3, 77, 200, 0.2, 64, True, 4),
                     ('deep', 2, 2, 64, 64, 0.0, 32, False, 2),
                     ('deep', 2, 8, 100, 30, 0.1, 64, False, 6),
                     ('residual', 3, 12, 100, 30, 0.1, 48, False, 15)]


def make_problem(conditional, gen, irt, A, B, I, missing, H, drop, seed):
    resp, mask, g = simulated(irt, B, I, A, missing, seed)
    D = O.item_feat_dim(irt, A)
    eps_item = torch.randn(3, I, D, generator=g)
    eps_ab = torch.randn(3, B, A, generator=g)
    torch.manual_seed(seed)
    model = CLS[irt](A, I, hidden_dim=H, ability_merge='product', generative_model=gen, replace_missing_with_prior=not drop,
                     conditional_posterior=conditional)
    return model, resp, mask, eps_item, eps_ab


def keep_entries(keep, grads):
    """The exclusion rule: drop from `keep` (name -> bool tensor) what this step's gradients (name -> tensor) leave at rounding level."""
    for k, g in grads.items():
        keep[k] &= g.abs() >= EXCLUDE_BELOW * g.abs().max()


def oracle_trajectory(conditional, model, resp, mask, eps_item, eps_ab, gen, irt, A, drop, beta=1.0):
    """Three float64 torch.optim.Adam steps (lr 5e-3) on the oracle's gradients.  Returns the parameters after steps 1 and 3, the
    first loss, and per tensor the entries to compare (keep_entries on the float64 gradients of every step)."""
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(list(params.values()), lr=5e-3)
    keep = {k: torch.ones_like(v, dtype=torch.bool) for k, v in params.items()}
    after, loss0 = {}, None
    for step in range(3):
        out, grads = O.elbo_loss_and_grads({k: v.detach() for k, v in params.items()}, resp.double(), mask, eps_item[step].double(),
                                           eps_ab[step].double(), irt_model=irt, ability_dim=A, replace_missing_with_prior=not drop,
                                           annealing_factor=beta, conditional_posterior=conditional, generative_model=gen)
        if step == 0:
            loss0 = float(out['loss'])
        for k, p in params.items():
            p.grad = grads[k].double()
        keep_entries(keep, {k: grads[k] for k in params})
        opt.step()
        if step in (0, 2):
            after[step + 1] = {k: v.detach().clone() for k, v in params.items()}
    return after, loss0, keep


_ORACLE = {}


def oracle_of(conditional, case):
    """The float64 trajectory of a case, computed once and shared (never written to)."""
    if (conditional, case) not in _ORACLE:
        gen, irt, A, B, I, missing, H, drop, seed = case
        model, resp, mask, eps_item, eps_ab = make_problem(conditional, *case)
        _ORACLE[conditional, case] = oracle_trajectory(conditional, model, resp, mask, eps_item, eps_ab, gen, irt, A, drop)
    return _ORACLE[conditional, case]


def compare_kept(state, want, keep, tol, what):
    for k, v in want.items():
        dropped = 1.0 - float(keep[k].float().mean())
        assert dropped <= EXCLUDE_CAP, (k, dropped)
        err = float(((state[k].double().cpu() - v.double().cpu()).abs() * keep[k]).max())
        print(what, k, f'err {err:.3e}', f'excluded {dropped:.4f}')
        assert err < tol, (what, k, err)


def print_excluded_shares(conditional, cases):
    """Input selection for a list of oracle cases (CPU only): the largest share of any tensor the exclusion rule would leave out."""
    for case in cases:
        _, _, keep = oracle_of(conditional, case)
        worst = max((1.0 - float(v.float().mean()), k) for k, v in keep.items())
        print('conditional' if conditional else 'unconditional', case, 'largest excluded share %.4f (%s)' % worst,
              'ok' if worst[0] <= EXCLUDE_CAP else 'TRY OTHER INPUTS')


# ---------------------------------------------------------------------------
# resident matrices and the trainer's state
# ---------------------------------------------------------------------------
def resident(conditional, gen, irt, A, P, I, H=64, missing=0.15, seed=7, codes=False, drop=False):
    d = dev()
    resp, mask, g = simulated(irt, P, I, A, missing, seed)
    resp, mask = ops.pad_rows(resp.to(d), mask.bool().to(d))
    if codes:
        resp, mask = ops.pack_cell_codes(resp, mask), None
    torch.manual_seed(seed)
    model = CLS[irt](A, I, hidden_dim=H, ability_merge='product', generative_model=gen, conditional_posterior=conditional,
                     replace_missing_with_prior=not drop).to(d)
    return model, resp, mask, g


def state_of(model, tr):
    return ({k: v.clone() for k, v in model.state_dict().items()}, tr.par_m.clone(), tr.par_v.clone(), tr.item_m.clone(), tr.item_v.clone())


def assert_same_state(s0, s1):
    for k in s0[0]:
        assert torch.equal(s0[0][k], s1[0][k]), k
    for a, b in zip(s0[1:], s1[1:]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# host side: descriptors, models, CLI arguments, code-object notes
# ---------------------------------------------------------------------------
def desc(irt, A, I=20, B=16, conditional=False, n_flows=0, mask=_lib.MASK_U8):
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A, conditional=conditional, n_flows=n_flows)
    return ops._make_desc(spec, B, I, mask, _lib.REG_SAMPLED if n_flows else _lib.REG_KL, True, I, I)


def _model(gen='deep', merge='product', cond=False, flows=0, H=64, irt=2, A=2):
    return CLS[irt](A, 12, hidden_dim=H, ability_merge=merge, conditional_posterior=cond, generative_model=gen, n_norm_flows=flows)


def _args(argv):
    return cli.finalize_args(cli.build_parser().parse_args(argv))


BUILD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'variational-item-response-theory-public_amd', 'csrc', 'build')
LLVM = '/opt/rocm/lib/llvm/bin'


def built_objects(*patterns):
    """The in-tree objects of these names; skips the calling test when the build directory or the LLVM tools are not there."""
    objs = [o for pat in patterns for o in sorted(glob.glob(os.path.join(BUILD_DIR, pat)))]
    if not objs or not os.path.exists(os.path.join(LLVM, 'llvm-readelf')):
        pytest.skip('no in-tree objects / LLVM tools')
    return objs


def kernel_notes(obj):
    """{kernel symbol: (vgpr_spill_count, private_segment_fixed_size)} from the gfx950 code object's notes of an in-tree object."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, 'fat.bin'), os.path.join(tmp, 'dev.co')
        subprocess.run([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, obj], check=True)
        subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                        '--input=' + fat, '--output=' + co, '--unbundle'], check=True)
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], check=True, capture_output=True, text=True).stdout
    res = {}
    for blk in notes.split('  - .agpr_count:')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        res[name] = (int(re.search(r'\.vgpr_spill_count:\s+(\d+)', blk).group(1)),
                     int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk).group(1)))
    return res
