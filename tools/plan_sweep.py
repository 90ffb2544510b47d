"""Every public answer of the planner (csrc/vibo_planner.hip) over a fixed sweep of descriptors, one line each: vibo_plan_kernel,
vibo_plan_cond_passes, vibo_workspace_bytes, vibo_train_step_supported, vibo_train_step_draws_noise, vibo_train_step_sample_optional
(rows in order / gathered; for a library from before that query: the rule it replaced, evaluated here) and vibo_multi_workspace_bytes
(1, 3 and 16 samples), plus the error string where vibo_plan_kernel refuses.  No launch, no GPU needed (without one the planner
assumes 256 compute units).  Two builds of the library plan alike exactly when their outputs are byte-identical:

    python tools/plan_sweep.py | sha256sum
    VIBO_HIP_LIB=/path/to/other/libvibo_hip.so python tools/plan_sweep.py | sha256sum

The sweep is the full factorial of num_item x ability_dim x posterior x mask_dtype x flags over every constant the planner compares
against, times `per_cell` seeded draws (without replacement) from persons x irt_model x row strides x want_grad x flows /
regulariser x missing_mode: 52 800 cells x 24 = 1 267 200 distinct descriptors by default."""
import argparse
import ctypes
import hashlib
import itertools
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'variational-item-response-theory-public_amd'))
from vibo_amd import _lib  # noqa: E402

ITEMS = (3, 4, 5, 64, 65, 128, 129, 144, 192, 255, 256, 304, 320, 512, 640, 896, 1000, 1023, 1024, 1025, 32767, 32768)
ABILITY_DIMS = (1, 2, 3, 4, 5, 8, 9, 16)
POSTERIORS = (_lib.POSTERIOR_UNCONDITIONAL, _lib.POSTERIOR_CONDITIONAL, _lib.POSTERIOR_GIVEN)
MASKS = (_lib.MASK_U8, _lib.MASK_I64, _lib.MASK_NONE, _lib.MASK_CODES, _lib.MASK_SIGN)
_SINGLE = (_lib.FLAG_KERNEL_VALU, _lib.FLAG_KERNEL_MATRIX, _lib.FLAG_NO_EMIT_CODES, _lib.FLAG_COND_VALU, _lib.FLAG_COND_MATRIX,
           _lib.FLAG_COND_THREE_PASS)
_REFUSED = (_lib.FLAG_KERNEL_VALU | _lib.FLAG_KERNEL_MATRIX, _lib.FLAG_COND_VALU | _lib.FLAG_COND_MATRIX)
FLAGS = (0,) + _SINGLE + tuple(a | b for a, b in itertools.combinations(_SINGLE, 2) if a | b not in _REFUSED)
PERSONS = (1, 8, 1024, 2048, 4096, 8192, 16384, 32768, 2**31 - 65536 - 1, 2**31 - 65536, 2**31 - 65536 + 1)
IRT = (1, 2, 3)
STRIDES = ('padded', 'unpadded', 'odd')
# (n_flows, reg_mode): flows need the sampled regulariser -- the last pair is refused by the descriptor check
FLOWS_REG = ((0, _lib.REG_KL), (0, _lib.REG_SAMPLED), (2, _lib.REG_SAMPLED), (2, _lib.REG_KL))
REST = tuple(itertools.product(PERSONS, IRT, STRIDES, (0, 1), FLOWS_REG, (_lib.MISSING_PRIOR, _lib.MISSING_DROP)))


def descriptors(per_cell=24, seed=0):
    """Yield the sweep's ViboDesc objects (one object, refilled: copy what you keep)."""
    rng = random.Random(seed)
    d = _lib.ViboDesc()
    d.abi_version = _lib.ABI_VERSION
    for items, dim, post, mask, flags in itertools.product(ITEMS, ABILITY_DIMS, POSTERIORS, MASKS, FLAGS):
        for k in rng.sample(range(len(REST)), per_cell):
            persons, irt, stride, grad, (flows, reg), missing = REST[k]
            d.num_person, d.num_item, d.ability_dim, d.irt_model = persons, items, dim, irt
            d.posterior, d.missing_mode, d.mask_dtype, d.reg_mode = post, missing, mask, reg
            d.n_flows, d.want_grad, d.flags = flows, grad, flags
            row = items if stride == 'unpadded' else ((items + 3) & ~3) | (1 if stride == 'odd' else 0)
            d.response_row_stride = d.mask_row_stride = row
            yield d


def answers(lib, d):
    """The planner's public answers for one descriptor, as the sweep prints them."""
    p = ctypes.byref(d)
    kernel = lib.vibo_plan_kernel(p)
    err = lib.vibo_last_error_string().decode() if kernel < 0 else ''
    noise = lib.vibo_train_step_draws_noise(p)
    if hasattr(lib, 'vibo_train_step_sample_optional'):
        lazy = [lib.vibo_train_step_sample_optional(p, gathered) for gathered in (0, 1)]
    else:      # a library from before the query: the rule of vibo_elbo_fwd_bwd_step_noise that it replaced
        lazy = [noise, int(noise and not (d.mask_dtype != _lib.MASK_CODES and (d.num_item + 127) // 128 < 8))]
    return (kernel, lib.vibo_plan_cond_passes(p), lib.vibo_workspace_bytes(p), lib.vibo_train_step_supported(p), noise, *lazy,
            lib.vibo_multi_workspace_bytes(p, 1), lib.vibo_multi_workspace_bytes(p, 3), lib.vibo_multi_workspace_bytes(p, 16), err)


def line(d, a):
    return ('B=%d I=%d A=%d irt=%d post=%d miss=%d mask=%d reg=%d flows=%d grad=%d stride=%d flags=%d -> '
            'kernel=%d cond=%d ws=%d step=%d noise=%d lazy=%d/%d multi=%d/%d/%d %s\n'
            % ((d.num_person, d.num_item, d.ability_dim, d.irt_model, d.posterior, d.missing_mode, d.mask_dtype, d.reg_mode, d.n_flows,
                d.want_grad, d.response_row_stride, d.flags) + a))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--per-cell', type=int, default=24, help='draws per factorial cell (default 24: 1 013 760 descriptors)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--digest', action='store_true', help='print only the descriptor count and the SHA-256 of the output')
    args = ap.parse_args()
    lib = ctypes.CDLL(_lib.LIB_PATH)        # (_lib.load() wants every export of the header: an older library lacks the newest)
    for name, restype, argtypes in _lib.PROTOTYPES:
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    sha, n = hashlib.sha256(), 0
    for d in descriptors(args.per_cell, args.seed):
        text = line(d, answers(lib, d))
        n += 1
        if args.digest:
            sha.update(text.encode())
        else:
            sys.stdout.write(text)
    if args.digest:
        print(n, sha.hexdigest())


if __name__ == '__main__':
    main()
