"""What the host-side tests of the row formats (sign rows, tile rows, tile rows under a caller-supplied posterior, the launch decision)
share, once each: a descriptor of the headline shape, the call of an export on NULL pointers, and the small host matrix the deciders
of vibo_amd.ops are driven with.  A plain module: it needs neither the library nor a device."""
import ctypes

import torch

from vibo_amd import _lib


def desc(B=1_000_000, I=1000, A=8, irt=2, mask=_lib.MASK_SIGN, posterior=_lib.POSTERIOR_UNCONDITIONAL, n_flows=0, flags=0, grad=1,
         stride=None):
    d = _lib.ViboDesc()
    d.abi_version = _lib.ABI_VERSION
    d.num_person, d.num_item, d.ability_dim, d.irt_model = B, I, A, irt
    d.posterior, d.n_flows, d.flags, d.want_grad = posterior, n_flows, flags, grad
    d.reg_mode = _lib.REG_SAMPLED if n_flows else _lib.REG_KL
    d.mask_dtype = mask
    d.response_row_stride = d.mask_row_stride = ((I + 3) & ~3) if stride is None else stride
    return d


def _null_call(fn, d):
    args = []
    for t in fn.argtypes[1:]:
        args.append(None if t is ctypes.c_void_p or isinstance(t, type(ctypes.POINTER(_lib.ViboDesc))) else (64 if t is ctypes.c_int else 0))
    return fn(ctypes.byref(d), *args)


def matrix(P=12, I=8, seed=0, consistent=True):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(P, I, generator=g) > 0.2
    resp = torch.where(mask, (torch.rand(P, I, generator=g) < 0.5).float(), torch.tensor(-1.0))
    if not consistent:
        resp[3, 4], mask[3, 4] = 1.0, False
    return resp, mask
