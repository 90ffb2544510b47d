"""What the tests of sparse response rows share, once each: the image's constants as include/vibo_hip_sparse_rows.h states them,
matrices with prescribed row and column lengths, the fp64 oracle on the densified rows, the CPU stand-in of the sparse launch, and the
person pass's grid rule.  A plain module: it needs neither the library nor a device."""
import re
import os

import torch

from oracle import vibo_table_ref as T
from vibo_amd import _lib, ops, sparse

HEADER = os.path.join(os.path.dirname(_lib.HEADER_PATH), 'vibo_hip_sparse_rows.h')
CHUNK = _lib.SPARSE_CHUNK


def header_constants():
    """{name: value} of the header's `#define VIBO_SPARSE_* <integer>` lines."""
    with open(HEADER) as f:
        return {k: int(v) for k, v in re.findall(r'^#define (VIBO_SPARSE_\w+) (\d+)', f.read(), flags=re.M)}


def person_waves(B):
    """Waves of the person pass for a call on B persons (THE GRID RULE of the header): 4 per workgroup."""
    return 4 * min(-(-B // _lib.SPARSE_ROWS_PER_BLOCK), _lib.SPARSE_MAX_BLOCKS)


def rows_of_wave(B, w):
    return len(range(w, B, person_waves(B)))


def matrix_with_row_lengths(lengths, I, seed):
    """(response fp32 with -1 at missing cells, mask bool) [len(lengths), I]: row r observes exactly lengths[r] cells at random items,
    answered right or wrong by a fair coin."""
    g = torch.Generator().manual_seed(seed)
    P = len(lengths)
    mask = torch.zeros(P, I, dtype=torch.bool)
    for r, n in enumerate(lengths):
        mask[r, torch.randperm(I, generator=g)[:n]] = True
    right = torch.rand(P, I, generator=g) < 0.5
    return torch.where(mask, right.float(), torch.tensor(-1.0)), mask


def matrix_with_column_lengths(lengths, P, seed):
    """The same by column: item i is answered by exactly lengths[i] persons."""
    r, m = matrix_with_row_lengths(lengths, P, seed)
    return r.t().contiguous(), m.t().contiguous()


def problem(irt, A, I, B, seed, scale=1.0):
    """(table [2, 2A], item [I, D], eps [B, A]) host tensors from one generator."""
    g = torch.Generator().manual_seed(seed)
    D = ops.item_feat_dim(irt, A)
    return torch.randn(2, 2 * A, generator=g) * 0.7, torch.randn(I, D, generator=g) * scale, torch.randn(B, A, generator=g)


def oracle(spec, table, item, resp, mask, eps, reg_mode=_lib.REG_KL, want_grad=True):
    """oracle.vibo_table_ref.fused_elbo_ref in fp64 on dense rows."""
    return T.fused_elbo_ref(table.double(), item.double(), resp.double(), mask, eps.double(), irt_model=spec.irt_model,
                            ability_dim=spec.ability_dim, replace_missing_with_prior=not spec.drop_missing,
                            mode='kl' if reg_mode == _lib.REG_KL else 'sampled', want_grad=want_grad)


def install_standin():
    """Swap the sparse entries of ops._BACKEND for a CPU stand-in that densifies the range and calls the fp32 oracle, as
    oracle/cpu_backend.install does for the dense entries.  -> restore()."""
    saved = {k: ops._BACKEND[k] for k in ('sparse_elbo', 'sparse_encode')}

    def cfg(spec, reg_mode):
        return dict(irt_model=spec.irt_model, ability_dim=spec.ability_dim, replace_missing_with_prior=not spec.drop_missing,
                    mode='kl' if reg_mode == _lib.REG_KL else 'sampled')

    def elbo(spec, rows, table, item, eps, reg_mode, want_grad):
        resp, mask = rows.to_dense()
        out = T.fused_elbo_ref(table, item, resp, mask, eps, want_grad=want_grad, **cfg(spec, reg_mode))
        n_table, n_item = table.numel(), item.numel()
        flat = torch.zeros(_lib.NUM_SCALARS + 2 * n_table + n_item, dtype=torch.float32)
        flat[_lib.S_LL], flat[_lib.S_REG] = out['ll'], out['reg']
        flat[_lib.S_KL], flat[_lib.S_LOGQ0], flat[_lib.S_LOGP] = out['kl_ability'], out['logq0'], out['logp']
        flat[_lib.S_NOBS] = float(mask.sum())
        raw = ops.RawElbo(flat=flat, n_table=n_table, n_item=n_item, n_flow=0, table_shape=tuple(table.shape),
                          ability_mu=out['ability_mu'], ability_logvar=out['ability_logvar'], ability=out['ability'],
                          ability_k=None, ability_ladj=None)
        if want_grad:
            raw.grad_table(0).copy_(out['g_table'][0])
            raw.grad_table(1).copy_(out['g_table'][1])
            raw.grad_item(tuple(item.shape)).copy_(out['g_item'])
        return raw

    def encode(spec, rows, table):
        resp, mask = rows.to_dense()
        out = T.fused_elbo_ref(table, torch.zeros(rows.num_item, spec.item_dim), resp, mask, torch.zeros(rows.num_person, spec.ability_dim),
                               want_grad=False, **cfg(spec, _lib.REG_KL))
        return out['ability_mu'], out['ability_logvar']

    ops._BACKEND.update(sparse_elbo=elbo, sparse_encode=encode)

    def restore():
        ops._BACKEND.update(saved)
    return restore


def cells_of(rows):
    """The image's two sides as sets of (person, item, right)."""
    def side(ptr, cell, by_row):
        out = set()
        ptr, cell = ptr.cpu().tolist(), (cell.cpu().to(torch.int64) & 0xffffffff).tolist()
        for q in range(len(ptr) - 1):
            for k in range(ptr[q], ptr[q + 1]):
                out.add((q, cell[k] >> 1, cell[k] & 1) if by_row else (cell[k] >> 1, q, cell[k] & 1))
        return out
    return side(rows.row_ptr, rows.row_cell, True), side(rows.col_ptr, rows.col_cell, False)
