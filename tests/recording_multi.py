"""The recording stand-in for ops._BACKEND['multi'] that the host tests of log_marginal's multi-sample path share."""
import torch

from oracle import cpu_backend
from oracle import vibo_table_ref as T
from vibo_amd import _lib


class RecordingMulti:
    """ops._BACKEND['multi'] evaluated sample by sample on the fp32 table oracle; keeps every call's arguments.  The table of sample
    s is table[s] of a stacked table ([S, B, 2A] given posteriors, [S, 2, I, 2A] conditional encoder tables of the item samples) and
    the table itself otherwise.  given=True: every call must carry a given-posterior spec.  answer=False: records and answers None,
    as a backend that does not cover the call."""

    def __init__(self, answer=True, given=False):
        self.calls, self.answer, self.given = [], answer, given

    def __call__(self, spec, response, mask, mask_code, row_index, table, items, eps, flow, reg_mode, num_person):
        self.calls.append(dict(spec=spec, mask=mask, mask_code=mask_code, table=table, items=items, eps=eps, flow=flow, reg_mode=reg_mode,
                               num_person=num_person))
        assert reg_mode == _lib.REG_SAMPLED and row_index is None and (spec.given or not self.given)
        if not self.answer:
            return None
        S, A = items.shape[0], spec.ability_dim
        resp, msk = cpu_backend._rows(response, mask, mask_code, None)
        flows = [(f[:A], f[A:2 * A], f[2 * A:2 * A + 1]) for f in flow] if flow is not None else None
        out = torch.zeros(S, _lib.NUM_SCALARS)
        for s in range(S):
            o = T.fused_elbo_ref(table[s] if table.dim() in (3, 4) else table, items[s], resp, msk, eps[s], flow_uhat_w_b=flows,
                                 want_grad=False, **cpu_backend._cfg(spec, reg_mode))
            out[s, _lib.S_LL], out[s, _lib.S_REG], out[s, _lib.S_KL] = o['ll'], o['reg'], o['kl_ability']
            out[s, _lib.S_LOGQ0], out[s, _lib.S_LOGP], out[s, _lib.S_LADJ] = o['logq0'], o['logp'], o['ladj_sum']
        return out
