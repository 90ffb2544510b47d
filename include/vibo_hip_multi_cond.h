/*
 * vibo_hip_multi_cond.h -- the multi-sample forward of the conditional product of experts: two more exports of libvibo_hip.so,
 * declared beside vibo_hip.h (its types, constants and conventions; include that header first or let this one do it).
 * vibo_amd/_lib.py binds them from this file as it binds the others from vibo_hip.h.
 */
#ifndef VIBO_HIP_MULTI_COND_H
#define VIBO_HIP_MULTI_COND_H

#include "vibo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * vibo_elbo_multi_forward_given's pass for the product of experts of the conditional posterior (d->posterior must be VIBO_POSTERIOR_CONDITIONAL, else -3),
 * whose expert table depends on the item sample and which vibo_elbo_multi_forward refuses with -8.  `tables` holds the encoder's
 * (mu | logvar) table of every item sample, [num_samples][2][num_item][2 ability_dim] (the `table` of vibo_elbo_fwd_bwd, one per
 * sample; computed from the item sample in front of the item-side flows).  Inside the call, on `stream`:
 *   1. fp32 rows (+ u8 mask or none) are packed once into 1-byte cell codes in the workspace, in minibatch order; VIBO_MASK_CODES rows
 *      are read as they are (through row_index);
 *   2. per group of up to 64 / (2 ability_dim) samples ONE one-hot x table contraction over the codes gives every sample's experts'
 *      sums (precision | precision-weighted mean, side by side in up to 64 columns) and, once per call, the rows' observed counts;
 *   3. a per-person finish turns them into the samples' posteriors (vibo_encode's arithmetic: under VIBO_MISSING_PRIOR the N(0,1)
 *      experts of the missing cells are added; a person without an observed cell under VIBO_MISSING_DROP comes out NaN);
 *   4. vibo_elbo_multi_forward_given's pass runs on the codes with those posteriors (stride num_person * 2 ability_dim).
 *     out_scalars[s][VIBO_NUM_SCALARS]   the heads of vibo_elbo_multi_forward_given for the posterior of sample s (NOBS = num_person *
 *                                        num_item; S_LL and S_REG are what log_marginal reads)
 *     posterior_out                      optional [num_samples][num_person][2 ability_dim] (mu | logvar), minibatch order; NULL: the
 *                                        posteriors stay in the workspace
 * Shapes: those of vibo_elbo_multi_forward_given (4..32767 items, rows chunkable in 4 cells, no int64 mask, ability_dim <= 8);
 * outside them -8 and a workspace query of 0: loop over vibo_elbo_fwd_bwd instead.  The same answer for VIBO_MASK_CODES rows at
 * ability_dim >= 3, where one launch per sample was measured faster (1M x 1k, 16 samples: 13.0 against 13.8 ms at 3 dims, 13.5
 * against 18.5 at 8; fp32 rows and 1 - 2 dims win); VIBO_FLAG_COND_MATRIX pins this call there.
 * Workspace: vibo_multi_cond_workspace_bytes(d, num_samples) bytes, 256-byte aligned (0: no plan for the descriptor).
 */
size_t vibo_multi_cond_workspace_bytes(const vibo_desc* d, int num_samples);
int vibo_elbo_multi_forward_cond(const vibo_desc* d, int num_samples, const float* response, const void* mask,
                                 const int64_t* row_index, const float* tables, const float* item, const float* eps,
                                 const float* flow, float* out_scalars, float* posterior_out, void* workspace,
                                 size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VIBO_HIP_MULTI_COND_H */
