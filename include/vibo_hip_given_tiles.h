/*
 * vibo_hip_given_tiles.h -- the tile image of a resident matrix (vibo_hip_tile_rows.h) under a caller-supplied posterior
 * (VIBO_POSTERIOR_GIVEN): two queries and the ELBO call, declared beside vibo_hip.h (its types, constants and conventions; include
 * that header and vibo_hip_tile_rows.h first or let this one do it).  vibo_amd/_lib.py binds the exports from this file as it binds
 * the others from vibo_hip.h.
 *
 * The image is the one vibo_tile_rows_build writes: what a matrix' code words and counts are depends on its cells alone, so the
 * image of a matrix serves the plain model's launches and these.  Build it with the same descriptor under
 * VIBO_POSTERIOR_UNCONDITIONAL and VIBO_FLAG_KERNEL_MATRIX.
 *
 * Every export of vibo_hip.h and vibo_hip_tile_rows.h keeps refusing a VIBO_MASK_TILES descriptor whose posterior is
 * VIBO_POSTERIOR_GIVEN (-8; size queries: 0): the combination is taken by the exports below alone.
 */
#ifndef VIBO_HIP_GIVEN_TILES_H
#define VIBO_HIP_GIVEN_TILES_H

#include "vibo_hip_tile_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * 1 if vibo_elbo_fwd_bwd_given_tiles takes a call with this descriptor, else 0: d->mask_dtype == VIBO_MASK_TILES, d->posterior ==
 * VIBO_POSTERIOR_GIVEN, no flows, 4..1024 items (one panel: the kernel's slot lanes read and write the posterior themselves), and
 * the matrix row-split kernel as the plan's engine -- by the planner's thresholds or by VIBO_FLAG_KERNEL_MATRIX.  Launches
 * nothing, needs no GPU.
 */
int vibo_given_tile_rows_supported(const vibo_desc* d);

/*
 * Workspace of vibo_elbo_fwd_bwd_given_tiles: what vibo_workspace_bytes answers for the same matrix as rows padded to whole
 * 4-cell chunks under VIBO_MASK_U8; 0 where vibo_given_tile_rows_supported answers 0.  Launches nothing, needs no GPU.
 */
size_t vibo_given_tiles_workspace_bytes(const vibo_desc* d);

/*
 * vibo_elbo_fwd_bwd (vibo_hip.h: the same arguments in the same order, the same outputs) on the tile image of the matrix under a
 * caller-supplied posterior.  `response` is the image (16-byte aligned, else -8); `mask`, `row_index`, `flow`, `ability_k`,
 * `ability_ladj` and `grad_flow` must be NULL; `table` is the posterior [num_person][2 ability_dim] (mean | log-variance) and
 * `grad_table` receives the two gradient sets [2][num_person][2 ability_dim], as in the VIBO_POSTERIOR_GIVEN call on rows.
 * Every output has the bits of that call on the rows the image was built from.
 * Returns 0, or before anything is launched: the descriptor checks' code; -8 a descriptor vibo_given_tile_rows_supported refuses,
 * a non-NULL row_index (vibo_last_error_string names it) or an unaligned image; -5 a NULL required pointer or a non-NULL one
 * of those that must be NULL; -7 a workspace that is too small or not 256-byte aligned.
 */
int vibo_elbo_fwd_bwd_given_tiles(const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index,
                                  const float* table, const float* item, const float* eps, const float* flow,
                                  float* out_scalars, float* ability_mu, float* ability_logvar, float* ability,
                                  float* ability_k, float* ability_ladj, float* grad_table, float* grad_item,
                                  float* grad_flow, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIBO_HIP_GIVEN_TILES_H */
