/*
 * vibo_hip_sign_rows.h -- fp32 response rows whose sign bit is the mask: one more row format of libvibo_hip.so, one query and
 * one verifier, declared beside vibo_hip.h (its types, constants and conventions; include that header first or let this one do
 * it).  vibo_amd/_lib.py binds the exports from this file as it binds the others from vibo_hip.h.
 */
#ifndef VIBO_HIP_SIGN_ROWS_H
#define VIBO_HIP_SIGN_ROWS_H

#include "vibo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * vibo_desc.mask_dtype = VIBO_MASK_SIGN: `mask` is NULL and a cell is missing iff the sign bit of its fp32 response is set
 * (the reference stores -1 at missing cells and builds every mask from that); an observed cell is read as in every other fp32
 * format (bit 0 of the float's top byte: 0.0f wrong, 1.0f right).  -0.0f and negative NaNs count as missing.  The matrix
 * row-split kernel then streams 4 instead of 5 bytes per cell and issues half of the load instructions.
 *
 * Taken only where it is implemented -- a call the planner sends to the single-launch matrix row-split kernel: unconditional
 * posterior, no flows, 4..1024 items, rows chunkable as for VIBO_MASK_U8 (response stride only), row_index == NULL -- by
 *     vibo_elbo_fwd_bwd, vibo_elbo_fwd_bwd_step, vibo_elbo_fwd_bwd_step_noise (also drawing its own noise),
 *     vibo_workspace_bytes, vibo_plan_kernel, vibo_train_step_supported / _draws_noise / _sample_optional
 * (the three step queries answer what they answer for the same descriptor with VIBO_MASK_U8).  Every other export, and every other shape,
 * refuses the descriptor before anything is launched: -8 (size queries: 0; vibo_dtrain_scratch_offset: -1) with
 * vibo_last_error_string naming the format where the export sets it.
 */
#define VIBO_MASK_SIGN 4

/* 1 if a call with this descriptor (d->mask_dtype == VIBO_MASK_SIGN) is taken, else 0.  Launches nothing, needs no GPU. */
int vibo_sign_rows_supported(const vibo_desc* d);

/*
 * Does the sign of the responses say what the mask says?  d describes fp32 rows with a VIBO_MASK_U8 mask (num_person x num_item,
 * the two row strides).  *differs (device memory) is zeroed, then set to 1 if any cell i < num_item of any row has a mask byte
 * above 1 (the matrix kernel reads mask bytes as 0 / 1) or (mask byte == 1) != (sign bit of the response clear); the cells of
 * the row padding are not looked at.  Where it stays 0, a VIBO_MASK_SIGN call on `response` alone forms the code words of the
 * VIBO_MASK_U8 call on (response, mask), so every output agrees bit for bit.  One streaming pass (5 B per cell), asynchronous
 * on `stream`.
 * Returns 0, or: the descriptor checks' code; -8 mask_dtype != VIBO_MASK_U8; -5 a NULL pointer.
 */
int vibo_rows_sign_is_mask(const vibo_desc* d, const float* response, const void* mask, int32_t* differs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIBO_HIP_SIGN_ROWS_H */
