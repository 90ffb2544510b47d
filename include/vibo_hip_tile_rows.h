/*
 * vibo_hip_tile_rows.h -- a resident response matrix as prepacked code-word tiles: one more row format of libvibo_hip.so, two
 * queries and the builder of its image, declared beside vibo_hip.h (its types, constants and conventions; include that header
 * and vibo_hip_sign_rows.h first or let this one do it).  vibo_amd/_lib.py binds the exports from this file as it binds the others from vibo_hip.h.
 */
#ifndef VIBO_HIP_TILE_ROWS_H
#define VIBO_HIP_TILE_ROWS_H

#include "vibo_hip_sign_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * vibo_desc.mask_dtype = VIBO_MASK_TILES: `response` points at the tile image of the matrix (vibo_tile_rows_build; 16-byte
 * aligned), `mask` is NULL, and the descriptor's two row strides are not read.  The matrix row-split kernel then loads the code
 * words and the answer counts of a batch of 32 rows as it consumes them -- five load instructions per wave and batch, about
 * 1.06 bytes per cell of the padded panel -- and packs and counts nothing.  What the words and counts of a matrix are depends
 * on its cells alone, so an image is built once per matrix and serves every launch on it, whatever the model.
 *
 * Taken only where it is implemented -- the shapes of VIBO_MASK_SIGN (vibo_hip_sign_rows.h): a call the planner sends to the
 * single-launch matrix row-split kernel: unconditional posterior, no flows, 4..1024 items, row_index == NULL, any number of
 * persons the planner gives that kernel (or VIBO_FLAG_KERNEL_MATRIX) -- by
 *     vibo_elbo_fwd_bwd, vibo_elbo_fwd_bwd_step, vibo_elbo_fwd_bwd_step_noise (also drawing its own noise),
 *     vibo_workspace_bytes, vibo_plan_kernel, vibo_train_step_supported / _draws_noise / _sample_optional
 * (the three step queries answer what they answer for the same descriptor with VIBO_MASK_U8).  Every other export, and every
 * other shape, refuses the descriptor before anything is launched: -8 (size queries: 0; vibo_dtrain_scratch_offset: -1) with
 * vibo_last_error_string naming the format where the export sets it.  Every output of a launch on the image has the bits of the
 * launch on the rows the image was built from.
 *
 * THE IMAGE (an interface: vibo_tile_rows_build writes it, the kernel and tests/tile_rows_common.py read it).
 *   P persons x I items, W = ceil(I / 128) waves, NB = ceil(P / 32) batches.  All integers little-endian.
 *   image      = batch block [NB]                   batch bt = rows 32 bt .. 32 bt + 31; independent of the launch's grid
 *   batch block = wave block [W]                    wave q = items 128 q .. 128 q + 127
 *   wave block  = 4352 bytes = code words (4096) | counts (256)
 *   Lane l = 16 g + i16 (g = 0..3, i16 = 0..15) of the wave that reads the block owns, for u = 0, 1 and h = 0, 1 and j = 0..3,
 *   code word (u, 4 h + j): person (row of the batch) 16 h + 4 g + j at items 4 c + 0..3 of the matrix, c = 32 q + 16 u + i16,
 *   one byte per item, lowest byte = lowest item:
 *       0x00 missing | 0x38 observed, answered wrong | 0xB8 observed, answered right.
 *   The words lie as four runs of 1024 bytes, run k = 2 h + u, so that load k of a wave is one 16-byte-per-lane instruction:
 *       byte offset of word (u, 4 h + j) of lane l in the wave block = 1024 (2 h + u) + 16 l + 4 j.
 *   (runs 0 and 1 are M-tile 0 -- persons 0..15 of the batch --, runs 2 and 3 M-tile 1: the kernel may ask for them apart.)
 *   Counts: one dword per lane at byte offset 4096 + 4 l:
 *       bits  0..15  observed cells of row (l & 31) of the batch among the wave's 128 items
 *       bits 16..23  of those, answered right
 *       bits 24..31  observed cells among the lane's own 64 (its 16 words)
 *   Cells at items >= I, and rows >= P of the last batch, are 0x00 and are counted nowhere.
 *
 *   A cell of fp32 rows is "right" iff it is observed and bit 0 of the float's top byte is set (0.0f wrong, 1.0f right), as in
 *   every fp32 format.  Observed means: VIBO_MASK_U8 -- its mask byte is 1 (the bytes are 0 or 1, as the matrix kernel reads
 *   them on fp32 rows; the image of other byte values is whatever that kernel's pack forms from them); VIBO_MASK_NONE -- always;
 *   VIBO_MASK_SIGN -- the float's sign bit is clear; VIBO_MASK_CODES -- the code byte is 0 (wrong) or 1 (right), not 2.
 */
#define VIBO_MASK_TILES 6      /* (5 is no format: it stays a bad mask_dtype, -3) */
/* the two row formats of the ELBO call alone */
#define VIBO_MASK_IS_ELBO_ONLY(mask_dtype) ((mask_dtype) == VIBO_MASK_SIGN || (mask_dtype) == VIBO_MASK_TILES)

/* 1 if a call with this descriptor (d->mask_dtype == VIBO_MASK_TILES) is taken, else 0.  Launches nothing, needs no GPU. */
int vibo_tile_rows_supported(const vibo_desc* d);

/* Bytes of the image of d's matrix (d->mask_dtype == VIBO_MASK_TILES): 4352 ceil(I / 128) ceil(P / 32); 0 where the format is
 * not supported.  Launches nothing, needs no GPU. */
size_t vibo_tile_rows_bytes(const vibo_desc* d);

/*
 * Build the image of the matrix `src` describes: num_person x num_item source rows with their two row strides, as fp32 +
 * VIBO_MASK_U8, fp32 + VIBO_MASK_NONE, VIBO_MASK_SIGN (mask NULL in both) or VIBO_MASK_CODES (response NULL, the codes through
 * `mask`); the rest of the descriptor as for the launches that will read the image.  The words and counts are, bit for bit,
 * those the matrix kernel forms from the same source rows.  Rows of any alignment.  One streaming pass, asynchronous on `stream`.
 * Returns 0, or: the descriptor checks' code; -5 a NULL / mismatched pointer; -7 image_bytes below vibo_tile_rows_bytes or an
 * image that is not 16-byte aligned; -8 any other source format, or a shape the format is not supported for.
 */
int vibo_tile_rows_build(const vibo_desc* src, const void* response, const void* mask, void* image, size_t image_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIBO_HIP_TILE_ROWS_H */
