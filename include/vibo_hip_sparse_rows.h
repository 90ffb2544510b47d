/*
 * vibo_hip_sparse_rows.h -- a response matrix held as its observed cells only: one more row format of libvibo_hip.so, with an ELBO
 * call, an encode call and a validation pass of its own, declared beside vibo_hip.h (its types, constants and conventions; include
 * that header first or let this one do it).  vibo_amd/_lib.py binds the exports from this file as it binds the others from vibo_hip.h.
 *
 * Every other row format pays for each cell of the matrix, observed or not, and stops at 32 767 items.  Here a call costs the observed
 * cells of its persons: the plain model's per-person math needs a row's two counts (answered wrong, answered right) and the number
 * of its missing cells, never where they are, and only the decode, the log-likelihood and d LL / d item visit single cells.
 *
 * THE IMAGE (an interface: vibo_amd/sparse.py builds it, csrc/vibo_sparse.hip and tests/sparse_rows_common.py read it).
 *   P persons x I items with nnz observed cells, listed twice.  All integers little-endian; every array is device memory the caller owns.
 *   Row side (CSR)
 *     row_ptr   int64  [P + 1]   row_ptr[0] = 0, non-decreasing, row_ptr[P] = nnz; person p owns cells row_ptr[p] .. row_ptr[p + 1] - 1
 *     row_cell  uint32 [nnz]     item << 1 | right   (right = 1: answered right, 0: answered wrong), items strictly ascending inside a row
 *   Column side (CSC): the same cells, by item
 *     col_ptr   int64  [I + 1]   col_ptr[0] = 0, non-decreasing, col_ptr[I] = nnz
 *     col_cell  uint32 [nnz]     person << 1 | right, persons strictly ascending inside a column
 *     The chunk list cuts every column's list into pieces of at most VIBO_SPARSE_CHUNK entries, columns in order, pieces in order:
 *     col_chunk   int64 [I + 1]         item i owns chunks col_chunk[i] .. col_chunk[i + 1] - 1: ceil((col_ptr[i + 1] - col_ptr[i]) / VIBO_SPARSE_CHUNK)
 *                                       of them (none for an item nobody answered); col_chunk[0] = 0, col_chunk[I] = num_chunk
 *     chunk_item  int32 [num_chunk]     the item of chunk c
 *     chunk_first int64 [num_chunk]     its first entry of col_cell: col_ptr[item] + VIBO_SPARSE_CHUNK * (c - col_chunk[item]); the chunk ends
 *                                       VIBO_SPARSE_CHUNK entries later or at col_ptr[item + 1], whichever comes first
 *   An image without a column side (col_ptr == NULL, num_chunk == 0) serves vibo_sparse_encode and forward-only ELBO calls.
 *   Limits: 1 <= P, I < 2^31; nnz and num_chunk are int64 (the limit is device memory).
 *
 * No launch trusts an index.  A row-side cell whose item is >= I, and a column-side cell whose person is >= P, is not dereferenced: it
 * contributes nothing and adds one to the caller's `bad_cells` counter (sticky: the library only ever adds to it).  Pointer entries are
 * clamped to [0, nnz] and chunk entries to their arrays before they are used.  vibo_sparse_rows_check counts what is wrong with an image.
 *
 * THE GRID RULE (results are bitwise reproducible: the grid and every summation order depend on the descriptor and the image's sizes alone).
 *   Person pass: G = min(ceil(B / VIBO_SPARSE_ROWS_PER_BLOCK), VIBO_SPARSE_MAX_BLOCKS) workgroups of 4 waves, B = d->num_person.  Wave w
 *     (= 4 x workgroup + wave in it, w < 4 G) takes the call's rows w, w + 4 G, w + 8 G, ... in that order, one row at a time, lane l the
 *     row's cells l, l + 64, ...; sums over a row's cells are wave totals, sums over a wave's rows run in row order, and every wave leaves
 *     one partial record.  The finish adds the 4 G records: lane l of a wave adds records l, l + 64, ... in order, then a wave total.
 *   Item pass: one wave per chunk (4 chunks per workgroup), lane l the in-range entries l, l + 64, ... of the chunk, a wave total per
 *     column of `item`.  An item of one chunk gets its row of grad_item from that wave; an item of several chunks one record per chunk,
 *     added in chunk order by the finish; an item of no chunk zeros.
 */
#ifndef VIBO_HIP_SPARSE_ROWS_H
#define VIBO_HIP_SPARSE_ROWS_H

#include "vibo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIBO_SPARSE_CHUNK 512             /* entries of a column's list per chunk (the split measured for skewed destination lists; not yet timed on this format) */
#define VIBO_SPARSE_ROWS_PER_BLOCK 32     /* person pass: rows per workgroup until the grid is full ... */
#define VIBO_SPARSE_MAX_BLOCKS 1024       /* ... at this many workgroups of 4 waves */
#define VIBO_SPARSE_RECORD_FLOATS 72      /* a person-pass wave's partial record: ll, kl, logq0, logp, cells (an int32's bits), 0, 0, 0 | d table [2][2][16] */

/* The image (host memory, POD; the pointers are device pointers). */
typedef struct vibo_sparse_image {
    int64_t num_person;          /* P */
    int64_t num_item;            /* I */
    int64_t nnz;
    int64_t num_chunk;           /* 0: no column side */
    const int64_t* row_ptr;
    const uint32_t* row_cell;
    const int64_t* col_ptr;      /* NULL: no column side (then col_cell, col_chunk, chunk_item, chunk_first are not read) */
    const uint32_t* col_cell;
    const int64_t* col_chunk;
    const int32_t* chunk_item;
    const int64_t* chunk_first;
} vibo_sparse_image;

/*
 * 1 if the sparse calls take this descriptor, else 0: the plain model -- VIBO_POSTERIOR_UNCONDITIONAL, IRT decoder 1PL / 2PL / 3PL, both
 * missing_modes, VIBO_REG_KL and VIBO_REG_SAMPLED, n_flows == 0, ability_dim 1..VIBO_MAX_ABILITY_DIM, num_item >= 1.  d->num_person is
 * the B persons of a call; d->mask_dtype, the two row strides and d->flags are not read.  Launches nothing, needs no GPU.
 */
int vibo_sparse_rows_supported(const vibo_desc* d);

/*
 * Workspace bytes of vibo_sparse_elbo_fwd_bwd for d on an image of num_chunk chunks: the person pass's records (256-byte rounded) and,
 * with d->want_grad, one [D] record per chunk; 0 where the descriptor is not supported.  Launches nothing, needs no GPU.
 */
size_t vibo_sparse_workspace_bytes(const vibo_desc* d, int64_t num_chunk);

/*
 * One pass over the image that OVERWRITES *violations (device int64) with the number of failed checks:
 *   row_ptr[0] != 0, row_ptr[P] != nnz, each p with row_ptr[p] > row_ptr[p + 1] or an entry outside [0, nnz]    (one each; such a row's cells are skipped)
 *   each row-side cell with item >= I; each cell whose item is not above its predecessor's in the row
 *   the same for col_ptr / col_cell (person >= P; persons not ascending)
 *   each column-side cell (person p < P, item i) that a bisection of row p's list does not find with the same `right`
 *     (with both sides strictly sorted and of nnz cells each, this makes them the same set; in a row that is out of order the bisection may miss cells that are there)
 *   col_chunk[0] != 0, col_chunk[I] != num_chunk; each item whose chunk count is not ceil(length / VIBO_SPARSE_CHUNK); each chunk whose chunk_item or
 *     chunk_first is not what the layout above says
 * An image without a column side gets the row-side checks only.  Returns 0, -3 (sizes out of range), -5 (NULL pointer), or a HIP code.
 */
int vibo_sparse_rows_check(const vibo_sparse_image* image, int64_t* violations, void* stream);

/*
 * vibo_elbo_fwd_bwd for the contiguous persons [row0, row0 + d->num_person) of the image: outputs, layouts and meaning are those of that
 * call on the same rows held densely (include/vibo_hip.h) -- out_scalars [VIBO_NUM_SCALARS] (VIBO_S_NOBS: the range's cells, counted in integers and rounded to fp32 once; VIBO_S_LADJ 0),
 * ability_mu / ability_logvar / ability [B][A], grad_table [2][2][2A], grad_item [I][D] (an item with no cell in the range: exact zeros).
 * table [2][2A], item [I][D], eps [B][A].  d->want_grad == 0: the forward heads only; grad_table / grad_item may be NULL and the column
 * side is not read.  bad_cells: device int64 the call adds the untrusted cells it skipped to (see above), or NULL.
 * Two launches and a finish, no float atomics: bitwise reproducible by the grid rule above.
 * Returns 0, or: the descriptor checks' codes (-1, -2, -3); -3 an image whose sizes disagree with the descriptor or a range outside it;
 * -5 a NULL pointer; -7 a workspace below vibo_sparse_workspace_bytes or not 256-byte aligned; -8 a descriptor
 * vibo_sparse_rows_supported refuses, or gradients from an image without a column side.  Every message names the format ("sparse rows").
 */
int vibo_sparse_elbo_fwd_bwd(const vibo_desc* d, const vibo_sparse_image* image, int64_t row0,
                             const float* table, const float* item, const float* eps,
                             float* out_scalars, float* ability_mu, float* ability_logvar, float* ability,
                             float* grad_table, float* grad_item, int64_t* bad_cells,
                             void* workspace, size_t workspace_bytes, void* stream);

/* vibo_encode for the same range: the posterior's mean and log-variance [B][A] from the row side alone.  No workspace.  Return codes as above. */
int vibo_sparse_encode(const vibo_desc* d, const vibo_sparse_image* image, int64_t row0, const float* table,
                       float* ability_mu, float* ability_logvar, int64_t* bad_cells, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIBO_HIP_SPARSE_ROWS_H */
