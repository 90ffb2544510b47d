/*
 * vibo_hip_sparse_gather.h -- sparse response rows for an index vector of persons: the ELBO call and the encode call of
 * vibo_hip_sparse_rows.h for the persons person_index[0..B) in place of a contiguous range (person-shuffled minibatches, chosen
 * subsets).  Declared beside that header (its image, its constants, its grid rule and its conventions; this file includes it);
 * vibo_amd/_lib.py binds the exports from this file as it binds the others.  The range calls are untouched: same kernels' range
 * instantiations, same bits.
 *
 * THE INDEX AND THE MAP.
 *   person_index  int64 [B]  (device)  row r of `eps` and of the three [B][A] outputs belongs to person person_index[r] of the image.
 *   person_slot   int32 [P]  (device)  a caller-owned map, all VIBO_SPARSE_NO_SLOT before a call with gradients; the call builds in it
 *                                      "person -> the row of this call that owns it", uses it, and leaves it all VIBO_SPARSE_NO_SLOT again,
 *                                      stream-ordered.  One gathered call per map may be in flight.  With d->want_grad == 0 there is
 *                                      no map: person_slot may be NULL and is not touched.
 *   No launch trusts an index.  A row r whose person_index[r] is outside [0, P) is not live; with gradients neither is a row whose
 *   person an earlier row of the call names already (the smallest r owns a person: gradients of a person named twice would need
 *   two thetas in the item pass).  A row that is not live contributes nothing to any sum, gets zeros in its rows of
 *   ability_mu / ability_logvar / ability and adds one to `bad_cells`.  Without gradients repeats are ordinary rows.  A map entry that
 *   is neither VIBO_SPARSE_NO_SLOT nor a row of the call is skipped.
 *
 * THE LAUNCHES, in stream order, with no host synchronisation (the call can be captured into a graph):
 *   1. map build   B threads: q = person_index[r]; in range: atomicMin(&person_slot[q], r) -- an integer minimum, the same whatever
 *                  the arrival order.                                                             (with gradients only)
 *   2. person pass the range call's pass with the row taken from the index (q = person_index[r] in place of row0 + r), live rows only:
 *                  the same grid rule over B, the same lane and row order, the same records, the same finish.
 *   3. item pass   one wave per chunk as in the range call, without the bisection: the wave walks the whole chunk, lane l the entries
 *                  first + l, first + l + 64, ...; for a person q < P it looks up r = person_slot[q], skips VIBO_SPARSE_NO_SLOT and
 *                  reads theta from ability[r]; the same cell terms, the same wave totals, the same chunk records, the same item
 *                  finish.  An item with no cell among the call's persons gets exact zeros.          (with gradients only)
 *   4. map clear   B threads: person_slot[q] = VIBO_SPARSE_NO_SLOT for the in-range q.              (with gradients only)
 *   No float atomics.
 *
 * THE COST, plainly.  The person pass costs the batch's cells.  The item pass streams the image's WHOLE column side -- 4 bytes per
 * observed cell of the matrix, whatever B is -- and gathers one map entry per entry: the price of a fixed summation order without a
 * per-call sort.  A batch that is a small share of a large image pays mostly for cells that are not its own; the range call's
 * bisection has no counterpart for an unordered index.
 *
 * REPRODUCIBILITY.  Results are a function of the descriptor, the image and the index vector alone.
 *   1. Two launches agree bit for bit.
 *   2. With person_index = row0, row0 + 1, ..., row0 + B - 1 the person pass's outputs -- out_scalars, ability_mu, ability_logvar,
 *      ability, grad_table -- are bit-identical to vibo_sparse_elbo_fwd_bwd(row0)'s.  grad_item is bit-identical when the range is
 *      the whole image (there the range call's bisection window is the whole chunk, so the lanes take the same entries); otherwise
 *      it is equal to rounding, because the lanes' entries differ.
 *   3. A person's row of ability_mu / ability_logvar has the same bits at any position of any index vector, from either call below.
 */
#ifndef VIBO_HIP_SPARSE_GATHER_H
#define VIBO_HIP_SPARSE_GATHER_H

#include "vibo_hip_sparse_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIBO_SPARSE_NO_SLOT 0x7fffffff    /* a person_slot entry: no row of the call in flight owns this person */

/*
 * vibo_sparse_elbo_fwd_bwd for the persons person_index[0..B), B = d->num_person: outputs, layouts and meaning are that call's, row r
 * for person person_index[r].  workspace: vibo_sparse_workspace_bytes(d, image->num_chunk), as for the range call.
 * Returns that call's codes, and: -5 a NULL person_index, or a NULL person_slot with d->want_grad; -3 an image whose sizes disagree
 * with the descriptor; -8 a descriptor vibo_sparse_rows_supported refuses, or gradients from an image without a column side.
 * Every message names the format ("sparse rows").
 */
int vibo_sparse_elbo_fwd_bwd_gather(const vibo_desc* d, const vibo_sparse_image* image,
                                    const int64_t* person_index, int32_t* person_slot,
                                    const float* table, const float* item, const float* eps,
                                    float* out_scalars, float* ability_mu, float* ability_logvar, float* ability,
                                    float* grad_table, float* grad_item, int64_t* bad_cells,
                                    void* workspace, size_t workspace_bytes, void* stream);

/*
 * vibo_sparse_encode for the same persons: the posterior's mean and log-variance [B][A] from the row side alone.  No map and no
 * workspace: every row is independent, so repeats are allowed; an index outside [0, P) writes zeros and adds one to bad_cells.
 * Return codes as above.
 */
int vibo_sparse_encode_gather(const vibo_desc* d, const vibo_sparse_image* image, const int64_t* person_index, const float* table,
                              float* ability_mu, float* ability_logvar, int64_t* bad_cells, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIBO_HIP_SPARSE_GATHER_H */
