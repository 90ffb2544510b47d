/*
 * vibo_hip_sparse_row_driven.h -- the gathered ELBO call of vibo_hip_sparse_gather.h with a ROW-DRIVEN item pass: d LL / d item from the
 * batch's own cells, ordered by item once per call, in place of a walk over the image's whole column side.  Declared beside that header
 * (its index, its map, its conventions and its return codes; this file includes it); vibo_amd/_lib.py binds the exports from this file
 * as it binds the others.  The range calls, vibo_sparse_elbo_fwd_bwd_gather and the encode calls are untouched: same kernels, same bits.
 *
 * WHAT IS DIFFERENT.  The column side of the image is never read: col_ptr == NULL / num_chunk == 0 is accepted with d->want_grad (such
 * an image is 4 bytes per observed cell instead of 8).  The caller states the image's longest row, max_row_cells; it fixes the cell
 * capacity cap = B * max_row_cells (B = d->num_person) that the host sizes grids and workspace by, and it is NOT trusted: a live row's
 * cells beyond max_row_cells are not emitted (they take no part in grad_item; the person pass still sees the whole row) and each one
 * adds one to `bad_cells`.  cap must be in [1, 2^31).
 *
 * THE KEY.  One uint64 per emitted cell: item << (bP + 1) | person << 1 | right, bP = max(1, bit_length(P - 1)) for the image's P
 * persons.  Sorted over the bits [0, end_bit), end_bit = bP + 1 + bit_length(I) <= 63.  The pad key I << (bP + 1) is above every real
 * key: it stands for a cell whose item is >= I and fills the positions n .. cap that no cell takes.  A live person is owned by one row
 * of the call, so real keys are unique: the sorted list is a function of the SET of live persons alone, whatever the sort's stability
 * and whatever order the cells arrived in.
 *
 * THE LAUNCHES, in stream order, with no host synchronisation and no float atomics:
 *   1. map build     as in the column-driven gathered call (an integer atomicMin): liveness and ownership of repeats are that call's.
 *   2. person pass   that call's person pass and finish, unchanged.
 *   3. row offsets   two kernels.  B threads: len[r] = min(the live row's clamped cell count, max_row_cells), 0 for a row that is not
 *                    live.  Then an exclusive scan over the B rows (one workgroup, integers) leaves row_off[B + 1] and the batch's
 *                    cell count n = row_off[B] in device memory.  The host never reads n.
 *   4. emit          one wave per row, lane l the row's cells l, l + 64, ...: key[row_off[r] + k] as above; item >= I: the pad key
 *                    (the person pass counted that cell in bad_cells already).  The cells cut by max_row_cells are counted here.
 *                    Positions n .. cap get the pad key.
 *   5. sort          rocPRIM's device radix sort of the cap keys, ascending, over [0, end_bit), between the workspace's two key buffers.
 *   6. segment heads a thread per sorted position (the grid from cap; positions >= n and pad keys exit): a position whose item differs
 *                    from its predecessor's appends itself to the segment list through one integer atomic counter.  The list's order
 *                    is arbitrary and nothing depends on it.
 *   7. segment sums  grad_item is zeroed (a memset), then the waves of a host-known grid -- at most min(cap, I) segments, capped like
 *                    the person pass's grid: min(ceil(min(cap, I) / 4), VIBO_SPARSE_MAX_BLOCKS) workgroups of 4 waves -- stride over the
 *                    segment list.  A wave owns one item's segment: lane l takes the segment's entries l, l + 64, ... in order until
 *                    the item changes or n is reached, finds r = person_slot[person] (VIBO_SPARSE_NO_SLOT or a value outside [0, B) is
 *                    skipped), gathers theta from ability[r], RECOMPUTES the cell's terms with the person pass's statements and writes
 *                    the item's row of grad_item with the column-driven item kernel's per-column wave totals.  An item with no cell
 *                    among the call's persons keeps the memset's exact zeros.
 *   8. map clear     as in the column-driven call.
 *   Launches per call with gradients: 9 kernels of this library (map build, person pass, its finish, row lengths, row offsets, emit,
 *   segment heads, segment sums, map clear), two memsets (the counters, grad_item) and the sort's own kernels.
 *
 * THE COST, plainly.  Every pass after the person pass costs cap = B * max_row_cells keys, not the image: 8 bytes per key written by
 * the emit, the sort's passes over them (one per 8 key bits or fewer), 8 bytes per key read by the heads and the sums.  cap, not n: a
 * batch of short rows in an image with one long row pays for the long row B times.  A segment is walked by ONE wave: an item that
 * most of a large batch answers is a long serial walk (the column-driven pass cuts such a list into chunks of VIBO_SPARSE_CHUNK).
 * The workspace is 20 bytes per key and more: two key buffers and the sort's temporary storage.
 *
 * REPRODUCIBILITY.  Results are a function of the descriptor, the image, max_row_cells and the index vector alone.
 *   1. Two launches agree bit for bit, in every output.
 *   2. out_scalars, ability_mu, ability_logvar, ability and grad_table are bit-identical to vibo_sparse_elbo_fwd_bwd_gather's for the
 *      same inputs (the same launches 1 and 2).  Hence statements 2 and 3 of vibo_hip_sparse_gather.h hold for them here as well.
 *   3. grad_item is bit-identical under any permutation of person_index applied together to the rows of eps: the sorted keys depend on
 *      the set of live persons, a segment's lanes take its entries by sorted position, and a person's theta has the same bits at any
 *      row.  (The column-driven call has the same property; here it is what the sort by person buys over an arrival-order scatter.)
 *   4. grad_item agrees with the column-driven call's to rounding, not bit for bit: there a lane takes the entries l, l + 64, ... of
 *      a chunk of the image's column, here of the batch's own segment, so the lanes' partial sums hold different cells.
 */
#ifndef VIBO_HIP_SPARSE_ROW_DRIVEN_H
#define VIBO_HIP_SPARSE_ROW_DRIVEN_H

#include "vibo_hip_sparse_gather.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Workspace bytes of vibo_sparse_elbo_fwd_bwd_gather_rows for d (B = d->num_person rows) on an image of num_person_image persons and
 * num_item items whose longest row has max_row_cells cells: the person pass's records as in vibo_sparse_workspace_bytes, then the row
 * offsets, the counters, the segment list, two buffers of cap keys and the sort's temporary storage (a bound that does not ask the
 * device: 4 bytes per key and 256 KiB; the call checks it against what the sort asks for), each 256-byte rounded.  With
 * d->want_grad == 0: vibo_sparse_workspace_bytes(d, 0).  0 where the descriptor is not supported, a size is out of range, or cap is
 * outside [1, 2^31).  Launches nothing, needs no GPU.
 */
size_t vibo_sparse_row_driven_workspace_bytes(const vibo_desc* d, int64_t num_item, int64_t num_person_image, int64_t max_row_cells);

/*
 * vibo_sparse_elbo_fwd_bwd_gather with the row-driven item pass above: arguments, outputs, layouts and return codes are that call's.
 * max_row_cells: the image's longest row as the caller states it (see WHAT IS DIFFERENT).  workspace: the query above, 256-byte aligned.
 * d->want_grad == 0 forwards to vibo_sparse_elbo_fwd_bwd_gather: no map, max_row_cells is not read, the same bits.
 * Returns that call's codes, and: -8 where cap = d->num_person * max_row_cells is outside [1, 2^31) (checked before anything else of
 * the call but the descriptor; the message names the column-driven call, which has no such limit), or where the sort asks for more
 * temporary storage than the workspace's bound; a positive HIP code from the sort.  An image without a column side is NOT refused.
 */
int vibo_sparse_elbo_fwd_bwd_gather_rows(const vibo_desc* d, const vibo_sparse_image* image,
                                         const int64_t* person_index, int32_t* person_slot, int64_t max_row_cells,
                                         const float* table, const float* item, const float* eps,
                                         float* out_scalars, float* ability_mu, float* ability_logvar, float* ability,
                                         float* grad_table, float* grad_item, int64_t* bad_cells,
                                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIBO_HIP_SPARSE_ROW_DRIVEN_H */
