/*
 * vibo_hip_person_tables.h -- the native train step of the two un-amortized methods, whose person-side parameters are tables with
 * one row per person: VI (vi.py: ability_mu_lookup / ability_logvar_lookup [P][A]) and maximum likelihood (mle.py: ability
 * [P][A]).  Declared beside vibo_hip.h (its types, constants and conventions); vibo_amd/_lib.py binds the exports from this file as
 * it binds the others from vibo_hip.h.
 *
 * A step is   vibo_ptrain_prologue -> vibo_elbo_fwd_bwd (VIBO_POSTERIOR_GIVEN, table = `posterior`) -> vibo_ptrain_epilogue
 * and is torch.optim.Adam on the dense tables: EVERY row of every table is updated every step -- moments decay and parameters move
 * on momentum also for persons outside the minibatch, whose gradient is exactly 0.  Nothing here is a lazy or sparse Adam.
 *
 * All pointers are device memory, the scalars beta / lr / step_count live on the device as in vibo_train_*, every call is
 * asynchronous on `stream` and hipGraph-capturable.  d describes the minibatch as the ELBO call between the two sees it
 * (num_person = B, num_item, ability_dim = A <= VIBO_MAX_ABILITY_DIM, irt_model; posterior must be VIBO_POSTERIOR_GIVEN).
 *
 *  mode        VIBO_PTRAIN_VI: two tables, table_a = mu, table_b = logvar; VIBO_PTRAIN_MLE: one table, table_a = ability,
 *              table_b is not read (NULL)
 *  table_rows  P: rows of each table
 *  index       [B] int64: the person of minibatch position b.  An index outside [0, table_rows) is never dereferenced: its
 *              position gets the posterior row (0 | 0), its gradient is dropped and *bad_count is incremented (sticky: nothing
 *              here ever clears it).  A person may occur more than once: the gradients of its positions are summed in position
 *              order (what embedding backward does), bitwise reproducibly.
 *  slot        [P] int32, all -1 between two steps (the caller fills it once): the inverse map person -> owning position.  The
 *              prologue claims slot[index[b]] for the first position that names the person, the epilogue reads it and leaves
 *              it all -1 again.  4 B per person and step.
 *  person_m/v  Adam's moments of the tables: table k's [P][A] at person_m + k * moment_stride (VI: k = 0 mu, 1 logvar;
 *              moment_stride >= P A; a multiple of 4 keeps the second table on the 16-byte path)
 *  step_count  int32[2]: [0] Adam's t (the prologue ticks it), [1] completed steps = the noise counter (the epilogue ticks it)
 *
 * Return codes: 0, or -2 / -3 the descriptor checks of vibo_hip.h, -6 a descriptor these calls do not take (posterior, flows,
 * ability_dim, mode), -8 d->mask_dtype == VIBO_MASK_SIGN (a row format of the ELBO call alone), -5 a NULL pointer; otherwise the
 * hipError_t of the launch.  All of that is decided before anything is launched and needs no GPU.
 */
#ifndef VIBO_HIP_PERSON_TABLES_H
#define VIBO_HIP_PERSON_TABLES_H

#include "vibo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIBO_PTRAIN_VI 0
#define VIBO_PTRAIN_MLE 1

/*
 * One launch: step_count[0] += 1; posterior[b] = (mu[index[b]] | logvar[index[b]]) (VI) or (ability[index[b]] | 0) (MLE); the slot
 * claims.  VI only: item_feat = item_mu + exp(.5 item_logvar) eps_item and the item-KL partial sums in kl_parts (one per 64 item
 * entries), as vibo_train_prologue; with draw_noise eps_item [I][D] and eps_ability [B][A] are WRITTEN first, with the values
 * vibo_fill_normal gives at counter step_count[1] for stream 0 and stream ability_stream_id (as vibo_train_prologue_noise).
 * MLE has no noise and no item sample: item_mu .. kl_parts (but for step_count) are not read and may be NULL; the ELBO call takes
 * the item table itself and a zero eps.
 */
int vibo_ptrain_prologue(const vibo_desc* d, int mode, int64_t table_rows, const float* table_a, const float* table_b,
                         const int64_t* index, float* posterior, int32_t* slot, int32_t* bad_count, const float* item_mu,
                         const float* item_logvar, float* eps_item, uint64_t seed, int draw_noise, float* eps_ability,
                         uint32_t ability_stream_id, float* item_feat, float* kl_parts, int32_t* step_count, void* stream);

/*
 * flat: what vibo_elbo_fwd_bwd left, [8 scalars | grad_table [2][B][2A] | grad_item [I][D]].
 *   loss      VI: -LL + beta (REG + KL_item); MLE: -LL / (B num_item)
 *   items     VI: (item_mu, item_logvar) through the sample and the item KL, Adam in place (item_m / item_v: [mu | logvar]);
 *             MLE: Adam on the item table `item_mu` with g = -dLL/ditem / (B num_item) (item_logvar, eps_item, kl_parts: NULL)
 *   persons   vibo_person_table_adam's update of every entry of every table, with
 *             VI: g = -grad_table[0] + beta grad_table[1], columns 0..A for mu and A..2A for logvar; MLE: g = -grad_table[0][:, :A] / (B num_item)
 *   step_count[1] += 1
 * Two launches: everything above, then B threads that put the claimed slots back to -1 (the update's threads all read the map;
 * a launch boundary is what orders the reset behind the last of them).
 */
int vibo_ptrain_epilogue(const vibo_desc* d, int mode, int64_t table_rows, const float* flat, const int64_t* index,
                         const float* kl_parts, const float* eps_item, const float* beta, const float* lr, int32_t* step_count,
                         float* table_a, float* table_b, float* person_m, float* person_v, int64_t moment_stride, int32_t* slot,
                         float* item_mu, float* item_logvar, float* item_m, float* item_v, float* loss_out, void* stream);

/*
 * The person-table update alone (the device code the epilogue runs): claims, update, reset -- three launches, slot all -1 before
 * and after.  grad_rows: [2][B][2A] as vibo_elbo_fwd_bwd leaves it in VIBO_POSTERIOR_GIVEN mode; step_count[0] is Adam's t and is
 * only read.  For every entry of every table: g = the gradient of its person summed over the positions that name it (exactly 0
 * where none does), then m = .9 m + .1 g, v = .999 v + .001 g g, p -= lr / (1 - .9^t) m / (sqrt(v) / sqrt(1 - .999^t) + 1e-8)
 * (torch.optim.Adam, the arithmetic of every trainer here).  Flat over the P A entries in 16-byte groups (scalar where a pointer
 * is not 16-byte aligned), grid-stride over at most VIBO_PTRAIN_MAX_BLOCKS workgroups of 256 threads, no atomics, fixed order.
 */
#define VIBO_PTRAIN_MAX_BLOCKS 2048
int vibo_person_table_adam(const vibo_desc* d, int mode, int64_t table_rows, const int64_t* index, const float* grad_rows,
                           const float* beta, const float* lr, const int32_t* step_count, float* table_a, float* table_b,
                           float* person_m, float* person_v, int64_t moment_stride, int32_t* slot, int32_t* bad_count,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIBO_HIP_PERSON_TABLES_H */
