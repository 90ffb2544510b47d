/*
 * vibo_hip_decoder_multi.h -- the multi-sample forward of the per-term MLP decoders: two more exports of libvibo_hip.so,
 * declared beside vibo_hip.h (its types, constants and conventions; include that header first or let this one do it).
 * vibo_amd/_lib.py binds them from this file as it binds the others from vibo_hip.h.
 */
#ifndef VIBO_HIP_DECODER_MULTI_H
#define VIBO_HIP_DECODER_MULTI_H

#include "vibo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The forward of vibo_decoder_fwd_bwd (d->want_grad must be 0, else -5) for num_samples stacked samples in ONE launch:
 * log_marginal's importance samples and posterior_predictive's draws of the --generative-model link | deep | residual models.
 * Per sample s the network of vibo_decoder_fwd_bwd is evaluated on
 *     U [num_samples][I][64] (or NULL),  V [num_samples][B][64],  L [num_samples][B][I] (or NULL),  guess [num_samples][I] (or NULL);
 * w1, W2, b2, w3, b3 and d->resid are shared by the samples, and so are the response / mask rows (strides in d).
 *   ll_part [num_samples][n_wave]   n_wave = 4 ceil(I / 64) d->person_chunks records per sample, each the bits of the record
 *                                   vibo_decoder_fwd_bwd writes for that sample alone with the same person_chunks (sum them per sample)
 *   prob_sum                        optional [B][I]: sum over the samples of P(response = 1), added cell by cell in sample order (the
 *                                   bits of adding the prob_out of num_samples single calls in that order).  prob_accumulate = 0: the
 *                                   call's first sample overwrites the cell; != 0: it adds onto what the caller left there (a
 *                                   sum continued over several calls).  Cells outside [B][I] are not touched.
 * Every ll_part record is fully overwritten.  d->person_chunks: any value in 1..B; vibo_decoder_multi_person_chunks(B, I,
 * num_samples) fills the chip with the samples' own parallelism counted in (fewer chunks as num_samples grows; between 1 and
 * (B + 1) / 2; 0 for an empty shape).  With prob_sum one workgroup owns a cell for all samples, so the samples supply no
 * parallelism there: vibo_decoder_person_chunks(B, I) is the value to pass.
 * Returns as vibo_decoder_fwd_bwd, checked before anything is launched and with vibo_last_error_string set: -1 NULL descriptor;
 * -2 num_person, num_item or num_samples < 1; -6 hidden_dim != 64; -3 person_chunks outside 1..B; -5 a required pointer
 * (response, V, W2, b2, w3, b3, ll_part) missing, w1 or resid without L, or want_grad != 0; -4 U or V not 16-byte aligned.
 */
int vibo_decoder_multi_person_chunks(int num_person, int num_item, int num_samples);
int vibo_decoder_multi_forward(const vibo_decoder_desc* d, int num_samples,
                               const float* response, const uint8_t* mask,
                               const float* U, const float* V, const float* L, const float* guess, const float* w1,
                               const float* W2, const float* b2, const float* w3, const float* b3,
                               float* ll_part, float* prob_sum, int prob_accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIBO_HIP_DECODER_MULTI_H */
