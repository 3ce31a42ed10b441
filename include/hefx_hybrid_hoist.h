/* hefx_hybrid_hoist.h -- extension of include/hefx_hybrid.h: hoisted hybrid key switching.  Many rotations of the same
 * ciphertext share ONE digit decomposition (steps 1-3 of hefx_hybrid.h), and a plaintext-weighted sum of rotated ciphertexts
 * takes ONE mod-down (step 5) per output instead of one per rotation.  Same library, same conventions as hefx_hybrid.h: device
 * pointers, NTT form, canonical words in and out, asynchronous on the caller's stream, scratch is the context's.  A header of
 * its own because the test suite enumerates hefx_hybrid.h.
 *
 * THE INTEGER STATEMENT.  Notation of hefx_hybrid.h: level L, alpha, the rows R = [0, L) u S, P, G_j(L), keys [dnum][2][k][N];
 * pi_g is the NTT-domain gather of hefx_galois_permute.
 *
 * Digits.  For a source ciphertext (c0, c1), E_j[m] with m in R is the output of steps 1-3 of hefx_hybrid.h applied to
 * x = c1, NOT permuted: c1's own NTT row for m in G_j(L), the NTT of the uncorrected base conversion ext_j[m] elsewhere.
 *
 * Term.  For an element g (odd, below 2N) and a key K:
 *   A[c][m] = sum_j pi_g(E_j[m]) K[j][c][m] mod q_m for m in R,  c in {0, 1};
 *   for c = 0 and m < L, (P mod q_m) pi_g(c0[m]) is added.
 * A NULL key requires g = 1 and denotes the identity term: A[c][m] = (P mod q_m) c_c[m] on the data rows, 0 on S.
 *
 * Mod-down.  MD is step 5 of hefx_hybrid.h, unchanged, applied to each polynomial of a pair of R-row polynomials.
 *
 * Hoisted rotation.  out = (MD(A[0]), MD(A[1])).  P c0 is folded in BEFORE MD; because P c0 is 0 on S and MD divides the data
 * rows by P exactly, these are the words of adding pi_g(c0) after it.
 * These are NOT the words of hefx_hybrid_apply_galois_batch, except at g = 1 with a real key: that entry decomposes pi_g(c1),
 * this one permutes the decomposition of c1.  The uncorrected base conversion does not commute with the sign flips of the
 * automorphism (X^i -> +-X^(g i mod N)): the integer ext_j stands for differs, coefficient by coefficient, by a multiple of
 * D_j(L) between the two orders.  Both decrypt to the rotated plaintext: |pi_g(ext_j)| < alpha D_j(L) still, so the noise
 * bound of hefx_hybrid.h's switch holds unchanged.  With a NULL key the output is MD(P c), which is within alpha of c per
 * coefficient (the uncorrected conversion of floor(P/2) from S), not a copy of c.
 *
 * Combine (double hoisting).  For G outputs over the terms t = i m + k (source i < n, element k < m):
 *   B_o[c][m] = sum_t pt[o][t][m] A_t[c][m] mod q_m for m in R, over the terms whose plaintext is not NULL;
 *   out[o] = (MD(B_o[0]), MD(B_o[1])).
 * pt[o][t] is a KEY-LEVEL plaintext [k][N], of which the rows [0, L) u S are read.  One rounding per output: these are not
 * the words of rotate + hefx_multiply_plain + hefx_add_many, which round once per rotation.
 *
 * Row transforms of a call: n L inverse and n ceil(L/alpha)(L + alpha) forward for the digits (run as in hefx_hybrid.h, the
 * own rows transformed along), then 2 alpha inverse and 2 L forward per OUTPUT: n m outputs for the rotate entry, G for the
 * combine entry.
 *
 * WORKSPACE.  The context's scratch, in rows of N words; x = 2 at poly_degree 32768 (a block that a transform reads is held
 * twice there), else 1; T = n m terms, O outputs (T for the rotate entry, G for the combine entry), dn = ceil(L/alpha):
 *   n L  +  x n dn (L + alpha)  +  2 T L  +  xa 2 T alpha  +  [combine: 2 G L + x 2 G alpha]  +  x 2 O L,
 * xa = x for the rotate entry, 1 for the combine entry.  A call whose workspace would pass 1 GiB (the chunk rule of
 * hefx_hybrid.h) is refused with HEFX_ERR_UNSUPPORTED before anything is submitted: no chunking, no environment knob.
 *
 * HOST.  As hefx_hybrid.h: the constants of (alpha, L) are made on the host at the first use of the pair and travel with the
 * call's table through the descriptor ring.  NO entry of this header waits for the device, at first use of an element or of
 * a pair or later: the kernels compute the automorphism's index, no gather or flip table is built.
 * Both entries are held to stream order, operands, plaintexts and keys arriving on the caller's stream behind a shut gate, by
 * tests/test_gpu_streams_ext.py.
 */
#ifndef HEFX_HYBRID_HOIST_H
#define HEFX_HYBRID_HOIST_H

#include "hefx_hybrid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HEFX_HYBRID_HOIST_MAX_TERMS 64 /* n * m */
#define HEFX_HYBRID_HOIST_MAX_OUT 64   /* G */

/* n sources, m elements:  d_ct_out[i * m + k] = the hoisted rotation of d_ct_in[i] by galois_elts[k] with d_keys[k].
 * d_ct_in[i], d_ct_out[.] = [2][L][N]; d_keys[k] = [dnum][2][k][N] of which the digits 0 .. ceil(L/alpha) - 1 are read, or
 * NULL with galois_elts[k] == 1 (the identity term).  HEFX_ERR_INVALID before anything is submitted: alpha or L out of
 * range (hefx_hybrid.h), n < 1, m < 1, n * m > HEFX_HYBRID_HOIST_MAX_TERMS, a null pointer, an even or too large element,
 * a NULL key with an element other than 1, and the aliasing rule: an output may overlap, in BYTES, no input, not the read
 * digits of a key and no other output. */
int hefx_hybrid_rotate_hoisted_batch(hefx_context *ctx, int alpha, int L, int n, const uint64_t *const *d_ct_in, int m,
                                     const uint32_t *galois_elts, const uint64_t *const *d_keys, uint64_t *const *d_ct_out,
                                     void *stream);

/* G outputs over the n * m terms:  d_ct_out[o] = (MD(B_o[0]), MD(B_o[1])), the plaintext of output o and term t = i * m + k
 * at d_pts[o * n * m + t] ([k][N]; NULL: a structural zero, no term).  Errors as above, and: G < 1,
 * G > HEFX_HYBRID_HOIST_MAX_OUT, an output with no term; an output may overlap no plaintext (k N words) either. */
int hefx_hybrid_plain_combine_hoisted(hefx_context *ctx, int alpha, int L, int n, const uint64_t *const *d_ct_in, int m,
                                      const uint32_t *galois_elts, const uint64_t *const *d_keys, int G,
                                      const uint64_t *const *d_pts, uint64_t *const *d_ct_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_HYBRID_HOIST_H */
