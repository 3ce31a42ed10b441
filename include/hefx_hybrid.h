/* hefx_hybrid.h -- extension of the C-ABI in hefx.h: hybrid key switching (Han and Ki, CT-RSA 2020): alpha data primes per
 * RNS digit and alpha special primes, beside the scheme of hefx.h (one digit per data prime, one special prime), whose entries
 * and kernels are untouched.  Same library (libhefx.so), same conventions as hefx.h and hefx_encaps.h: device pointers, NTT
 * form, canonical words, asynchronous on the caller's stream, scratch is the context's.  A header of its own for the reason
 * hefx_refresh.h gives: two tables of the test suite enumerate hefx.h.
 *
 * THE INTEGER STATEMENT.  A context has primes q_0 .. q_(k-1).  alpha lies in 1 .. HEFX_HYBRID_ALPHA_MAX and below k.  The
 * special rows are S = {k-alpha .. k-1}, P their product; there are D = k - alpha data primes and dnum = ceil(D / alpha)
 * digits; digit j owns the data rows G_j = {j alpha .. min((j+1) alpha, D) - 1}.  At level L (1 <= L <= D) the digits are
 * j < ceil(L / alpha), G_j(L) = G_j cut to [0, L), D_j(L) = prod_{i in G_j(L)} q_i, Dhat_i = D_j(L) / q_i: the last digit may
 * be partial, so the constants depend on (alpha, L).
 *
 * Key, [dnum][2][k][N]:  key[j] = (-(a_j s + e_j) + F_j (.) s', a_j) over all k rows, F_j[m] = P mod q_m for m in G_j and 0
 * in every other row, the special rows included; a_j is polynomial j of a dnum-polynomial uniform draw from sub-stream
 * 2 stream_id, e_j the same of the noise from 2 stream_id + 1.  At alpha = 1 these are the words of hefx_keygen_kswitch.
 *
 * Switch of a polynomial x ([L][N], NTT form) to ks[c], c in {0, 1}:
 *   1. x~ = INTT of the L rows.
 *   2. per digit j, coefficient by coefficient:  y_i = x~_i (Dhat_i^-1 mod q_i) mod q_i for i in G_j(L);  for every target
 *      m in ([0, L) \ G_j(L)) u S:  ext_j[m] = sum_i y_i (Dhat_i mod q_m) mod q_m  -- fast base conversion with no correction
 *      term: the integer it stands for lies in [0, alpha D_j(L)).  For m in G_j(L) the NTT-form row of ext_j is x's own row m.
 *   3. forward NTT of the converted rows.
 *   4. acc[c][m] = sum_j ext_j[m] key[j][c][m] mod q_m for m in [0, L) u S.
 *   5. mod-down with rounding.  For t in S: u_t = INTT(acc[c][t]); u_t <- (u_t + (floor(P/2) mod q_t)) mod q_t;
 *      z_t = u_t ((P/q_t)^-1 mod q_t) mod q_t.  For j < L: v_j = sum_t z_t ((P/q_t) mod q_j) mod q_j;
 *      t_j = v_j - (floor(P/2) mod q_j) mod q_j;  ks[c][j] = (acc[c][j] - NTT_j(t_j)) P^-1 mod q_j.  Canonical words.
 * At alpha = 1 steps 2 and 5 collapse (y = x~, z = u) to the digit lift and the (u + floor(P/2)) mod P mod-down of the key switch
 * of hefx.h: the words are those of hefx_switch_key / hefx_apply_galois / hefx_relinearize.
 *
 * Row transforms at level L: L inverse (step 1), ceil(L/alpha)(L + alpha) - L forward over converted rows (step 3),
 * 2 alpha inverse and 2 L forward (step 5): 168 at L = 20, alpha = 4, where hefx.h's scheme takes about L^2 + 5 L = 500.
 * This build hands step 3 to the engine's transform in TWO launches, all data rows and all special rows, whose blocks are
 * whole: the L own rows of the digits are transformed along (their result is never read), so step 3 RUNS
 * ceil(L/alpha)(L + alpha) rows, 188 in all at L = 20, alpha = 4.
 *
 * HEFX_HYBRID_ALPHA_MAX.  The 128-bit sums would allow more (a sum of alpha products of words below 2^61 needs
 * alpha 2^122 < 2^128, the MAC over ceil(L/alpha) <= 61 digits fits for every alpha >= 1); 8 is what a lane holds in registers
 * (2 alpha words of y_i / z_t) and what a chain of at most 62 primes can use: beyond 8 the digits gain nothing on the special
 * rows they add.
 *
 * HOST.  The constants of a pair (alpha, L) -- Dhat_i^-1, Dhat_i mod q_m, (P/q_t)^-1, (P/q_t) mod q_j, floor(P/2) and P^-1 mod
 * every row: (L + 2 alpha + 5) L + 3 alpha words -- are computed on the host at the first use of the pair and kept with the
 * context; every call copies them, with its item table, through the context's descriptor ring in front of its launches.  NO
 * entry of this header waits for the device, at first use or later (beyond what hefx.h says of a full descriptor ring and
 * of a scratch buffer that cannot grow): no gather table is built, the kernels compute the automorphism's index.
 * The entries are held to stream order -- operands that arrive on the caller's stream, a wrap of the descriptor ring, scratch
 * growth and a chunked call behind a shut stream -- by tests/test_gpu_streams_ext.py.
 *
 * poly_degree 2048 .. 32768.  Batches are cut into chunks whose workspace stays below 1 GiB (one item at least).
 * No security claim: alpha special primes add their bits to QP -- {60, 50 x 13, 60, 60} at N = 32768 is 830 of the 881 bits of
 * the HE-standard table, a third 60-bit special prime would exceed it.
 */
#ifndef HEFX_HYBRID_H
#define HEFX_HYBRID_H

#include "hefx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HEFX_HYBRID_ALPHA_MAX 8

/* dnum = ceil((k - alpha) / alpha), the digits of a hybrid key of this context; HEFX_ERR_INVALID for alpha outside
 * 1 .. min(k - 1, HEFX_HYBRID_ALPHA_MAX), HEFX_ERR_UNSUPPORTED below poly_degree 2048. */
int hefx_hybrid_digits(hefx_context *ctx, int alpha);

/* The hybrid switching key for the secret d_new_sk under d_sk (both [k][N]), d_out = [dnum][2][k][N], as stated above;
 * key32, stream_id as hefx_keygen_kswitch (stream_id below 2^62).  d_out may overlap neither secret in BYTES:
 * HEFX_ERR_INVALID before anything is submitted. */
int hefx_hybrid_keygen(hefx_context *ctx, int alpha, const uint64_t *d_sk, const uint64_t *d_new_sk, const uint8_t *key32,
                       uint64_t stream_id, uint64_t *d_out, void *stream);

/* n independent items, the batch convention of hefx_apply_galois_batch:
 *   d_ct_out[i] = (pi_g(c0) + ks0(pi_g(c1)), ks1(pi_g(c1))),  (c0, c1) = d_ct_in[i], g = galois_elts[i] (odd, below 2N),
 * pi_g the NTT-domain gather of hefx_galois_permute; the element 1 is the plain switch.  d_ct_in[i], d_ct_out[i] = [2][L][N],
 * d_keys[i] = [dnum][2][k][N] of which digits 0 .. ceil(L/alpha) - 1 are read; 1 <= L <= k - alpha.
 * HEFX_ERR_INVALID before anything is submitted: alpha < 1, alpha >= k, alpha > HEFX_HYBRID_ALPHA_MAX, L outside
 * 1 .. k - alpha, n < 1, a null pointer, an even or too large element, and the aliasing rule -- d_ct_out[i] == d_ct_in[i]
 * exactly is allowed (both polynomials are staged before anything is written); any other overlap in BYTES of an output
 * with an output, with an input (another item's included) or with the read digits of a key is refused. */
int hefx_hybrid_apply_galois_batch(hefx_context *ctx, int alpha, int L, int n, const uint64_t *const *d_ct_in,
                                   const uint32_t *galois_elts, const uint64_t *const *d_keys, uint64_t *const *d_ct_out,
                                   void *stream);

/* n relinearisations from size 3 with one key (of s^2):  d_ct2[i] = (c0 + ks0(c2), c1 + ks1(c2)),  (c0, c1, c2) = d_ct3[i]
 * = [3][L][N], d_ct2[i] = [2][L][N].  Errors as above; the aliasing rule is hefx_relinearize's: an output may overlap no
 * input (its own included, d_ct2[i] == d_ct3[i] too), no other output and not the read digits of the key, in BYTES. */
int hefx_hybrid_relinearize_batch(hefx_context *ctx, int alpha, int L, int n, const uint64_t *const *d_ct3,
                                  const uint64_t *d_key, uint64_t *const *d_ct2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_HYBRID_H */
