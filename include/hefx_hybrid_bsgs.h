/* hefx_hybrid_bsgs.h -- extension of include/hefx_hybrid_hoist.h: a whole baby-step giant-step stage on hybrid keys in ONE
 * call, the giant steps hoisted (the second half of double hoisting: Bossuat, Mouchet, Troncoso-Pastoriza, Hubaux, Eurocrypt
 * 2021, Alg. 6).  The inner sums of the combine entry stay in the extended basis; only their c1 is brought down and switched,
 * in the extended basis again; c0 rides along under the automorphism; every output is mod-downed ONCE.  Same library, same
 * conventions as hefx_hybrid_hoist.h: device pointers, NTT form, canonical words in and out, asynchronous on the caller's
 * stream, scratch is the context's, the constants of (alpha, L) travel through the descriptor ring, and the entry never waits
 * for the device: the kernels compute the automorphism's index.  A header of its own because the test suite enumerates
 * hefx_hybrid_hoist.h.  The entry is held to stream order, alone and behind other users of the context's scratch, by
 * tests/test_gpu_streams_ext.py.
 *
 * THE INTEGER STATEMENT.  Notation of hefx_hybrid.h and hefx_hybrid_hoist.h: level L, alpha, R = [0, L) u S, P, MD (step 5),
 * pi_g, the terms t = i m + k and their A_t.
 *
 * Inner sums.  B_o[c][r] for o < G, r in R is the combine's sum of hefx_hybrid_hoist.h, unchanged:
 *   B_o[c][r] = sum_t pt[o][t][r] A_t[c][r] mod q_r over the terms whose plaintext is not NULL.
 *
 * Giant step.  For an inner sum with a giant key K' and element g (odd, below 2N):
 *   d_o = MD(B_o[1])                                -- step 5 of hefx_hybrid.h on that ONE polynomial, [L][N];
 *   F_{o,j}[r], r in R = the digits of d_o          -- steps 1-3 of hefx_hybrid.h applied to x = d_o, NOT permuted;
 *   W_o[c][r] = sum_j pi_g(F_{o,j}[r]) K'[j][c][r] + [c = 0] pi_g(B_o[0][r])  mod q_r   for EVERY r in R.
 * The special rows are included: B_o[0] is not zero there.  No factor P is applied: B_o[0] carries it already.
 * For an inner sum with a NULL giant key (its element must be 1): W_o = B_o.
 *
 * Outputs.  out[q] = (MD(sum_{dest[o] = q} W_o[0]), MD(sum_{dest[o] = q} W_o[1])) for q < O, the sums mod q_r row by row.
 * Every output has at least one inner sum.
 *
 * WHY.  Write B_o = (b0, b1) over the modulus Q_L P; it decrypts (b0 + b1 s) to P times the inner sum's plaintext.  Only
 * the part that multiplies s has to change hands under the automorphism: pi_g(b0) + pi_g(b1) pi_g(s).  A key switch takes an
 * operand over Q_L, so b1 is divided by P first (d_o), and K' gives back P d_o pi_g(s) + noise over Q_L P: the same modulus
 * b0 lives in.  b0 needs no switch and no division, so it is gathered as it is, special rows included, and the sum of all
 * giant terms of an output is divided by P once.
 *
 * NOISE.  One source, the identity baby term, plaintext 1, r giant terms into one output; s the secret, |s|_1 <= N.
 *   - d_o = b1 / P + eps, |eps| <= alpha per coefficient (rounding 1/2, and the uncorrected conversion of hefx_hybrid.h
 *     step 5 stands for an integer in [0, alpha P): at most alpha - 1 multiples of P) -- bounded by alpha + 1 below.
 *   - W_o[0] + W_o[1] pi_g(s) = pi_g(b0) + P pi_g(d_o) pi_g(s) + E_o, E_o the switch's digit-times-key-noise sum, the one
 *     hefx_hybrid.h's switch has; after the division by P it is within that switch's bound B per giant term.
 *   - P d_o s = b1 s + P eps s: after the division, eps s, at most (alpha + 1) N per coefficient and giant term.
 *   - the final MD adds at most alpha per coefficient of each polynomial, alpha (1 + N) through 1 and s.
 *   max |dec(out) - sum pi_g(dec(ct))| <= r (B + (alpha + 1) N) + alpha (1 + N).
 *
 * Row transforms of a call, dn = ceil(L/alpha): the sources' digits n (L + dn (L + alpha)) as in hefx_hybrid_hoist.h; per
 * giant-rotated inner sum alpha inverse (the special rows of b1), L forward (its spread), L inverse and dn (L + alpha)
 * forward (the digits of d_o): alpha + L + L + dn (L + alpha); per output 2 alpha inverse and 2 L forward.
 *
 * WORKSPACE.  The context's scratch, in rows of N words; x = 2 at poly_degree 32768, else 1; T = n m terms; Gr the inner
 * sums with a giant key.  Fixed:
 *   n L + x n dn (L + alpha) + 2 T (L + alpha) + 2 G (L + alpha) + 2 O L + x 2 O alpha + x 2 O L
 * (the last three blocks are the output accumulators W and their spread).  The accumulators carry across inner sums, so
 * the giant phase runs in chunks of C <= Gr giant-rotated inner sums, each chunk taking
 *   (C + C mod 2) alpha + x (C + C mod 2) L + 2 C L + x C dn (L + alpha).
 * C is the largest count for which fixed + chunk stays within 1 GiB (the chunk rule of hefx_hybrid.h).  A call is refused
 * with HEFX_ERR_UNSUPPORTED, before anything is submitted, only when C = 1 does not fit.
 */
#ifndef HEFX_HYBRID_BSGS_H
#define HEFX_HYBRID_BSGS_H

#include "hefx_hybrid_hoist.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of hefx_hybrid_plain_combine_hoisted up to d_pts ([G][n * m]) describe the G inner sums.  Inner sum o is
 * rotated by giant_elts[o] with d_giant_keys[o] ([dnum][2][k][N], digits 0 .. ceil(L/alpha) - 1 read; NULL with the element
 * 1: no giant rotation) and added into output dest[o]; d_ct_out[q] = [2][L][N] for q < O.
 * HEFX_ERR_INVALID before anything is submitted, and a refused call writes nothing: every refusal of the combine entry
 * (alpha, L, n, m, n * m, a null pointer, an even or too large element, a NULL key with an element other than 1, an inner sum
 * with no term); O < 1, O > G, G > HEFX_HYBRID_HOIST_MAX_OUT; dest[o] outside [0, O); an output with no inner sum; an even
 * or too large giant element; a NULL giant key with an element other than 1, a giant key with the element 1; and the
 * aliasing rule: an output may overlap, in BYTES, no input, not the read digits of a key or of a giant key, no plaintext
 * and no other output. */
int hefx_hybrid_bsgs_hoisted(hefx_context *ctx, int alpha, int L, int n, const uint64_t *const *d_ct_in, int m,
                             const uint32_t *galois_elts, const uint64_t *const *d_keys, int G, const uint64_t *const *d_pts,
                             const uint32_t *giant_elts, const uint64_t *const *d_giant_keys, const uint32_t *dest, int O,
                             uint64_t *const *d_ct_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_HYBRID_BSGS_H */
