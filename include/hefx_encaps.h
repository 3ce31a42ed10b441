/* hefx_encaps.h -- extension of the C-ABI in hefx.h: sparse-secret encapsulation for CKKS bootstrapping (Bossuat,
 * Troncoso-Pastoriza, Hubaux, ACNS 2022).  Same library (libhefx.so), same conventions as hefx.h and hefx_refresh.h: device
 * pointers, NTT form, canonical words, asynchronous on the caller's stream, scratch is the context's, tables travel in
 * kernel arguments.  A header of its own for the reason hefx_refresh.h gives: two tables of the test suite enumerate hefx.h.
 *
 * The scheme.  The program runs under a dense secret s.  At the last prime q_0 the ciphertext is switched to an auxiliary
 * SPARSE secret s' (hefx_switch_key at L = 1, with a key that lives at q_0 P only), raised to the top of the chain under s'
 * -- the integer part I of the raised plaintext m + q_0 I, and with it EvalMod's range K, depend on the weight of s' alone
 * -- and switched back to s there.  hefx_raise_switch does the last two steps in one call, and cheaply: the polynomial
 * raised from ONE prime has centred coefficients |x| < q_0 / 2, which is already "one digit", so the return switch needs no
 * RNS decomposition.  With Kc = sum_{j<L} key_j, the COLLAPSED key (hefx_collapse_key; the row-wise sum of the switching
 * key's digits, itself an encryption of P s' with noise sum_j e_j), the switch is moddown(x Kc).
 *
 * poly_degree 2048 .. 32768 -- this extension serves the one ring hefx_mod_raise does not.
 * The three entries are held to stream order by tests/test_gpu_streams_ext.py.
 */
#ifndef HEFX_ENCAPS_H
#define HEFX_ENCAPS_H

#include "hefx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = (c0 + ks0(c1), ks1(c1)): the key switch of hefx_apply_galois without an automorphism (its Galois element 1), the
 * words of SEAL's switch_key_inplace on c1 added to (c0, 0).  d_ct_in, d_ct_out = [2][L][N], d_key = [k-1][2][k][N] of
 * which digits 0 .. L-1 are read, 1 <= L <= k - 1.  d_ct_out == d_ct_in exactly is allowed (served from a scratch copy);
 * any other overlap of d_ct_out with d_ct_in, or any with the L digits of d_key, in BYTES: HEFX_ERR_INVALID before
 * anything is submitted. */
int hefx_switch_key(hefx_context *ctx, int L, const uint64_t *d_ct_in, const uint64_t *d_key, uint64_t *d_ct_out,
                    void *stream);

/* The collapsed key of level L: out[c][m] = sum_{j<L} key[j][c][m] mod q_m for m = 0 .. L-1, and out[c][L] the same sum
 * over the special prime's row k-1.  d_key = [k-1][2][k][N], d_out = [2][L+1][N], 1 <= L <= k - 1.  One element-wise
 * launch; run once per (key, level).  d_out may not overlap the L digits of d_key in BYTES: HEFX_ERR_INVALID before
 * anything is submitted. */
int hefx_collapse_key(hefx_context *ctx, int L, const uint64_t *d_key, uint64_t *d_out, void *stream);

/* Mod-raise from one prime and key switch with a collapsed key, fused.  d_ct_in = [2][1][N] (c0, c1 at q_0),
 * d_ckey = [2][L_out+1][N] (hefx_collapse_key at L_out), d_ct_out = [2][L_out][N]; 2 <= L_out <= k - 1.
 *
 * The integer statement, P = q_(k-1):
 *   x   = the centred lift of c1 from q_0 by hefx_mod_raise's rule: a coefficient v <= floor(q_0 / 2) stands for v,
 *         otherwise for v - q_0;
 *   acc[c][m] = NTT_m(x mod q_m) * ckey[c][m] mod q_m        over m in {0 .. L_out-1, P}, c in {0, 1};
 *   the mod-down is the key switch's own (SEAL's switch_key_inplace): u = INTT_P(acc[c][P]); u = (u + floor(P/2)) mod P;
 *   t_j = (u mod q_j) - (floor(P/2) mod q_j);  md[c][j] = (acc[c][j] - NTT_j(t_j)) * P^-1 mod q_j;
 *   out[0] = md[0] + the centred lift of c0 (row j: NTT_j of it),  out[1] = md[1].  Canonical words.
 * These are the words of the ordinary key switch (hefx_switch_key at L_out) run on x written as two digits
 * x = c1 - q_0 neg (neg the 0/1 polynomial of the coefficients above floor(q_0 / 2)) against the two-digit key
 * (Kc, -q_0 Kc): every modulus sees x Kc.
 *
 * Row transforms: 2 inverse (c0, c1 at q_0) + 2 (L_out - 1) + 1 forward (x at q_1 .. q_(L_out-1) and P, c0's lift at
 * q_1 .. q_(L_out-1); row 0 of both is the input's own NTT row) + 2 inverse at P + 2 L_out forward (the t_j)
 * = 4 L_out + 3, linear in L_out, where the ordinary key switch of the raised ciphertext takes about L_out^2 + 5 L_out.
 *
 * d_ct_out may overlap neither d_ct_in nor d_ckey in BYTES (d_ct_out == d_ct_in included): HEFX_ERR_INVALID before
 * anything is submitted. */
int hefx_raise_switch(hefx_context *ctx, int L_out, const uint64_t *d_ct_in, const uint64_t *d_ckey, uint64_t *d_ct_out,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_ENCAPS_H */
