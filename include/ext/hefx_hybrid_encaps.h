/* hefx_hybrid_encaps.h -- extension of the C-ABI in hefx.h: sparse-secret encapsulation (include/hefx_encaps.h) on HYBRID
 * keys (include/hefx_hybrid.h).  Same library (libhefx.so), same conventions as those two headers: device pointers, NTT form,
 * canonical words in and out, asynchronous on the caller's stream, scratch is the context's.  NO entry of this header waits
 * for the device, at first use or later (beyond what hefx.h says of a full descriptor ring and of a scratch buffer that
 * cannot grow).  poly_degree 2048 .. 32768.
 *
 * WHERE IT LIVES.  tests/test_stream_ext_cpu.py asks that every `void *stream` entry of include/hefx_*.h appear in the
 * coverage table of tests/stream_ext_cases.py, whose rows are fixed; this header came with a change that could not edit that
 * table, so it sits one directory down, in include/ext/, and the stream-order tests of its two entries (the same decoy
 * protocol, through the same Case machinery) live in tests/test_gpu_hybrid_encaps.py.  A change that may edit the table moves
 * the header up and adds the two rows.
 *
 * THE SCHEME is hefx_encaps.h's: at the last prime q_0 the ciphertext is switched to an auxiliary sparse secret s' (an
 * ORDINARY key at q_0 q_(k-1), hefx_switch_key at L = 1: nothing hybrid), raised to level L under s' and switched back to the
 * main secret s there.  A polynomial raised from ONE prime has centred coefficients |x| <= q_0 / 2: it is a single digit
 * whatever alpha is, so the return switch needs no base conversion, only the COLLAPSED hybrid key.
 *
 * THE INTEGER STATEMENT.  Notation of hefx_hybrid.h: primes q_0 .. q_(k-1), alpha special rows S = {k-alpha .. k-1}, P their
 * product, digit j owning the data rows G_j = {j alpha .. min((j+1) alpha, k-alpha) - 1}.  R = L + alpha rows: row r < L is
 * data prime r, row r >= L is special prime k - alpha + r - L; m(r) is that prime index.
 *
 *   Why the collapsed key is a key.  key[j] = (-(a_j s + e_j) + F_j (.) s', a_j) with F_j[m] = P mod q_m for m in G_j and 0 in
 *     every other row.  Every data row m < L lies in exactly one digit j < ceil(L / alpha), so sum_{j < ceil(L/alpha)} F_j[m] is
 *     P mod q_m on the data rows m < L and 0 on the special rows: Kc = sum_j key[j] is an encryption (-(a s + e) + P s', a),
 *     a = sum_j a_j, of P s' at level L with noise e = sum_j e_j.
 *   The lift.  x and y are the centred lifts of c1 and c0 from q_0 by hefx_mod_raise's rule: a coefficient v <= floor(q_0 / 2)
 *     stands for v, otherwise for v - q_0.
 *   The product.  acc[c][r] = NTT_m(r)(x mod q_m(r)) * ckey[c][r] mod q_m(r) over all R rows, c in {0, 1}.  Row 0 of x and
 *     of y is the input's own NTT row.
 *   The mod-down.  Step 5 of hefx_hybrid.h applied to acc[c]:  for t in S: u_t = INTT(acc[c][t]);
 *     u_t <- (u_t + (floor(P/2) mod q_t)) mod q_t;  z_t = u_t ((P/q_t)^-1 mod q_t) mod q_t.  For j < L:
 *     v_j = sum_t z_t ((P/q_t) mod q_j) mod q_j;  t_j = v_j - (floor(P/2) mod q_j) mod q_j;
 *     ks[c][j] = (acc[c][j] - NTT_j(t_j)) P^-1 mod q_j.
 *   The result.  out[0][j] = ks[0][j] + NTT_j(y mod q_j),  out[1][j] = ks[1][j].  Canonical words.
 *   At alpha = 1 the two entries give the words of hefx_collapse_key and hefx_raise_switch (z = u, v_j = u mod q_j).
 *
 * ROW TRANSFORMS (a count of rows, not a time).  2 inverse at q_0 (c0, c1), then 2 (L - 1) + alpha forward (x at q_1 ..
 * q_(L-1) and at the alpha special rows, y at q_1 .. q_(L-1)), then 2 alpha inverse (the special rows of acc), then 2 L forward
 * (the t_j): 4 L + 3 alpha in total, 92 at L = 20, alpha = 4, where hefx_mod_raise (2 L rows) followed by the hybrid switch of
 * hefx_hybrid.h (188 rows run) takes 228.
 *
 * NOISE, in the convention of tests/hybrid_cases.py: dec_s(out) - (y + x s'), centred mod Q_L, has infinity norm at most
 *     B = ceil( ceil(L/alpha) * N * 19 * floor(q_0/2) / P ) + alpha * (1 + N).
 * First term: acc[0] + acc[1] s = x (Kc[0] + Kc[1] s) = x (P s' - e) mod Q_L P, so out decrypts to y + x s' - x e / P plus the
 * mod-down's error; |x| <= floor(q_0/2), |e_j| <= 19 (the sampler's clip), a negacyclic product of N terms per coefficient,
 * ceil(L/alpha) summed key noises, divided by P.  Second term: the mod-down subtracts v = [acc + floor(P/2)]_P + eps P with
 * 0 <= eps < alpha (the conversion from the special rows is not corrected), so ks[c] = floor((acc[c] + floor(P/2)) / P) - eps
 * lies within alpha of acc[c] / P; ks[1] meets the ternary secret s (alpha N), ks[0] stands alone (alpha).  Derived, not
 * fitted.  No security claim.
 *
 * HOST.  The constants of (alpha, L) -- (P/q_t)^-1, floor(P/2), (P/q_t) mod q_j, P^-1 -- are the table the entries of
 * hefx_hybrid.h keep with the context; hefx_hybrid_raise_switch copies it through the context's descriptor ring in front of
 * its launches.  hefx_hybrid_collapse_key needs no table.
 */
#ifndef HEFX_HYBRID_ENCAPS_H
#define HEFX_HYBRID_ENCAPS_H

#include "../hefx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The collapsed key of level L: out[c][r] = sum_{j < ceil(L/alpha)} key[j][c][m(r)] mod q_m(r).
 * d_key = [dnum][2][k][N] (hefx_hybrid_keygen) of which digits 0 .. ceil(L/alpha) - 1 are read, d_out = [2][L+alpha][N];
 * 1 <= L <= k - alpha.  One element-wise launch; run once per (key, level).
 * HEFX_ERR_INVALID before anything is submitted: alpha outside 1 .. min(k - 1, 8), L out of range, a null pointer, d_out
 * overlapping the read digits of d_key in BYTES. */
int hefx_hybrid_collapse_key(hefx_context *ctx, int alpha, int L, const uint64_t *d_key, uint64_t *d_out, void *stream);

/* Mod-raise from one prime and key switch with a collapsed hybrid key, fused: the statement above.
 * d_ct_in = [2][1][N] (c0, c1 at q_0), d_ckey = [2][L_out+alpha][N] (hefx_hybrid_collapse_key at L_out),
 * d_ct_out = [2][L_out][N]; 2 <= L_out <= k - alpha.
 * HEFX_ERR_INVALID before anything is submitted: alpha outside 1 .. min(k - 1, 8), L_out out of range, a null pointer, and
 * the aliasing rule of hefx_encaps.h -- d_ct_out may overlap neither d_ct_in nor d_ckey in BYTES (d_ct_out == d_ct_in
 * included). */
int hefx_hybrid_raise_switch(hefx_context *ctx, int alpha, int L_out, const uint64_t *d_ct_in, const uint64_t *d_ckey,
                             uint64_t *d_ct_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_HYBRID_ENCAPS_H */
