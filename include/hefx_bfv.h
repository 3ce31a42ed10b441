/* hefx_bfv.h -- extension of the C-ABI in hefx.h: the operations that are specific to BFV, exact and on the device -- the
 * tensor product scaled by t/Q (Evaluator::multiply / square on BFV ciphertexts), the rounding of decryption, and the rest
 * of the scheme's arithmetic: a message scaled by Delta and added to c_0 (encryption, add_plain), the centred lift of a
 * message into every row (multiply_plain), the invariant noise budget, and BatchEncoder's slot transform modulo t.
 * Same library (libhefx.so), same conventions as hefx.h: device pointers, canonical words, asynchronous on the caller's
 * stream, no host wait, HEFX_ERR_INVALID before anything is submitted.  UNLIKE hefx.h, the polynomials here are in
 * COEFFICIENT form: that is how a BFV ciphertext is kept (include/seal/seal.h).
 *
 * Why a header of its own: for the reason stated at the top of hefx_refresh.h -- two tables of the test suite enumerate
 * hefx.h, and the change that added these entries could not touch either.
 *
 * Definitions.  Q = q_0 ... q_(L-1), the first L primes of the context (odd).  t is the plain modulus.
 *   - A word vector x[L][N] in coefficient form stands, per coefficient, for the centred integer x^: x when
 *     x <= floor(Q/2), otherwise x - Q (the rule of hefx_mod_raise).
 *   - R(z) = sign(z) * floor((t |z| + (Q-1)/2) / Q): t z / Q rounded to nearest; Q is odd, so there are no ties.
 *   - Delta = floor(Q / t).
 * Every entry is exact: its words are this mathematical function of its inputs, whatever the method.
 *
 * Method (csrc/hefx_bfv.hip): a working basis of the L data primes followed by auxiliary primes just below 2^60, wide
 * enough to hold t (z + K Q) + (Q-1)/2 without wrap-around, where |z| < 3 N (Q/2)^2 for a product and K = N Q; the
 * operands are extended to it exactly (the lift of hefx_mod_raise), multiplied through the NTT, and the quotient by Q is
 * read off the upper mixed-radix digits.  The noise budget takes the mixed-radix digits of t x mod Q, complements them when
 * they lie above those of (Q-1)/2, and reduces the bit length of the magnitude over the polynomial.  The slot transform is
 * the engine's own negacyclic NTT over a one-prime context {t} that the object owns.  No floating point and no division
 * anywhere.
 *
 * Scratch and streams.  The working basis, its tables and the scratch belong to the hefx_bfv OBJECT.  Two objects may be
 * used on two streams at once.  ONE object on two streams at once (or from two host threads at once) is the caller's
 * error: its calls must be ordered on the device, like those of one hefx_context.
 *
 * Unsupported shapes (hefx_bfv_create answers HEFX_ERR_UNSUPPORTED): poly_degree 32768, and an (L, t) whose working
 * basis needs more than HEFX_BFV_MAX_BASIS primes -- the L data primes plus ceil(bits(7 t N Q / 4) / ~60) auxiliary
 * ones.  BFVDefault(4096) (L = 2) and BFVDefault(8192) (L = 4 and every level below) fit with any t < 2^60.
 */
#ifndef HEFX_BFV_H
#define HEFX_BFV_H

#include "hefx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most primes of a working basis (data + auxiliary): the width of the mixed-radix digit arrays */
#define HEFX_BFV_MAX_BASIS 16
/* the most polynomials of a product: size_a + size_b - 1 <= HEFX_BFV_SIZE_MAX (at most three terms per output
 * polynomial: the bound |z| < 3 N (Q/2)^2 the working basis is sized from) */
#define HEFX_BFV_SIZE_MAX 6

typedef struct hefx_bfv hefx_bfv;

/* ctx: the data context (primes q_0 .. q_(k-1)); L: data primes in use, 1 <= L <= the data primes of ctx (k - 1, or 1
 * when k == 1); 2 <= t < 2^60 with gcd(t, q_j) = 1 for j < L, otherwise HEFX_ERR_INVALID.  Builds the working basis (a
 * context of its own over the L data primes and the auxiliary ones), the rounding tables, the per-row constants
 * (Delta mod q_j, t mod q_j), the slot tables when t allows batching, and the scratch of the entries below, on the device
 * of ctx; waits for its own uploads.  ctx must outlive the object. */
int hefx_bfv_create(hefx_context *ctx, int L, uint64_t t, hefx_bfv **out);
/* waits for the device, then frees everything the object owns */
void hefx_bfv_destroy(hefx_bfv *b);
/* auxiliary primes of the working basis (0 for a null object): what create had to add to the L data primes */
int hefx_bfv_aux_count(const hefx_bfv *b);

/* out[k][j][n] = R(c_k[n]) mod q_j for c_k = sum_{i+j=k} a^_i * b^_j in Z[X]/(X^N + 1): d_a = [size_a][L][N],
 * d_b = [size_b][L][N], d_out = [size_a + size_b - 1][L][N], all in coefficient form; each size >= 2 and
 * size_a + size_b - 1 <= HEFX_BFV_SIZE_MAX.  d_a == d_b is allowed (a square).  d_out may overlap neither d_a nor d_b in
 * BYTES (d_out == d_a included): HEFX_ERR_INVALID before anything is submitted.  The inputs are left as they are. */
int hefx_bfv_multiply(hefx_bfv *b, int size_a, const uint64_t *d_a, int size_b, const uint64_t *d_b, uint64_t *d_out,
                      void *stream);

/* m[n] = R(x^[n]) mod t, N words, for d_x = [L][N] in coefficient form: the message of a BFV decryption from
 * x = [c_0 + c_1 s + ...]_Q.  d_m may not overlap d_x in BYTES (d_m == d_x included): HEFX_ERR_INVALID before anything
 * is submitted.  d_x is left as it is. */
int hefx_bfv_decrypt_round(hefx_bfv *b, const uint64_t *d_x, uint64_t *d_m, void *stream);

/* out[j][n] = (c0_in[j][n] + (Delta mod q_j) * (m[n] mod q_j)) mod q_j for n < ncoeff and out[j][n] = c0_in[j][n] for
 * ncoeff <= n < N: what encryption and add_plain add to c_0.  d_m holds ncoeff words, 1 <= ncoeff <= N; d_c0_in and d_out
 * are [L][N]; d_c0_in may be NULL, which stands for zeros.  d_out == d_c0_in exactly is allowed (the operation is
 * element-wise); d_out may not overlap d_c0_in in any other way, nor d_m, in BYTES: HEFX_ERR_INVALID before anything is
 * submitted.  The inputs are left as they are (d_c0_in unless it is d_out). */
int hefx_bfv_scale_plain_add(hefx_bfv *b, const uint64_t *d_m, int ncoeff, const uint64_t *d_c0_in, uint64_t *d_out,
                             void *stream);

/* out[j][n] = m[n] mod q_j when m[n] <= floor(t/2), otherwise q_j - ((t - m[n]) mod q_j), for n < ncoeff; zeros for
 * ncoeff <= n < N: the message as a ring element with centred coefficients, d_out = [L][N].  ntt_form != 0: the rows are
 * then transformed forward -- the operand hefx_multiply_plain takes.  d_m holds ncoeff words, 1 <= ncoeff <= N.  d_out
 * may not overlap d_m in BYTES: HEFX_ERR_INVALID before anything is submitted.  d_m is left as it is. */
int hefx_bfv_lift_plain(hefx_bfv *b, const uint64_t *d_m, int ncoeff, int ntt_form, uint64_t *d_out, void *stream);

/* *d_budget (one 32-bit word) = max(0, bits(Q) - bits(W) - 1) with W = max_n |v[n]|, v[n] the centred representative of
 * t x^[n] mod Q and bits(0) = 0, for d_x = [L][N] in coefficient form (as for hefx_bfv_decrypt_round): the invariant
 * noise budget.  d_budget may not overlap d_x in BYTES: HEFX_ERR_INVALID before anything is submitted.  d_x is left as it
 * is. */
int hefx_bfv_noise_budget(hefx_bfv *b, const uint64_t *d_x, uint32_t *d_budget, void *stream);

/* 1 when t is prime and t = 1 mod 2N (the object then owns a one-prime context over {t}), else 0; 0 for a null object */
int hefx_bfv_batching(const hefx_bfv *b);

/* d_m[N] = the polynomial modulo t with m(psi^(e_i)) = values[i] mod t for i < nvalues and 0 in the other slots, where psi
 * is the minimal primitive 2N-th root modulo t, e_i = 3^i mod 2N for i < N/2 and e_(N/2+i) = -3^i mod 2N.  d_values holds
 * nvalues words, 1 <= nvalues <= N.  HEFX_ERR_UNSUPPORTED when hefx_bfv_batching(b) is 0.  d_m may not overlap d_values
 * in BYTES: HEFX_ERR_INVALID before anything is submitted.  d_values is left as it is. */
int hefx_bfv_batch_encode(hefx_bfv *b, const uint64_t *d_values, int nvalues, uint64_t *d_m, void *stream);

/* the inverse: values[i] = m(psi^(e_i)) for all N slots, d_m = [N] words below t, d_values = [N].  HEFX_ERR_UNSUPPORTED
 * when hefx_bfv_batching(b) is 0.  d_values may not overlap d_m in BYTES: HEFX_ERR_INVALID before anything is submitted.
 * d_m is left as it is. */
int hefx_bfv_batch_decode(hefx_bfv *b, const uint64_t *d_m, uint64_t *d_values, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_BFV_H */
