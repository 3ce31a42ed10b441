/* hefx_bfv.h -- extension of the C-ABI in hefx.h: the two operations that are specific to BFV, exact and on the device --
 * the tensor product scaled by t/Q (Evaluator::multiply / square on BFV ciphertexts) and the rounding of decryption.
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
 * Both entries are exact: their words are this mathematical function of their inputs, whatever the method.
 *
 * Method (csrc/hefx_bfv.hip): a working basis of the L data primes followed by auxiliary primes just below 2^60, wide
 * enough to hold t (z + K Q) + (Q-1)/2 without wrap-around, where |z| < 3 N (Q/2)^2 for a product and K = N Q; the
 * operands are extended to it exactly (the lift of hefx_mod_raise), multiplied through the NTT, and the quotient by Q is
 * read off the upper mixed-radix digits.  No floating point and no division anywhere.
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
 * context of its own over the L data primes and the auxiliary ones), the rounding tables and the scratch of the two
 * entries below, on the device of ctx; waits for its own uploads.  ctx must outlive the object. */
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

#ifdef __cplusplus
}
#endif
#endif /* HEFX_BFV_H */
