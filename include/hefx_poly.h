/* hefx_poly.h -- extension of the C-ABI in hefx.h: polynomial evaluation on CKKS ciphertexts.  Same library (libhefx.so),
 * same conventions as hefx.h: device pointers, NTT form, canonical words, asynchronous on the caller's stream.
 *
 * Two things live here.
 *   hefx_scalar_combine   the inner loop of every polynomial evaluator: G scalar combinations  sum_k w[g][k] * ct_k + c_g
 *                         of the same m ciphertexts in ONE pass over the inputs.  The NTT of a constant polynomial is that
 *                         constant in every slot, so a scalar plaintext is L words, not L * N: no plaintext is ever
 *                         materialised, and inputs of a higher level are read through their own row stride (the row prefix
 *                         IS the mod-dropped ciphertext).
 *   hefx_poly_plan        the depth-optimal Paterson-Stockmeyer plan of a polynomial in the power or the Chebyshev basis, as
 *                         a flat list of steps over numbered slots (host-only planner, csrc/hefx_poly_plan.h), and
 *                         hefx_poly_weight_residue, the one rounding rule every weight of a plan goes through.
 *
 * Why a header of its own: two tables of the test suite enumerate hefx.h (the aliasing cases and the binding's symbol list);
 * a later change that may extend those tables can move the declarations below into hefx.h as they are.
 */
#ifndef HEFX_POLY_H
#define HEFX_POLY_H

#include "hefx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HEFX_COMBINE_MAX_IN 256 /* m: inputs of one hefx_scalar_combine */
#define HEFX_COMBINE_MAX_OUT 16 /* G: outputs of one hefx_scalar_combine */

/* For every polynomial p < size, row j < L and slot x:
 *     d_out[g][p][j][x] = ( sum_k h_weights[g][k][j] * d_in[k][p][j][x] + (p == 0 ? h_consts[g][j] : 0) ) mod q_j,
 * canonical -- the words of hefx_mod_drop of each input to L rows, hefx_ckks_encode_scalar of each weight,
 * hefx_multiply_plain, hefx_add_many and hefx_add_plain, from one kernel that reads every input word once for all G outputs.
 *   d_in[k]    [size][in_rows[k]][N], in_rows[k] >= L: the first L rows of every polynomial are read, the rest skipped
 *   h_weights  [G][m][L] residues, each < q_j; HOST memory, copied before the call returns (may be transient).  A weight of
 *              zero is legal and is a term of zero
 *   h_consts   [G][L] residues, each < q_j, HOST memory, or NULL for no constant
 *   d_out[g]   [size][L][N]
 * 1 <= m <= HEFX_COMBINE_MAX_IN, 1 <= G <= HEFX_COMBINE_MAX_OUT, size >= 1, 1 <= L <= the context's prime count.
 * Aliasing: no output may overlap an input (all in_rows[k] rows of it) or another output, in BYTES, d_out[g] == d_in[k]
 * included: HEFX_ERR_INVALID before anything is submitted.  HEFX_ERR_INVALID as well, before anything is submitted: a
 * residue >= q_j, in_rows[k] < L, m or G out of range, a null pointer.  The words of the inputs are taken as canonical.
 * The call waits on the host for nothing but a descriptor-ring slot of its own. */
int hefx_scalar_combine(hefx_context *ctx, int L, int size, int m, const uint64_t *const *d_in, const int *in_rows, int G,
                        const uint64_t *h_weights, const uint64_t *h_consts, uint64_t *const *d_out, void *stream);

/* round_half_away(value * scale) mod q, canonical: the word hefx_ckks_encode_scalar(value, scale) writes into a row of
 * modulus q.  The product is formed in float64; below 2^63 its rounded magnitude is reduced as a 64-bit integer, from 2^63 up
 * as m * 2^e (hefx_ckks_encode_wide); a negative value gives q - r.  A non-finite product gives 0. */
uint64_t hefx_poly_weight_residue(double value, double scale, uint64_t q);

/* ---- the plan ---------------------------------------------------------------------------------------------------------
 * Slots hold ciphertexts; slot 0 is the input (level = nprimes rows, scale in_scale).  Steps run in order:
 *   HEFX_POLY_MUL      dst = relinearize(a * b): both operands dropped to the lower of their levels (`level`), the tensor
 *                      product relinearised and NOT rescaled; scale = scale(a) * scale(b)
 *   HEFX_POLY_COMBINE  dst = rescale_to_next( sum over terms[a .. a + b) of round(coef * wscale) * slot[src]
 *                      + round(constant * cscale) ): hefx_scalar_combine at `level` rows, then one rescale.  Every term has
 *                      scale(src) * wscale = S = cscale (to float64 rounding); the result has level - 1 rows and carries
 *                      scale = S / q_(level-1), stated in `scale`
 *   HEFX_POLY_ADD      dst = a + b, both at `level`, scales equal (to float64 rounding)
 * The last step's dst is the result: nprimes - ceil(log2(degree + 1)) rows, scale target_scale. */
enum { HEFX_POLY_MUL = 0, HEFX_POLY_COMBINE = 1, HEFX_POLY_ADD = 2 };
enum { HEFX_POLY_BASIS_POWER = 0, HEFX_POLY_BASIS_CHEBYSHEV = 1 };

typedef struct hefx_poly_step {
    int32_t op;        /* HEFX_POLY_* */
    int32_t dst;       /* slot written (every slot is written once) */
    int32_t a, b;      /* MUL / ADD: operand slots; COMBINE: first term and number of terms (b >= 1) */
    int32_t level;     /* rows the step runs at */
    int32_t has_const; /* COMBINE: `constant` is added */
    double constant;   /* COMBINE: the constant, encoded at cscale */
    double cscale;     /* COMBINE: S */
    double scale;      /* scale of dst */
} hefx_poly_step;

typedef struct hefx_poly_term {
    int32_t src; /* slot */
    int32_t pad_;
    double coef, wscale; /* the weight is round_half_away(coef * wscale) */
} hefx_poly_term;

/* Plans  sum_i coeffs[i] x^i  (HEFX_POLY_BASIS_POWER) or  sum_i coeffs[i] T_i(x)  (HEFX_POLY_BASIS_CHEBYSHEV, Chebyshev
 * polynomials of the first kind; the input is assumed in [-1, 1], any change of variable is the caller's) for an input of
 * `nprimes` rows over primes[0 .. nprimes) at scale in_scale; target_scale <= 0: in_scale.  Trailing zero coefficients are
 * dropped; what remains must have degree >= 1.
 * Paterson-Stockmeyer with the baby-step count searched over powers of two: depth exactly ceil(log2(degree + 1)) levels in
 * either basis and, among those plans, the fewest MULs.  Scales are tracked, never overwritten: a node that must deliver
 * (level, S) asks its quotient for S * q_level / scale(giant step) one level up, and the leaves absorb whatever scale is
 * asked of them in their weights.  No transparent ciphertext is formed: a zero coefficient is no term, a chunk that is only a
 * constant becomes a weight on its giant step.
 * Writes at most max_steps steps and max_terms terms; *nsteps, *nterms, *nslots (slots used, the input included) always
 * receive what the plan needs, so a call with max_steps = max_terms = 0 sizes the arrays (HEFX_ERR_INVALID with them set).
 * HEFX_ERR_INVALID: bad arguments, a constant polynomial, not enough levels (nprimes - depth < 1).  Host only: no device
 * is touched. */
int hefx_poly_plan(int degree, const double *coeffs, int basis, int nprimes, const uint64_t *primes, double in_scale,
                   double target_scale, hefx_poly_step *steps, int max_steps, int *nsteps, hefx_poly_term *terms,
                   int max_terms, int *nterms, int *nslots);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_POLY_H */
