/* hefx_bootstrap.h -- extension of the C-ABI in hefx.h: the fused node of EvalMod, the polynomial step of CKKS bootstrapping
 * between the two linear transforms (include/hefx_dft.h).  Same library (libhefx.so), same conventions as hefx.h: device
 * pointers, NTT form, canonical words, asynchronous on the caller's stream.
 *
 * A node of a Paterson-Stockmeyer plan (include/hefx_poly.h) is  sum_p u_p * (a_p * b_p) + sum_k w_k * ct_k + c.  Run step by
 * step every product is relinearised on its own before hefx_scalar_combine sums them.  Relinearisation is linear, so the sum
 * can be formed at size 3 and relinearised ONCE: hefx_product_combine forms it in one pass -- the tensor products are never
 * written -- and a double angle 2 x^2 - 1 is the same call with P = 1, a = b, u = 2, c = -1.  The plan (which products a node
 * defers, the scales) is host code: algorithms.evaluate_polynomial_many, bootstrap.py.
 *
 * Why a header of its own: two tables of the test suite enumerate hefx.h (the aliasing cases and the binding's symbol list);
 * a later change that may extend those tables can move the declaration below into hefx.h as it is.
 */
#ifndef HEFX_BOOTSTRAP_H
#define HEFX_BOOTSTRAP_H

#include "hefx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HEFX_PRODUCT_COMBINE_MAX_PRODUCTS 32 /* P: products of one node */
#define HEFX_PRODUCT_COMBINE_MAX_LIN 64      /* m: linear terms of one node */
#define HEFX_PRODUCT_COMBINE_MAX_ITEMS 64    /* n: items that run the node in lockstep */

/* n items run the same node (the two chains of the DFT, or a batch).  For every item i < n, row j < L and slot x, with
 * a = d_a[i*P + p], b = d_b[i*P + p], l = d_lin[i*m + k], subscripts 0 / 1 their two polynomials:
 *     d_out[i][0][j][x] = ( sum_p h_u[p][j] * a0 * b0               + sum_k h_w[k][j] * l0 + h_c[j] ) mod q_j
 *     d_out[i][1][j][x] = ( sum_p h_u[p][j] * (a0 * b1 + a1 * b0)   + sum_k h_w[k][j] * l1          ) mod q_j
 *     d_out[i][2][j][x] = ( sum_p h_u[p][j] * a1 * b1                                               ) mod q_j,
 * canonical: the residue of the integer sum -- the words of hefx_mod_drop of every operand to L rows, hefx_multiply per
 * product, a scalar plaintext product (hefx_multiply_plain by the constant polynomial of the weight) at size 3 / size 2,
 * hefx_add_many over the size-3 terms and over the size-2 terms, hefx_add of the two sums on the first two polynomials, and
 * hefx_add_plain of the constant.  Nothing is relinearised or rescaled.
 *   d_a, d_b   HOST arrays of n * P device pointers, row-major [n][P]; operand p is [2][a_rows[p]][N] (d_b: b_rows[p]) in every
 *              item, a_rows[p], b_rows[p] >= L: the first L rows of each polynomial are read through the operand's own row
 *              stride (the row prefix IS the mod-dropped ciphertext).  d_a[i*P + p] == d_b[i*P + p] (a square) is allowed, and
 *              an operand may stand in several places
 *   d_lin      HOST array of n * m device pointers, [n][m]; term k is [2][lin_rows[k]][N], lin_rows[k] >= L.  m == 0: d_lin,
 *              lin_rows and h_w are not read and may be NULL
 *   h_u        [P][L] residues, each < q_j;  h_w  [m][L] residues, each < q_j;  h_c  [L] residues, each < q_j, or NULL for no
 *              constant.  HOST memory, shared by the n items, copied before the call returns (may be transient).  A weight of
 *              zero is legal and is a term of zero
 *   d_out[i]   [3][L][N]
 * 1 <= P <= HEFX_PRODUCT_COMBINE_MAX_PRODUCTS, 0 <= m <= HEFX_PRODUCT_COMBINE_MAX_LIN, 1 <= n <= HEFX_PRODUCT_COMBINE_MAX_ITEMS,
 * 1 <= L <= the context's prime count.  One launch and one descriptor-ring slot for the whole call.
 * HEFX_ERR_UNSUPPORTED, before anything is submitted: 2P + m + L (P + m + 1) + n (2P + m + 1) words do not fit one
 * descriptor-ring slot (10240).
 * HEFX_ERR_INVALID, before anything is submitted (a refused call writes nothing): P, m, n or L out of range; a null pointer; a
 * row count below L or above the context's prime count; a residue >= q_j; an output that overlaps an operand (ALL its rows), a
 * linear term or another output in BYTES, d_out[i] == d_a[i*P + p] included ("Aliasing").
 * The words of the inputs are taken as canonical.  The call waits on the host for nothing but a descriptor-ring slot of its
 * own. */
int hefx_product_combine(hefx_context *ctx, int L, int n, int P, const uint64_t *const *d_a, const int *a_rows,
                         const uint64_t *const *d_b, const int *b_rows, const uint64_t *h_u, int m, const uint64_t *const *d_lin,
                         const int *lin_rows, const uint64_t *h_w, const uint64_t *h_c, uint64_t *const *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_BOOTSTRAP_H */
