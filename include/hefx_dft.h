/* hefx_dft.h -- extension of the C-ABI in hefx.h: the hot loop of the homomorphic DFT (CoeffToSlot / SlotToCoeff, the linear
 * transforms of CKKS bootstrapping).  Same library (libhefx.so), same conventions as hefx.h: device pointers, NTT form,
 * canonical words, asynchronous on the caller's stream.
 *
 * A stage of those transforms is a matrix given by a few cyclic diagonals over all N/2 slots, applied in baby-step/giant-step
 * form: the same few rotated ciphertexts are multiplied by many different plaintexts and summed per giant step.
 * hefx_plain_combine forms all those inner sums in ONE pass over the rotated ciphertexts.  The plan of the transforms
 * (which diagonals, which split, which scales) is host code: seal_fyp_logistic_regression_amd/dft.py.
 *
 * Why a header of its own: two tables of the test suite enumerate hefx.h (the aliasing cases and the binding's symbol list);
 * a later change that may extend those tables can move the declaration below into hefx.h as it is.
 */
#ifndef HEFX_DFT_H
#define HEFX_DFT_H

#include "hefx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HEFX_PLAIN_COMBINE_MAX_IN 256 /* m: inputs of one hefx_plain_combine */
#define HEFX_PLAIN_COMBINE_MAX_OUT 64 /* G: outputs of one hefx_plain_combine */

/* For every output g < G, polynomial p < 2, row j < L and slot x:
 *     d_out[g][p][j][x] = ( sum over k < m with d_pts[g*m + k] != NULL of  d_pts[g*m + k][j][x] * d_in[k][p][j][x] ) mod q_j,
 * canonical: the residue of the integer sum -- the words of hefx_multiply_plain per term followed by hefx_add_many, and of
 * hefx_multiply_plain_sum on the non-null terms of each output -- from ONE launch that reads every input word once for a tile
 * of 1, 2, 4 or 8 outputs (the widest that still fills the device: DESIGN.md) and every plaintext word once for both
 * polynomials.
 *   d_in[k]    [2][L][N]
 *   d_pts      HOST array of G * m device pointers, row-major [G][m]; each [L][N] or NULL.  NULL is a structural zero: no
 *              term, nothing read.  The same plaintext may stand in several places.  The array is copied before the call
 *              returns (may be transient)
 *   d_out[g]   [2][L][N]
 * 1 <= m <= HEFX_PLAIN_COMBINE_MAX_IN, 1 <= G <= HEFX_PLAIN_COMBINE_MAX_OUT, 1 <= L <= the context's prime count.  The tiles
 * of a call run side by side in its one launch.
 * HEFX_ERR_UNSUPPORTED, before anything is submitted: m + G * m + G pointers do not fit one descriptor-ring slot (10240).
 * HEFX_ERR_INVALID, before anything is submitted (a refused call writes nothing): m, G or L out of range; a null d_in[k] or
 * d_out[g]; an output with no term (every d_pts[g*m + .] NULL); an output that overlaps an input, a plaintext or another
 * output in BYTES, d_out[g] == d_in[k] included ("Aliasing").
 * Whether a plaintext is the zero polynomial (SEAL: "result ciphertext is transparent") is the caller's check, as for
 * hefx_multiply_plain_sum.  The call waits on the host for nothing but a descriptor-ring slot of its own. */
int hefx_plain_combine(hefx_context *ctx, int L, int m, const uint64_t *const *d_in, int G, const uint64_t *const *d_pts,
                       uint64_t *const *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_DFT_H */
