/* hefx_refresh.h -- extension of the C-ABI in hefx.h: exact mod-raise of plaintexts and the ciphertext refresh built
 * on it (decrypt -> lift -> encrypt in one call).  Same library (libhefx.so), same conventions as hefx.h: device
 * pointers, NTT form, canonical words, asynchronous on the caller's stream.
 *
 * Why a header of its own: two tables of the test suite enumerate hefx.h -- the aliasing cases (one row per entry with
 * a device input and a device output) and the binding's symbol list -- and the change that added these entries could not
 * touch either.  A later change that may extend those tables can move the declarations below into hefx.h as they are.
 *
 * The refresh.  A CKKS ciphertext at its last prime cannot be multiplied again; the holder of the secret key refreshes
 * it by decrypting and re-encrypting at a higher level (the reference's training loop does so after every step,
 * logistic_regression_ckks.cpp:362-381, through decode and encode).  Decode followed by encode at the same scale is the
 * identity on the integer polynomial, so no floating point is needed: the plaintext's coefficients, taken as centred
 * representatives x in (-Q_in/2, Q_in/2) of their residues mod Q_in = q_0 ... q_(L_in-1), are written mod the primes of
 * the higher level -- exact integer work (mixed-radix digits, Horner), the first step of every CKKS bootstrapping too.
 *
 * None of the entries waits on the host for anything but a pointer-table ring slot of its own (hefx_refresh_batch);
 * their tables travel in kernel arguments and their scratch is the context's.  They are held to stream order, against
 * references outside the engine, by tests/test_gpu_streams_ext.py.
 * This build serves poly_degree 1024 .. 16384 here (32768: HEFX_ERR_UNSUPPORTED).
 */
#ifndef HEFX_REFRESH_H
#define HEFX_REFRESH_H

#include "hefx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most primes the lift reads (L_in): the width of its mixed-radix digit array, as in hefx_ckks_decode */
#define HEFX_LIFT_MAX_LIN 16
/* items hefx_refresh_batch takes through one set of launches */
#define HEFX_REFRESH_GROUP 64

/* out[count][L_out][N] = the centred lift of in[count][L_in][N]; NTT form in and out.  1 <= L_in < L_out <= the number
 * of data primes (k - 1, or 1 when k == 1), L_in <= HEFX_LIFT_MAX_LIN.  Every coefficient x in [0, Q_in) stands for x
 * when x <= floor(Q_in / 2) and for x - Q_in otherwise (the rule of hefx_ckks_decode); rows below L_in of the output are
 * the input's words.  d_in is left as it is.  d_out may not overlap d_in in BYTES (d_out == d_in included):
 * HEFX_ERR_INVALID before anything is submitted. */
int hefx_mod_raise(hefx_context *ctx, int L_in, int L_out, int count, const uint64_t *d_in, uint64_t *d_out,
                   void *stream);

/* decrypt (any size >= 2) -> lift -> encrypt at L_out, L_in <= L_out: out[2][L_out][N] holds the words of hefx_decrypt
 * at L_in, hefx_mod_raise (skipped when L_in == L_out) and hefx_encrypt at L_out with the same key32 / stream_id.
 * d_ct = [size][L_in][N], d_sk = [>= L_in][N], d_pk = [2][k][N].  The plaintext never leaves the device.  d_out may
 * overlap neither d_ct, nor the L_in rows of d_sk, nor d_pk, in BYTES (d_out == d_ct included): HEFX_ERR_INVALID before
 * anything is submitted. */
int hefx_refresh(hefx_context *ctx, int L_in, int size, int L_out, const uint64_t *d_ct, const uint64_t *d_sk,
                 const uint64_t *d_pk, const uint8_t *key32, uint64_t stream_id, uint64_t *d_out, void *stream);

/* n items in lockstep, item i with stream id first_stream_id + i: the words of n hefx_refresh calls, from one set of
 * launches (decrypt sums, transforms, lift, sampling, encrypt) per HEFX_REFRESH_GROUP items instead of one per item.
 * No output may overlap, in BYTES, a ciphertext of the call (another item's included), the L_in rows of d_sk, d_pk or
 * another output: HEFX_ERR_INVALID before anything is submitted. */
int hefx_refresh_batch(hefx_context *ctx, int L_in, int size, int L_out, int n, const uint64_t *const *d_cts,
                       const uint64_t *d_sk, const uint64_t *d_pk, const uint8_t *key32, uint64_t first_stream_id,
                       uint64_t *const *d_outs, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HEFX_REFRESH_H */
