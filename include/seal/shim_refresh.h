// seal/shim_refresh.h -- the refresh of a CKKS ciphertext for users of the seal.h shim: decrypt, exact lift to the first
// level, encrypt, as ONE engine call (hefx_refresh / hefx_refresh_batch, include/hefx_refresh.h).  Not part of SEAL's API
// -- SEAL has no such call; the reference's training loop spells it decrypt / decode / encode / encrypt
// (logistic_regression_ckks.cpp:362-381) -- and therefore not in seal.h: a program includes this header next to
// seal/seal.h when it wants it, and the libraries that stand in for libhefx.so under seal.h alone need no new symbol.
//
//     seal::hefx_refresh(decryptor, encryptor, ct, dest);      // dest: size 2, first level, ct's scale
//     seal::hefx_refresh(decryptor, encryptor, cts, dests);    // the same for every element, in lockstep
//
// The encryptor's sampler advances as it does for encrypt(): one stream id per ciphertext.
#pragma once
#include <vector>

#include "../hefx_refresh.h"
#include "seal.h"

namespace seal {

namespace shim {
inline int refresh_target_rows(const SEALContext &ctx) { return ctx.rows_of(ctx.first_parms_id()); }
inline void refresh_check(const SEALContext &ctx, const Ciphertext &ct, const Encryptor &enc, const Decryptor &dec)
{
    if (!ctx.is_ckks()) throw std::invalid_argument("unsupported scheme");
    if (!ct.buf || ct.size() < 2 || !ct.is_ntt_form()) throw std::invalid_argument("encrypted is not valid for encryption parameters");
    if (ct.rows > refresh_target_rows(ctx)) throw std::invalid_argument("encrypted is not valid for encryption parameters");
    if (!enc.shim_public_key().buf || !dec.shim_secret_key().buf) throw std::invalid_argument("key is not valid for encryption parameters");
}
}  // namespace shim

// dest = a fresh encryption, at the first level, of what ct decrypts to; the scale is ct's
inline void hefx_refresh(const Decryptor &decryptor, const Encryptor &encryptor, const Ciphertext &ct, Ciphertext &dest)
{
    const auto &ctx = decryptor.shim_context();
    shim::refresh_check(*ctx, ct, encryptor, decryptor);
    auto &e = ctx->engine();
    const int L_in = ct.rows, L_out = shim::refresh_target_rows(*ctx);
    auto out = shim::new_buf(e, (std::size_t)2 * L_out * ctx->n());
    const shim::SamplerState &rnd = encryptor.shim_sampler();
    // (ready: what is recorded and still pending for ct is submitted first, as Decryptor::decrypt does)
    shim::check(::hefx_refresh(e->ready({ct.buf.get()}), L_in, (int)ct.size(), L_out, ct.buf->p, decryptor.shim_secret_key().buf->p,
                               encryptor.shim_public_key().buf->p, rnd.key.data(), rnd.stream(), out->p, nullptr));
    dest.set(out, 2, L_out, ctx->first_parms_id(), ct.scale());
}

// dests[i] = hefx_refresh(cts[i]) for ciphertexts of one level and size, one engine call (hefx_refresh_batch); ciphertexts
// of different shapes go one by one
inline void hefx_refresh(const Decryptor &decryptor, const Encryptor &encryptor, const std::vector<Ciphertext> &cts,
                         std::vector<Ciphertext> &dests)
{
    const auto &ctx = decryptor.shim_context();
    const std::size_t n = cts.size();
    bool uniform = n > 0;
    for (const Ciphertext &c : cts) {
        shim::refresh_check(*ctx, c, encryptor, decryptor);
        uniform = uniform && c.rows == cts[0].rows && c.size() == cts[0].size();
    }
    std::vector<Ciphertext> res(n);
    if (!uniform) {
        for (std::size_t i = 0; i < n; ++i) hefx_refresh(decryptor, encryptor, cts[i], res[i]);
        dests = std::move(res);
        return;
    }
    auto &e = ctx->engine();
    const int L_in = cts[0].rows, L_out = shim::refresh_target_rows(*ctx);
    hefx_context *h = e->live();  // every pending recorded operation is submitted: the inputs are many
    std::vector<shim::BufPtr> outs(n);
    std::vector<const std::uint64_t *> in_p(n);
    std::vector<std::uint64_t *> out_p(n);
    for (std::size_t i = 0; i < n; ++i) {
        outs[i] = shim::new_buf(e, (std::size_t)2 * L_out * ctx->n());
        in_p[i] = cts[i].buf->p;
        out_p[i] = outs[i]->p;
    }
    const shim::SamplerState &rnd = encryptor.shim_sampler();
    const std::uint64_t first = rnd.stream();
    for (std::size_t i = 1; i < n; ++i) (void)rnd.stream();
    shim::check(::hefx_refresh_batch(h, L_in, (int)cts[0].size(), L_out, (int)n, in_p.data(), decryptor.shim_secret_key().buf->p,
                                     encryptor.shim_public_key().buf->p, rnd.key.data(), first, out_p.data(), nullptr));
    for (std::size_t i = 0; i < n; ++i) res[i].set(outs[i], 2, L_out, ctx->first_parms_id(), cts[i].scale());
    dests = std::move(res);
}

}  // namespace seal
