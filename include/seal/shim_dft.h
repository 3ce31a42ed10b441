// seal/shim_dft.h -- the inner sums of a baby-step/giant-step matrix product for users of the seal.h shim
// (include/hefx_dft.h).  Not part of SEAL's API, and therefore not in seal.h: a program includes this header next to
// seal/seal.h when it wants it, and the libraries that stand in for libhefx.so under seal.h alone need no new symbol.
//
//     seal::hefx_plain_combine(evaluator, cts, pts, dests);
//         dests[g] = sum over the k with pts[g][k] != nullptr of  *pts[g][k] (.) cts[k],  ONE pass over the inputs
//         (hefx_plain_combine): the words and the checks of multiply_plain per term and add_many.  nullptr is a structural
//         zero: no term.  The ciphertexts share one level and scale, and so do the plaintexts.
//
// Not recorded in the shim's lazy graph: what is pending is submitted first and the call runs live.  The plan of
// CoeffToSlot / SlotToCoeff that feeds it is Python-only for now (seal_fyp_logistic_regression_amd/dft.py).
#pragma once
#include <cmath>
#include <vector>

#include "../hefx_dft.h"
#include "seal.h"

namespace seal {

inline void hefx_plain_combine(const Evaluator &evaluator, const std::vector<Ciphertext> &cts,
                               const std::vector<std::vector<const Plaintext *>> &pts, std::vector<Ciphertext> &dests)
{
    const auto &ctx = evaluator.shim_context();
    if (!ctx->is_ckks()) throw std::invalid_argument("unsupported scheme");
    const std::size_t m = cts.size(), G = pts.size();
    if (m < 1 || m > HEFX_PLAIN_COMBINE_MAX_IN || G < 1 || G > HEFX_PLAIN_COMBINE_MAX_OUT)
        throw std::invalid_argument("plain_combine: need 1..256 ciphertexts and 1..64 outputs");
    auto close = [](double a, double b) { return a == b || std::fabs(a - b) <= std::max(std::fabs(a), std::fabs(b)) * 9.094947017729282e-13; };
    const Ciphertext &c0 = cts[0];
    for (const Ciphertext &c : cts) {
        if (!c.buf || ctx->rows_of(c.parms_id()) != c.rows || !c.is_ntt_form()) throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if (c.parms_id() != c0.parms_id()) throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        if (c.size() != 2) throw std::invalid_argument("encrypted size must be 2");
        if (!close(c0.scale(), c.scale())) throw std::invalid_argument("scale mismatch");
    }
    const int L = c0.rows;
    double scale = 0.0;
    std::vector<const std::uint64_t *> pt_p(G * m, nullptr);
    for (std::size_t g = 0; g < G; ++g) {
        if (pts[g].size() != m) throw std::invalid_argument("plain_combine: need one plaintext (or nullptr) per output and ciphertext");
        bool any = false;
        for (std::size_t k = 0; k < m; ++k) {
            const Plaintext *p = pts[g][k];
            if (!p) continue;
            any = true;
            if (!p->buf || !p->is_ntt_form() || p->parms_id() != c0.parms_id()) throw std::invalid_argument("encrypted_ntt and plain_ntt parameter mismatch");
            const double s = c0.scale() * p->scale();
            if (!(s > 0 && (int)std::log2(s) < ctx->get_context_data(c0.parms_id())->total_coeff_modulus_bit_count()))
                throw std::invalid_argument("scale out of bounds");
            if (scale != 0.0 && !close(scale, s)) throw std::invalid_argument("scale mismatch");
            if (scale == 0.0) scale = s;
            if (p->is_zero()) throw std::logic_error("result ciphertext is transparent");
            pt_p[g * m + k] = p->buf->p;
        }
        if (!any) throw std::invalid_argument("plain_combine: an output has no term");
    }
    auto &e = ctx->engine();
    hefx_context *h = e->live();  // every pending recorded operation is submitted: the inputs are many
    std::vector<const std::uint64_t *> in_p(m);
    std::vector<shim::BufPtr> outs(G);
    std::vector<std::uint64_t *> out_p(G);
    for (std::size_t k = 0; k < m; ++k) in_p[k] = cts[k].buf->p;
    for (std::size_t g = 0; g < G; ++g) {
        outs[g] = shim::new_buf(e, 2 * (std::size_t)L * ctx->n());
        out_p[g] = outs[g]->p;
    }
    shim::check(::hefx_plain_combine(h, L, (int)m, in_p.data(), (int)G, pt_p.data(), out_p.data(), nullptr));
    std::vector<Ciphertext> res(G);
    for (std::size_t g = 0; g < G; ++g) res[g].set(outs[g], 2, L, c0.parms_id(), scale);
    dests = std::move(res);
}

}  // namespace seal
