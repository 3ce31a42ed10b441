// seal/shim_poly.h -- polynomial evaluation on CKKS ciphertexts for users of the seal.h shim (include/hefx_poly.h).  Not
// part of SEAL's API, and therefore not in seal.h: a program includes this header next to seal/seal.h when it wants it, and
// the libraries that stand in for libhefx.so under seal.h alone need no new symbol.
//
//     seal::hefx_scalar_combine(evaluator, cts, weights, wscales, consts, scale, parms_id, dests);
//         dests[g] = sum_k weights[g][k] * cts[k] + consts[g]  at level parms_id and scale `scale`, ONE pass over the inputs
//         (hefx_scalar_combine): the words and the checks of mod_switch_to, encode(double), multiply_plain, add_many, add_plain
//     seal::hefx_evaluate_poly(evaluator, relin_keys, ct, coeffs, basis, dest);
//         sum_i coeffs[i] ct^i  or  sum_i coeffs[i] T_i(ct)  in ceil(log2(degree + 1)) levels, scales tracked: the plan of
//         csrc/hefx_poly_plan.h -- the planner hefx_poly_plan hands out and the Python executor reads -- executed with the
//         evaluator's own multiply / relinearize / rescale_to_next and hefx_scalar_combine
//
// Neither is recorded in the shim's lazy graph: what is pending is submitted first and the calls run live.
#pragma once
#include <cmath>
#include <vector>

#include "../../seal_fyp_logistic_regression_amd/csrc/hefx_poly_plan.h"
#include "../hefx_poly.h"
#include "seal.h"

namespace seal {

enum class poly_basis { power = HEFX_POLY_BASIS_POWER, chebyshev = HEFX_POLY_BASIS_CHEBYSHEV };

namespace shim {
inline bool poly_close(double a, double b) { return a == b || std::fabs(a - b) <= std::max(std::fabs(a), std::fabs(b)) * 9.094947017729282e-13; }
inline void poly_check_scale(const SEALContext &ctx, double s, const parms_id_type &id)
{
    if (!(s > 0 && (int)std::log2(s) < ctx.get_context_data(id)->total_coeff_modulus_bit_count())) throw std::invalid_argument("scale out of bounds");
}
}  // namespace shim

// weights[g][k]: the scalar plaintext encode(weights[g][k], wscales[k]); cts[k].scale() * wscales[k] must be `scale` for every
// k (scale <= 0: taken from term 0); consts: one per output, encoded at `scale`, or empty for none
inline void hefx_scalar_combine(const Evaluator &evaluator, const std::vector<Ciphertext> &cts, const std::vector<std::vector<double>> &weights,
                                const std::vector<double> &wscales, const std::vector<double> &consts, double scale,
                                const parms_id_type &parms_id, std::vector<Ciphertext> &dests)
{
    const auto &ctx = evaluator.shim_context();
    if (!ctx->is_ckks()) throw std::invalid_argument("unsupported scheme");
    const std::size_t m = cts.size(), G = weights.size();
    if (m < 1 || m > HEFX_COMBINE_MAX_IN || G < 1 || G > HEFX_COMBINE_MAX_OUT || wscales.size() != m || (!consts.empty() && consts.size() != G))
        throw std::invalid_argument("scalar_combine: need 1..256 ciphertexts, 1..16 outputs, one weight scale per ciphertext");
    const int L = ctx->rows_of(parms_id);
    if (L == 0) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    const double S = scale > 0 ? scale : cts[0].scale() * wscales[0];
    for (std::size_t k = 0; k < m; ++k) {
        const Ciphertext &c = cts[k];
        if (!c.buf || ctx->rows_of(c.parms_id()) != c.rows || !c.is_ntt_form()) throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if (c.rows < L) throw std::invalid_argument("cannot switch to higher level modulus");
        if (c.size() != cts[0].size()) throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
        shim::poly_check_scale(*ctx, wscales[k], parms_id);
        shim::poly_check_scale(*ctx, c.scale() * wscales[k], parms_id);
        if (!shim::poly_close(S, c.scale() * wscales[k])) throw std::invalid_argument("scale mismatch");
    }
    shim::poly_check_scale(*ctx, S, parms_id);
    const auto &q = ctx->primes();
    std::vector<std::uint64_t> w(G * m * (std::size_t)L), cst(consts.empty() ? 0 : G * (std::size_t)L);
    for (std::size_t g = 0; g < G; ++g) {
        if (weights[g].size() != m) throw std::invalid_argument("scalar_combine: need one weight per output and ciphertext");
        for (std::size_t k = 0; k < m; ++k) {
            if (std::round(weights[g][k] * wscales[k]) == 0.0) throw std::logic_error("result ciphertext is transparent");
            for (int j = 0; j < L; ++j) w[(g * m + k) * L + j] = hefx_poly::weight_residue(weights[g][k], wscales[k], q[(std::size_t)j]);
        }
        for (int j = 0; j < L && !consts.empty(); ++j) cst[g * L + j] = hefx_poly::weight_residue(consts[g], S, q[(std::size_t)j]);
    }
    auto &e = ctx->engine();
    hefx_context *h = e->live();  // every pending recorded operation is submitted: the inputs are many
    const std::size_t size = cts[0].size();
    std::vector<const std::uint64_t *> in_p(m);
    std::vector<int> rows(m);
    std::vector<shim::BufPtr> outs(G);
    std::vector<std::uint64_t *> out_p(G);
    for (std::size_t k = 0; k < m; ++k) in_p[k] = cts[k].buf->p, rows[k] = cts[k].rows;
    for (std::size_t g = 0; g < G; ++g) {
        outs[g] = shim::new_buf(e, size * (std::size_t)L * ctx->n());
        out_p[g] = outs[g]->p;
    }
    shim::check(::hefx_scalar_combine(h, L, (int)size, (int)m, in_p.data(), rows.data(), (int)G, w.data(), consts.empty() ? nullptr : cst.data(),
                                      out_p.data(), nullptr));
    std::vector<Ciphertext> res(G);
    for (std::size_t g = 0; g < G; ++g) res[g].set(outs[g], size, L, parms_id, S);
    dests = std::move(res);
}

// The plan of hefx_poly_plan.h for (coeffs, basis) at ct's level and scale, executed: MUL = mod_switch_to the lower level,
// multiply, relinearize; COMBINE = hefx_scalar_combine and rescale_to_next; ADD = add.  target_scale <= 0: ct's scale.
inline void hefx_evaluate_poly(const Evaluator &evaluator, const RelinKeys &relin_keys, const Ciphertext &ct, const std::vector<double> &coeffs,
                               poly_basis basis, Ciphertext &dest, double target_scale = 0.0)
{
    const auto &ctx = evaluator.shim_context();
    if (!ct.buf || ct.size() != 2 || ctx->rows_of(ct.parms_id()) != ct.rows) throw std::invalid_argument("encrypted is not valid for encryption parameters");
    hefx_poly::Plan P;
    if (const char *err = hefx_poly::plan((int)coeffs.size() - 1, coeffs.data(), (int)basis, ct.rows, ctx->primes().data(), ct.scale(), target_scale, P))
        throw std::invalid_argument(std::string("poly_plan: ") + err);
    std::vector<Ciphertext> slots((std::size_t)P.nslots);
    slots[0] = ct;
    for (const hefx_poly::Step &st : P.steps) {
        Ciphertext &out = slots[(std::size_t)st.dst];
        if (st.op == hefx_poly::MUL) {
            Ciphertext a = slots[(std::size_t)st.a];
            evaluator.mod_switch_to_inplace(a, ctx->id_of_rows(st.level));
            if (st.a == st.b) {
                evaluator.square(a, out);
            } else {
                Ciphertext b = slots[(std::size_t)st.b];
                evaluator.mod_switch_to_inplace(b, ctx->id_of_rows(st.level));
                evaluator.multiply(a, b, out);
            }
            evaluator.relinearize_inplace(out, relin_keys);
        } else if (st.op == hefx_poly::COMBINE) {
            std::vector<Ciphertext> ins;
            std::vector<double> w, ws;
            for (int i = 0; i < st.b; ++i) {
                const hefx_poly::Term &t = P.terms[(std::size_t)(st.a + i)];
                ins.push_back(slots[(std::size_t)t.src]);
                w.push_back(t.coef);
                ws.push_back(t.wscale);
            }
            std::vector<Ciphertext> res;
            hefx_scalar_combine(evaluator, ins, {w}, ws, st.has_const ? std::vector<double>{st.constant} : std::vector<double>{}, st.cscale,
                                ctx->id_of_rows(st.level), res);
            evaluator.rescale_to_next(res[0], out);
        } else {
            evaluator.add(slots[(std::size_t)st.a], slots[(std::size_t)st.b], out);
        }
    }
    dest = slots[(std::size_t)P.steps.back().dst];
}

}  // namespace seal
