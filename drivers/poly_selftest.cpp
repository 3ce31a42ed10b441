// poly_selftest.cpp -- seal::hefx_evaluate_poly and seal::hefx_scalar_combine (include/seal/shim_poly.h) through
// include/seal/seal.h, at N = 4096 on {60, 40 x 5, 60} and scale 2^40.  The fused executor is held, WORD FOR WORD, to the same
// plan (csrc/hefx_poly_plan.h) executed through the shim's own call-by-call operations: every COMBINE as mod_switch_to,
// encode(double), multiply_plain per term, add_many, add_plain of the encoded constant, then rescale_to_next.  The decoded slots
// are compared with the polynomial in float64 as a sanity check of both.
// Exit code 0 = all checks passed.  Needs a HIP device.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "seal/seal.h"
#include "seal/shim_poly.h"

using namespace std;
using namespace seal;

static int failures = 0;
#define CHECK(cond, what)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            cout << "FAIL: " << what << endl;              \
            ++failures;                                    \
        } else                                             \
            cout << "ok:   " << what << endl;              \
    } while (0)

// the plan, call by call
static void evaluate_composed(const shared_ptr<SEALContext> &context, const Evaluator &evaluator, const CKKSEncoder &encoder, const RelinKeys &rk,
                              const Ciphertext &ct, const vector<double> &coeffs, poly_basis basis, Ciphertext &dest)
{
    hefx_poly::Plan P;
    const char *err = hefx_poly::plan((int)coeffs.size() - 1, coeffs.data(), (int)basis, (int)ct.coeff_mod_count(), context->primes().data(),
                                      ct.scale(), 0.0, P);
    if (err) throw invalid_argument(err);
    vector<Ciphertext> slots((size_t)P.nslots);
    slots[0] = ct;
    for (const hefx_poly::Step &st : P.steps) {
        const parms_id_type id = context->id_of_rows(st.level);
        Ciphertext &out = slots[(size_t)st.dst];
        if (st.op == hefx_poly::MUL) {
            Ciphertext a = slots[(size_t)st.a], b = slots[(size_t)st.b];
            evaluator.mod_switch_to_inplace(a, id);
            evaluator.mod_switch_to_inplace(b, id);
            if (st.a == st.b)
                evaluator.square(a, out);
            else
                evaluator.multiply(a, b, out);
            evaluator.relinearize_inplace(out, rk);
        } else if (st.op == hefx_poly::COMBINE) {
            vector<Ciphertext> prods;
            for (int i = 0; i < st.b; ++i) {
                const hefx_poly::Term &t = P.terms[(size_t)(st.a + i)];
                Ciphertext x = slots[(size_t)t.src], prod;
                evaluator.mod_switch_to_inplace(x, id);
                Plaintext w;
                encoder.encode(t.coef, id, t.wscale, w);
                evaluator.multiply_plain(x, w, prod);
                prods.push_back(prod);
            }
            Ciphertext sum;
            evaluator.add_many(prods, sum);
            if (st.has_const) {
                Plaintext c;
                encoder.encode(st.constant, id, st.cscale, c);
                evaluator.add_plain_inplace(sum, c);
            }
            evaluator.rescale_to_next(sum, out);
        } else {
            evaluator.add(slots[(size_t)st.a], slots[(size_t)st.b], out);
        }
    }
    dest = slots[(size_t)P.steps.back().dst];
}

static double reference_value(poly_basis basis, const vector<double> &c, double x)
{
    double t0 = 1.0, t1 = x, acc = c[0];
    for (size_t i = 1; i < c.size(); ++i) {
        acc += c[i] * t1;
        const double t2 = basis == poly_basis::power ? t1 * x : 2.0 * x * t1 - t0;
        t0 = t1, t1 = t2;
    }
    return acc;
}

int main()
{
    const size_t n = 4096;
    const double scale = pow(2.0, 40);
    EncryptionParameters params(scheme_type::CKKS);
    params.set_poly_modulus_degree(n);
    params.set_coeff_modulus(CoeffModulus::Create(n, {60, 40, 40, 40, 40, 40, 60}));
    auto context = SEALContext::Create(params);
    CKKSEncoder encoder(context);
    Evaluator evaluator(context);
    KeyGenerator keygen(context);
    Encryptor encryptor(context, keygen.public_key());
    Decryptor decryptor(context, keygen.secret_key());
    auto relin_keys = keygen.relin_keys();

    const size_t m = 64;
    vector<double> v(m);
    for (size_t i = 0; i < m; ++i) v[i] = -1.0 + 2.0 * (double)i / (double)(m - 1);
    Plaintext pv;
    encoder.encode(v, scale, pv);
    Ciphertext ct;
    encryptor.encrypt(pv, ct);

    struct Case {
        const char *name;
        poly_basis basis;
        vector<double> c;
    };
    vector<Case> cases = {
        {"sigmoid degree 3, power", poly_basis::power, {0.5, 1.20069, 0.00001, -0.81562}},
        {"sigmoid degree 7, power", poly_basis::power, {0.5, 1.73496, 0.00001, -4.19407, 0.00001, 5.43402, 0.00001, -2.50739}},
        {"a_0 + a_7 x^7", poly_basis::power, {0.5, 0, 0, 0, 0, 0, 0, -1.25}},
        {"degree 7, chebyshev", poly_basis::chebyshev, {0.5, 0.625, -0.125, 0.25, 0.0625, -0.1875, 0.03125, 0.015625}},
    };
    {
        Case big{"degree 31, chebyshev", poly_basis::chebyshev, {}};
        for (int k = 0; k <= 31; ++k) big.c.push_back(k % 2 ? 0.75 / (double)(k * k) : (k ? 0.0 : 0.5));  // an odd function + 1/2
        cases.push_back(big);
    }
    for (const Case &cs : cases) {
        Ciphertext fused, composed;
        hefx_evaluate_poly(evaluator, relin_keys, ct, cs.c, cs.basis, fused);
        evaluate_composed(context, evaluator, encoder, relin_keys, ct, cs.c, cs.basis, composed);
        int degree = (int)cs.c.size() - 1, depth = 0;
        while ((1 << depth) < degree + 1) ++depth;
        CHECK(fused.size() == 2 && (int)fused.coeff_mod_count() == 6 - depth && fused.parms_id() == composed.parms_id(),
              string(cs.name) + ": size 2, ceil(log2(d + 1)) levels down");
        CHECK(fabs(fused.scale() - scale) <= scale * 1e-12 && fabs(fused.scale() - composed.scale()) <= scale * 1e-12,
              string(cs.name) + ": the result carries the input's scale");
        const size_t words = fused.size() * fused.coeff_mod_count() * n;
        CHECK(composed.size() == fused.size() && memcmp(fused.data(), composed.data(), words * sizeof(uint64_t)) == 0,
              string(cs.name) + ": the words of the call-by-call plan");
        Plaintext p;
        decryptor.decrypt(fused, p);
        vector<double> got;
        encoder.decode(p, got);
        double err = 0;
        for (size_t i = 0; i < m; ++i) err = max(err, fabs(got[i] - reference_value(cs.basis, cs.c, v[i])));
        cout << "      max |decoded - p(x)| = " << err << endl;
        CHECK(err < 1e-5, string(cs.name) + ": decoded slots");
    }

    // hefx_scalar_combine on its own: two outputs from inputs of two levels, against multiply_plain / add_many / add_plain
    {
        Ciphertext sq;
        evaluator.square(ct, sq);
        evaluator.relinearize_inplace(sq, relin_keys);
        evaluator.rescale_to_next_inplace(sq);  // 5 rows, 2^80 / q_5
        const parms_id_type id = context->id_of_rows(4);
        const double S = scale * scale;
        const vector<double> ws = {S / ct.scale(), S / sq.scale()};
        const vector<vector<double>> w = {{0.25, -1.5}, {-0.81562, 0.00001}};
        const vector<double> consts = {0.5, -0.125};
        vector<Ciphertext> got;
        hefx_scalar_combine(evaluator, {ct, sq}, w, ws, consts, S, id, got);
        bool same = got.size() == 2;
        for (size_t g = 0; same && g < 2; ++g) {
            vector<Ciphertext> prods;
            const Ciphertext *src[2] = {&ct, &sq};
            for (size_t k = 0; k < 2; ++k) {
                Ciphertext x = *src[k], prod;
                evaluator.mod_switch_to_inplace(x, id);
                Plaintext pw;
                encoder.encode(w[g][k], id, ws[k], pw);
                evaluator.multiply_plain(x, pw, prod);
                prods.push_back(prod);
            }
            Ciphertext sum;
            evaluator.add_many(prods, sum);
            Plaintext pc;
            encoder.encode(consts[g], id, S, pc);
            evaluator.add_plain_inplace(sum, pc);
            same = got[g].size() == 2 && got[g].coeff_mod_count() == 4 && got[g].scale() == S &&
                   memcmp(got[g].data(), sum.data(), 2 * 4 * n * sizeof(uint64_t)) == 0;
        }
        CHECK(same, "hefx_scalar_combine: two outputs, inputs of two levels, the words of the call-by-call sequence");
        bool refused = false;
        try {
            vector<Ciphertext> t;
            hefx_scalar_combine(evaluator, {ct, sq}, w, {ws[0], ws[1] * 1.001}, consts, S, id, t);
        } catch (const invalid_argument &e) {
            refused = string(e.what()).find("scale mismatch") != string::npos;
        }
        CHECK(refused, "hefx_scalar_combine: a term at another scale is refused");
        refused = false;
        try {
            vector<Ciphertext> t;
            hefx_scalar_combine(evaluator, {ct, sq}, {{0.25, 1e-30}}, ws, {}, S, id, t);
        } catch (const logic_error &e) {
            refused = string(e.what()).find("transparent") != string::npos;
        }
        CHECK(refused, "hefx_scalar_combine: a weight that rounds to zero is a transparent term");
    }

    cout << (failures ? "POLY SELFTEST FAILED" : "POLY SELFTEST PASSED") << endl;
    return failures ? 1 : 0;
}
