// refresh_selftest.cpp -- seal::hefx_refresh (include/seal/shim_refresh.h) through include/seal/seal.h, at N = 4096 on the
// LR chain {60, 40 x 7, 60} and scale 2^40:
//   * a ciphertext is taken down to one prime; multiply_plain there is refused by SEAL's scale check (2^80 against a 60-bit
//     modulus: "scale out of bounds", the exception of logistic_regression_ckks.cpp:336);
//   * it is refreshed: size 2, first level, the scale it had;
//   * the same multiply_plain is now accepted, and after a rescale the decoded slots are the products;
//   * a size-3 ciphertext and the vector form (one engine call for ciphertexts of one shape) give the same values.
// Exit code 0 = all checks passed.  Needs a HIP device.
#include <cmath>
#include <cstdlib>
#include <iostream>

#include "seal/seal.h"
#include "seal/shim_refresh.h"

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

template <class F>
static bool throws_invalid(F f, const string &needle)
{
    try {
        f();
    } catch (const invalid_argument &e) {
        return string(e.what()).find(needle) != string::npos;
    } catch (...) {
    }
    return false;
}

int main()
{
    const size_t n = 4096;
    const double scale = pow(2.0, 40);
    EncryptionParameters params(scheme_type::CKKS);
    params.set_poly_modulus_degree(n);
    params.set_coeff_modulus(CoeffModulus::Create(n, {60, 40, 40, 40, 40, 40, 40, 40, 60}));
    auto context = SEALContext::Create(params);
    CKKSEncoder encoder(context);
    Evaluator evaluator(context);
    KeyGenerator keygen(context);
    Encryptor encryptor(context, keygen.public_key());
    Decryptor decryptor(context, keygen.secret_key());
    auto relin_keys = keygen.relin_keys();

    const size_t m = 16;
    vector<double> v(m), w(m);
    for (size_t i = 0; i < m; ++i) {
        v[i] = sin(0.37 * (double)i + 0.1);
        w[i] = 0.5 + cos(1.3 * (double)i) * 0.25;
    }
    auto slots = [&](const Ciphertext &c) {
        Plaintext p;
        decryptor.decrypt(c, p);
        vector<double> out;
        encoder.decode(p, out);
        out.resize(m);
        return out;
    };
    auto max_err = [&](const vector<double> &a, const vector<double> &b) {
        double e = 0;
        for (size_t i = 0; i < m; ++i) e = max(e, fabs(a[i] - b[i]));
        return e;
    };
    vector<double> vw(m);
    for (size_t i = 0; i < m; ++i) vw[i] = v[i] * w[i];

    Plaintext pv, pw_first, pw_last;
    encoder.encode(v, scale, pv);
    encoder.encode(w, scale, pw_first);
    encoder.encode(w, context->last_parms_id(), scale, pw_last);
    Ciphertext ct;
    encryptor.encrypt(pv, ct);
    evaluator.mod_switch_to_inplace(ct, context->last_parms_id());
    CHECK(ct.coeff_mod_count() == 1 && ct.parms_id() == context->last_parms_id(), "the ciphertext is down to one prime");
    CHECK(throws_invalid([&] { Ciphertext t; evaluator.multiply_plain(ct, pw_last, t); }, "scale out of bounds"),
          "multiply_plain at the last prime: scale out of bounds");

    Ciphertext fresh;
    hefx_refresh(decryptor, encryptor, ct, fresh);
    CHECK(fresh.size() == 2 && fresh.parms_id() == context->first_parms_id() && fresh.coeff_mod_count() == 8,
          "refreshed: size 2 at the first level");
    CHECK(fresh.scale() == ct.scale(), "refreshed: the scale is unchanged");
    CHECK(max_err(slots(fresh), v) < 1e-6, "refreshed: the slots are the values");
    Ciphertext prod;
    bool accepted = true;
    try {
        evaluator.multiply_plain(fresh, pw_first, prod);
        evaluator.rescale_to_next_inplace(prod);
    } catch (const exception &e) {
        accepted = false;
        cout << "      " << e.what() << endl;
    }
    CHECK(accepted, "multiply_plain after the refresh is accepted");
    if (accepted) {
        CHECK(prod.coeff_mod_count() == 7, "product rescaled to the next level");
        const double err = max_err(slots(prod), vw);
        cout << "      max |decoded - v * w| = " << err << endl;
        CHECK(err < 1e-5, "decoded slots of the product");
    }

    // a size-3 ciphertext (a product that was not relinearised), from two primes
    Ciphertext a, b, three;
    encryptor.encrypt(pv, a);
    Plaintext pw2;
    encoder.encode(w, scale, pw2);
    encryptor.encrypt(pw2, b);
    evaluator.multiply(a, b, three);
    evaluator.rescale_to_next_inplace(three);
    evaluator.mod_switch_to_inplace(three, context->get_context_data(context->last_parms_id())->parms_id());
    CHECK(three.size() == 3 && three.coeff_mod_count() == 1, "a size-3 ciphertext at one prime");
    Ciphertext three_fresh;
    hefx_refresh(decryptor, encryptor, three, three_fresh);
    CHECK(three_fresh.size() == 2 && three_fresh.parms_id() == context->first_parms_id(), "size 3 refreshed to size 2, first level");
    CHECK(max_err(slots(three_fresh), vw) < 1e-5, "size 3 refreshed: the slots are the products");

    // the vector form: one engine call for ciphertexts of one shape
    vector<Ciphertext> many(3), many_fresh;
    for (size_t i = 0; i < many.size(); ++i) {
        encryptor.encrypt(pv, many[i]);
        evaluator.mod_switch_to_inplace(many[i], context->last_parms_id());
    }
    hefx_refresh(decryptor, encryptor, many, many_fresh);
    bool all_ok = many_fresh.size() == 3;
    for (size_t i = 0; all_ok && i < many_fresh.size(); ++i)
        all_ok = many_fresh[i].size() == 2 && many_fresh[i].parms_id() == context->first_parms_id() &&
                 many_fresh[i].scale() == many[i].scale() && max_err(slots(many_fresh[i]), v) < 1e-6;
    CHECK(all_ok, "vector form: three ciphertexts refreshed in one call");
    // ... and already at the first level: a plain re-encryption
    Ciphertext top, top_fresh;
    encryptor.encrypt(pv, top);
    hefx_refresh(decryptor, encryptor, top, top_fresh);
    CHECK(top_fresh.parms_id() == context->first_parms_id() && max_err(slots(top_fresh), v) < 1e-6, "refresh at the first level");
    Ciphertext empty;
    CHECK(throws_invalid([&] { Ciphertext t; hefx_refresh(decryptor, encryptor, empty, t); }, "not valid"), "an empty ciphertext is refused");

    cout << (failures ? "SELFTEST FAILED" : "SELFTEST PASSED") << endl;
    return failures ? 1 : 0;
}
