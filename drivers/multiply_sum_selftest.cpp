// multiply_sum_selftest.cpp -- the fused ciphertext product sum through include/seal/seal.h and the C-ABI:
//   * Evaluator::hefx_multiply_sum against multiply + add_many, bit for bit, at d = 4 and d = 40, and its exceptions;
//   * the loop of Linear_Transform_Cipher (helper.h:212-234), restated op by op, against the words of
//     hefx_linear_transform_cipher, with the default power-of-two keys (NAF chains) and with a direct key per step.
// Exit code 0 = all checks passed.  Needs a HIP device.
#include <cmath>
#include <cstdlib>
#include <iostream>

#include "seal/seal.h"

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

// helper.h:212-234, call by call
static Ciphertext lt_cipher(Ciphertext ct, vector<Ciphertext> diags, GaloisKeys gk, Evaluator &evaluator)
{
    Ciphertext ct_rot, ct_new, out;
    evaluator.rotate_vector(ct, -(int)diags.size(), gk, ct_rot);
    evaluator.add(ct, ct_rot, ct_new);
    vector<Ciphertext> res(diags.size());
    evaluator.multiply(ct_new, diags[0], res[0]);
    for (size_t l = 1; l < diags.size(); l++) {
        Ciphertext tmp;
        evaluator.rotate_vector(ct_new, (int)l, gk, tmp);
        evaluator.multiply(tmp, diags[l], res[l]);
    }
    evaluator.add_many(res, out);
    return out;
}

int main()
{
    EncryptionParameters params(scheme_type::CKKS);
    params.set_poly_modulus_degree(8192);
    params.set_coeff_modulus(CoeffModulus::Create(8192, {60, 40, 40, 60}));
    auto context = SEALContext::Create(params);
    KeyGenerator keygen(context);
    PublicKey pk = keygen.public_key();
    SecretKey sk = keygen.secret_key();
    GaloisKeys gk = keygen.galois_keys();
    Encryptor encryptor(context, pk);
    Evaluator evaluator(context);
    Decryptor decryptor(context, sk);
    CKKSEncoder encoder(context);
    const double scale = pow(2.0, 40);

    auto enc = [&](const vector<double> &v, double s) {
        Plaintext p;
        Ciphertext c;
        encoder.encode(v, s, p);
        encryptor.encrypt(p, c);
        return c;
    };
    auto dec = [&](const Ciphertext &c) {
        Plaintext p;
        vector<double> v;
        decryptor.decrypt(c, p);
        encoder.decode(p, v);
        return v;
    };

    // ---- the extension member against multiply + add_many
    for (int d : {4, 40}) {
        vector<Ciphertext> as(d), bs(d), prods(d);
        vector<double> want(8, 0.0);
        for (int i = 0; i < d; i++) {
            vector<double> x(8), y(8);
            for (int j = 0; j < 8; j++) {
                x[j] = 0.05 * ((3 * i + 5 * j) % 13) - 0.3;
                y[j] = 0.04 * ((7 * i + 2 * j) % 11) - 0.2;
            }
            as[i] = enc(x, scale);
            bs[i] = i == 1 ? as[i] : (i % 5 == 2 ? bs[0] : enc(y, scale));  // a square term, one operand repeated
            if (i == 1) y = x;
            if (i != 1 && i % 5 == 2)
                for (int j = 0; j < 8; j++) y[j] = 0.04 * ((2 * j) % 11) - 0.2;
            for (int j = 0; j < 8; j++) want[j] += x[j] * y[j];
        }
        for (int i = 0; i < d; i++) evaluator.multiply(as[i], bs[i], prods[i]);
        Ciphertext ref, fast;
        evaluator.add_many(prods, ref);
        evaluator.hefx_multiply_sum(as, bs, fast);
        CHECK(fast.size() == 3 && fast.scale() == ref.scale() && fast.parms_id() == ref.parms_id() &&
                  shim::download(fast.buf) == shim::download(ref.buf),
              "hefx_multiply_sum == add_many(multiply), bit for bit, d = " + to_string(d));
        auto r = dec(fast);
        double err = 0;
        for (int j = 0; j < 8; j++) err = max(err, fabs(r[j] - want[j]));
        CHECK(err < 1e-4, "hefx_multiply_sum decrypts to the sum of products, d = " + to_string(d));
        if (d == 4) {
            Ciphertext t;
            CHECK(throws_invalid([&] { evaluator.hefx_multiply_sum(as, vector<Ciphertext>(bs.begin(), bs.begin() + 3), t); },
                                 "as many second operands"),
                  "hefx_multiply_sum: unequal list lengths are refused");
            vector<Ciphertext> bad = bs;
            bad[2] = prods[0];
            CHECK(throws_invalid([&] { evaluator.hefx_multiply_sum(as, bad, t); }, "size-2"),
                  "hefx_multiply_sum: a size-3 operand is refused like multiply does");
            bad = bs;
            bad[3] = enc(vector<double>{1.0}, pow(2.0, 30));
            CHECK(throws_invalid([&] { evaluator.hefx_multiply_sum(as, bad, t); }, "scale mismatch"),
                  "hefx_multiply_sum: mismatched scales are refused like add_many does");
            bad = bs;
            bad[0].scale() = pow(2.0, 120);
            CHECK(throws_invalid([&] { evaluator.hefx_multiply_sum(as, bad, t); }, "scale out of bounds"),
                  "hefx_multiply_sum: scale out of bounds like multiply");
            bad = bs;
            evaluator.mod_switch_to_next_inplace(bad[1]);
            CHECK(throws_invalid([&] { evaluator.hefx_multiply_sum(as, bad, t); }, "parameter mismatch"),
                  "hefx_multiply_sum: operands of different levels are refused like multiply does");
        }
    }

    // ---- helper.h:212-234 call by call against hefx_linear_transform_cipher
    for (int variant = 0; variant < 3; variant++) {
        const int d = variant == 0 ? 4 : 13;
        const bool direct = variant == 2;
        vector<vector<double>> M(d, vector<double>(d));
        vector<double> v(d), want(d, 0.0);
        for (int i = 0; i < d; i++) {
            v[i] = 0.1 * (i % 7) - 0.25;
            for (int j = 0; j < d; j++) M[i][j] = 0.01 * ((7 * i + 3 * j) % 11) - 0.05;
        }
        for (int i = 0; i < d; i++)
            for (int j = 0; j < d; j++) want[i] += M[i][j] * v[j];
        vector<Ciphertext> diags(d);
        for (int l = 0; l < d; l++) {
            vector<double> dv(d);
            for (int i = 0; i < d; i++) dv[i] = M[i][(i + l) % d];
            diags[l] = enc(dv, scale);
        }
        GaloisKeys keys = gk;
        if (direct) {
            vector<int> steps{-d};
            for (int l = 1; l < d; l++) steps.push_back(l);
            keys = keygen.galois_keys(steps);
        }
        Ciphertext cv = enc(v, scale);
        Ciphertext ref = lt_cipher(cv, diags, keys, evaluator);
        const vector<uint64_t> ref_words = shim::download(ref.buf);

        auto eng = context->engine();
        vector<const uint64_t *> dp, kp;
        vector<uint32_t> elts;
        for (auto &c : diags) dp.push_back(c.buf->p);
        for (auto &kv : keys.keys) {
            elts.push_back(kv.first);
            kp.push_back(kv.second->p);
        }
        auto out = shim::new_buf(eng, ref_words.size());
        const int rc = hefx_linear_transform_cipher(eng->live(), cv.rows, cv.buf->p, d, dp.data(), (int)kp.size(), elts.data(),
                                                    kp.data(), out->p, nullptr);
        const string tag = "d = " + to_string(d) + (direct ? ", direct keys" : ", default keys");
        CHECK(rc == HEFX_OK && shim::download(out) == ref_words,
              "hefx_linear_transform_cipher == the loop of helper.h:212-234, bit for bit, " + tag);
        auto r = dec(ref);
        double err = 0;
        for (int i = 0; i < d; i++) err = max(err, fabs(r[i] - want[i]));
        CHECK(ref.size() == 3 && err < 1e-4, "Linear_Transform_Cipher decrypts to M.v, " + tag);
        if (direct) {  // steps 1..d-1 keyed directly, -d not at all: the call-by-call loop's exception, from the engine
            vector<int> steps;
            for (int l = 1; l < d; l++) steps.push_back(l);
            GaloisKeys partial = keygen.galois_keys(steps);
            vector<const uint64_t *> pk2;
            vector<uint32_t> pe;
            for (auto &kv : partial.keys) {
                pe.push_back(kv.first);
                pk2.push_back(kv.second->p);
            }
            const int rc2 = hefx_linear_transform_cipher(eng->live(), cv.rows, cv.buf->p, d, dp.data(), (int)pk2.size(), pe.data(),
                                                         pk2.data(), out->p, nullptr);
            CHECK(rc2 == HEFX_ERR_INVALID && string(hefx_last_error()).find("Galois key not present") != string::npos &&
                      throws_invalid([&] { lt_cipher(cv, diags, partial, evaluator); }, "Galois key not present"),
                  "a missing Galois key: the engine's error is the loop's exception");
        }
    }

    cout << (failures ? "SELFTEST FAILED" : "SELFTEST PASSED") << endl;
    return failures ? 1 : 0;
}
