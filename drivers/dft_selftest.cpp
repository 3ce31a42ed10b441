// dft_selftest.cpp -- seal::hefx_plain_combine (include/seal/shim_dft.h) through include/seal/seal.h, at N = 4096 on
// {60, 40, 40, 40, 60} and scale 2^40.  The fused call is held, WORD FOR WORD, to the shim's own call-by-call operations --
// multiply_plain per term, then add_many -- on a dense pattern (5 ciphertexts, 9 outputs: several tiles in one launch) and on a
// sparse one (an output of one term, a ciphertext no output uses, nullptr in every unroll position).
// Exit code 0 = all checks passed.  Needs a HIP device.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "seal/seal.h"
#include "seal/shim_dft.h"

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

static bool same_as_the_sequence(const Evaluator &evaluator, const vector<Ciphertext> &cts, const vector<vector<const Plaintext *>> &pts,
                                 const vector<Ciphertext> &got, size_t n)
{
    if (got.size() != pts.size()) return false;
    for (size_t g = 0; g < pts.size(); ++g) {
        vector<Ciphertext> prods;
        for (size_t k = 0; k < cts.size(); ++k) {
            if (!pts[g][k]) continue;
            Ciphertext prod;
            evaluator.multiply_plain(cts[k], *pts[g][k], prod);
            prods.push_back(prod);
        }
        Ciphertext sum;
        if (prods.size() == 1)
            sum = prods[0];
        else
            evaluator.add_many(prods, sum);
        const size_t words = 2 * sum.coeff_mod_count() * n;
        if (got[g].size() != 2 || got[g].parms_id() != sum.parms_id() || got[g].scale() != sum.scale() ||
            memcmp(got[g].data(), sum.data(), words * sizeof(uint64_t)) != 0)
            return false;
    }
    return true;
}

int main()
{
    const size_t n = 4096;
    const double scale = pow(2.0, 40);
    EncryptionParameters params(scheme_type::CKKS);
    params.set_poly_modulus_degree(n);
    params.set_coeff_modulus(CoeffModulus::Create(n, {60, 40, 40, 40, 60}));
    auto context = SEALContext::Create(params);
    CKKSEncoder encoder(context);
    Evaluator evaluator(context);
    KeyGenerator keygen(context);
    Encryptor encryptor(context, keygen.public_key());

    const size_t slots = n / 2;
    auto values = [&](unsigned seed) {
        vector<double> v(slots);
        unsigned x = seed * 2654435761u + 12345u;
        for (size_t i = 0; i < slots; ++i) {
            x = x * 1664525u + 1013904223u;
            v[i] = (double)(x >> 8) / (double)(1u << 24) * 2.0 - 1.0;
        }
        return v;
    };
    vector<Ciphertext> cts(5);
    for (size_t k = 0; k < cts.size(); ++k) {
        Plaintext p;
        encoder.encode(values(100 + (unsigned)k), scale, p);
        encryptor.encrypt(p, cts[k]);
    }
    vector<Plaintext> pool(7);
    for (size_t i = 0; i < pool.size(); ++i) encoder.encode(values(200 + (unsigned)i), scale, pool[i]);

    {   // dense: 9 outputs of 5 terms; the seven plaintexts stand in several places
        vector<vector<const Plaintext *>> pts(9, vector<const Plaintext *>(5));
        for (size_t g = 0; g < 9; ++g)
            for (size_t k = 0; k < 5; ++k) pts[g][k] = &pool[(g * 5 + k) % pool.size()];
        vector<Ciphertext> got;
        hefx_plain_combine(evaluator, cts, pts, got);
        CHECK(got.size() == 9 && got[0].scale() == scale * scale && got[0].coeff_mod_count() == 4, "dense: nine outputs at the product scale");
        CHECK(same_as_the_sequence(evaluator, cts, pts, got, n), "dense: the words of multiply_plain per term and add_many");
    }
    {   // sparse
        const Plaintext *X = nullptr, *a = &pool[0], *b = &pool[1], *c = &pool[2], *d = &pool[3];
        vector<vector<const Plaintext *>> pts = {
            {X, X, a, X, X},   // a single term
            {a, X, b, c, X},   // (ciphertext 1 is used by no output)
            {X, X, X, d, a},
            {b, X, X, X, c},
        };
        vector<Ciphertext> got;
        hefx_plain_combine(evaluator, cts, pts, got);
        CHECK(same_as_the_sequence(evaluator, cts, pts, got, n), "sparse: the words of multiply_plain per term and add_many");
    }
    {   // the checks of the sequence
        bool refused = false;
        try {
            vector<Ciphertext> t;
            hefx_plain_combine(evaluator, cts, {{&pool[0], nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr}}, t);
        } catch (const invalid_argument &e) {
            refused = string(e.what()).find("no term") != string::npos;
        }
        CHECK(refused, "an output without a term is refused");
        refused = false;
        try {
            Plaintext zero;
            encoder.encode(0.0, scale, zero);
            vector<Ciphertext> t;
            hefx_plain_combine(evaluator, cts, {{&pool[0], &zero, nullptr, nullptr, nullptr}}, t);
        } catch (const logic_error &e) {
            refused = string(e.what()).find("transparent") != string::npos;
        }
        CHECK(refused, "a zero plaintext is a transparent term");
        refused = false;
        try {
            Plaintext other;
            encoder.encode(values(1), scale * 2.0, other);
            vector<Ciphertext> t;
            hefx_plain_combine(evaluator, cts, {{&pool[0], &other, nullptr, nullptr, nullptr}}, t);
        } catch (const invalid_argument &e) {
            refused = string(e.what()).find("scale mismatch") != string::npos;
        }
        CHECK(refused, "a plaintext at another scale is refused");
    }

    cout << (failures ? "DFT SELFTEST FAILED" : "DFT SELFTEST PASSED") << endl;
    return failures ? 1 : 0;
}
