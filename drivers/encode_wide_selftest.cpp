// encode_wide_selftest.cpp -- CKKSEncoder at any scale through include/seal/seal.h:
//   * encode(vector<complex<double>>) -> decode(vector<complex<double>>&) round trip, within a float64 decoder's band of
//     the coefficients actually held, at a narrow (2^40) and a wide (2^80) scale;
//   * the real overloads agree with the complex ones on real input, word for word;
//   * encode(double) == hefx_ckks_encode_scalar's words == round(value * scale) mod q_j in every slot;
//   * a wide encode inside a recorded program leaves the words of the call-by-call run;
//   * SEAL's checks and messages on the new overloads.
// With SEAL_SHIM_HOST_ENCODE=1 in the environment the same program runs the host fallback, and adds a scale above 2^128
// (which the fallback's 128-bit cast used to break): the scalar's words exactly, the vector by its round trip.
// Exit code 0 = all checks passed.  Needs a HIP device.
#include <cmath>
#include <complex>
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

// round(value * scale) mod q for an integer-valued double of any size: m * 2^e with m < 2^53
static uint64_t residue(double co, uint64_t q)
{
    int ex = 0;
    const double fr = frexp(fabs(co), &ex);
    const int sh = ex > 53 ? ex - 53 : 0;
    const uint64_t m = (uint64_t)ldexp(fr, ex - sh);
    const uint64_t r = shim::mulmod(m % q, shim::powmod(2, (uint64_t)sh, q), q);
    return co < 0 ? (r ? q - r : 0) : r;
}

int main()
{
    const char *he = getenv("SEAL_SHIM_HOST_ENCODE");
    const bool host = he && *he && *he != '0';
    const size_t n = 4096;
    EncryptionParameters params(scheme_type::CKKS);
    params.set_poly_modulus_degree(n);
    params.set_coeff_modulus(CoeffModulus::Create(n, {60, 50, 50, 50, 60}));  // four data rows: 210 bits
    auto context = SEALContext::Create(params);
    CKKSEncoder encoder(context);
    Evaluator evaluator(context);
    KeyGenerator keygen(context);
    Encryptor encryptor(context, keygen.public_key());
    const auto &q = context->primes();
    const int L = 4;

    vector<complex<double>> vc(n / 2);
    vector<double> vr(n / 2);
    for (size_t i = 0; i < n / 2; ++i) {
        vc[i] = complex<double>(sin(0.37 * (double)i + 0.1), cos(1.91 * (double)i) * 0.8);
        vr[i] = sin(0.61 * (double)i + 0.3);
    }
    auto max_err = [&](const vector<complex<double>> &a, const vector<complex<double>> &b) {
        double e = 0;
        for (size_t i = 0; i < a.size(); ++i) e = max(e, abs(a[i] - b[i]));
        return e;
    };

    // The plaintext holds integers within 0.5 + (encoder's band) of the exact coefficients, so its slots are within
    // sqrt(N) * (0.5 + band) / scale of the values (a slot is a sum of N coefficients times roots; 2-norm bound), and a
    // float64 decoder adds sqrt(N) (E + (4L + 2) u) max|z| < 1e-11 (tests/exact_ckks.py (d)).  The encoder's band is below
    // 2^-40 * scale * max|v| (hefx.h), i.e. below 2^-40 in the slots: 1e-11 + 64 * (0.5 / scale + 2^-40) < 1e-10 from 2^40 up.
    for (double scale : {pow(2.0, 40), pow(2.0, 80), host ? pow(2.0, 140) : pow(2.0, 120)}) {
        Plaintext pc, pr, prc;
        vector<complex<double>> back, backr;
        vector<double> backd;
        encoder.encode(vc, scale, pc);
        encoder.decode(pc, back);
        CHECK(back.size() == n / 2 && max_err(back, vc) < 1e-10 && pc.scale() == scale && pc.parms_id() == context->first_parms_id(),
              "complex encode -> complex decode at scale 2^" << log2(scale) << ": error " << max_err(back, vc));
        encoder.encode(vr, scale, pr);
        vector<complex<double>> vrc(vr.begin(), vr.end());
        encoder.encode(vrc, scale, prc);
        CHECK(shim::download(pr.buf) == shim::download(prc.buf),
              "real and complex overloads agree word for word on real input at scale 2^" << log2(scale));
        encoder.decode(pr, backd);
        encoder.decode(pr, backr);
        double e = 0, eim = 0;
        for (size_t i = 0; i < n / 2; ++i) {
            e = max(e, fabs(backd[i] - vr[i]));
            eim = max(eim, max(fabs(backr[i].imag()), fabs(backr[i].real() - backd[i])));
        }
        CHECK(e < 1e-10 && eim < 1e-10, "real decode == real part of the complex decode at scale 2^" << log2(scale));
    }

    // scalars: every word of row j is round(value * scale) mod q_j
    for (double scale : {pow(2.0, 40), pow(2.0, 80), host ? pow(2.0, 140) : pow(2.0, 120)}) {
        bool ok = true;
        for (double value : {1.5, -0.37, 0.0, 12345.678}) {
            Plaintext p;
            encoder.encode(value, scale, p);
            const auto w = shim::download(p.buf);
            const double co = round(value * scale);
            for (int j = 0; j < L && ok; ++j)
                for (size_t i = 0; i < n && ok; i += 97) ok = w[(size_t)j * n + i] == residue(co, q[j]);
            ok = ok && w.size() == (size_t)L * n && p.is_zero() == (co == 0.0);
        }
        CHECK(ok, "encode(double) holds round(value * scale) mod q_j in every row at scale 2^" << log2(scale));
    }

    // SEAL's checks on the new overloads
    {
        Plaintext p;
        vector<complex<double>> big(n / 2 + 1, 1.0), out;
        CHECK(throws_invalid([&] { encoder.encode(big, pow(2.0, 40), p); }, "values has invalid size"), "complex encode: too many values");
        CHECK(throws_invalid([&] { encoder.encode(vc, -1.0, p); }, "scale out of bounds") &&
                  throws_invalid([&] { encoder.encode(vc, pow(2.0, 211), p); }, "scale out of bounds"),
              "complex encode: scale out of bounds");
        CHECK(throws_invalid([&] { encoder.encode(vc, parms_id_type{{1, 2, 3, 4}}, pow(2.0, 40), p); }, "parms_id is not valid"),
              "complex encode: unknown parms_id");
        Plaintext empty;
        CHECK(throws_invalid([&] { encoder.decode(empty, out); }, "plain is not valid"), "complex decode: an empty plaintext");
    }

    // a wide encode inside a recorded program: x * y at 2^80, plus z encoded at that scale, recorded and live
    {
        auto run = [&](bool lazy) {
            context->engine()->lazy = lazy;
            Plaintext px, py, pz, ps;
            Ciphertext cx, prod, sum, sum2;
            encoder.encode(vr, pow(2.0, 40), px);
            encryptor.encrypt(px, cx);
            encoder.encode(vector<double>(n / 2, 0.75), pow(2.0, 40), py);
            evaluator.multiply_plain(cx, py, prod);
            encoder.encode(vr, prod.scale(), pz);          // wide: 2^80
            evaluator.add_plain(prod, pz, sum);
            encoder.encode(-0.5, prod.scale(), ps);        // scalar at 2^80
            evaluator.add_plain(sum, ps, sum2);
            vector<vector<uint64_t>> words{shim::download(pz.buf), shim::download(ps.buf), shim::download(sum.buf)};
            // (the ciphertext itself differs from run to run: fresh encryption randomness; sum - prod does not)
            Ciphertext d;
            evaluator.sub(sum2, prod, d);
            words.push_back(shim::download(d.buf));
            context->engine()->lazy = true;
            return words;
        };
        const auto live = run(false), lazy = run(true);
        CHECK(live[0] == lazy[0] && live[1] == lazy[1] && live[3] == lazy[3],
              "a wide encode and a wide scalar inside a recorded program leave the words of the call-by-call run");
        // several wide encodes collected by the recorder go out as one batch: the words of single calls
        context->engine()->lazy = true;
        vector<Plaintext> ps(5);
        vector<vector<double>> vs(5, vr);
        for (int i = 0; i < 5; ++i) {
            for (auto &t : vs[i]) t *= (double)(i + 1) * 0.2;   // magnitudes from 2^62 up, at a scale with mantissa bits
            encoder.encode(vs[i], pow(2.0, 64) * 1.25, ps[i]);
        }
        vector<vector<uint64_t>> rec;
        for (auto &p : ps) rec.push_back(shim::download(p.buf));
        context->engine()->lazy = false;
        bool same = true;
        for (int i = 0; i < 5; ++i) {
            Plaintext p;
            encoder.encode(vs[i], pow(2.0, 64) * 1.25, p);
            same = same && shim::download(p.buf) == rec[i];
        }
        context->engine()->lazy = true;
        CHECK(same, "five recorded wide encodes (one batch) == five immediate ones");
    }

    cout << (failures ? "SELFTEST FAILED" : "SELFTEST PASSED") << endl;
    return failures ? 1 : 0;
}
