// bfv_selftest.cpp -- the BFV product and decryption of include/seal/seal.h, which run on the engine
// (include/hefx_bfv.h: hefx_bfv_multiply, hefx_bfv_decrypt_round), against the host path they replaced
// (include/seal/shim_bfv.h: multiply_host, decrypt_round_host), on the same ciphertexts:
//   * the words of Evaluator::square and Evaluator::multiply (2 x 2 and 3 x 3) equal the host path's;
//   * the message of Decryptor::decrypt equals the host rounding's, and invariant_noise_budget is the same number,
//     before and after a product;
//   * (x + y)^2 through add, square, relinearize decrypts to the right slots (where the plain modulus batches).
// At BFVDefault(4096) with t = 65537 and t = 1024 (1_bfv.cpp) and BFVDefault(8192) with t = 1032193 (vector_ops.cpp).
// Exit code 0 = all checks passed.  Needs a HIP device.
//
//   bfv_selftest --time N t reps   times one square and one decrypt, device path and host path alternating in one
//                                  process, and prints one JSON line of medians (tools/bfv_bench.py).  Compiled with
//                                  -DBFV_SELFTEST_PUBLIC_API_ONLY it uses nothing but SEAL's class API (no host path),
//                                  so that the same source times an older seal.h.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <string>

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

static double median(vector<double> v)
{
    sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}

struct Bfv {
    shared_ptr<SEALContext> context;
    unique_ptr<KeyGenerator> keygen;
    unique_ptr<Encryptor> encryptor;
    unique_ptr<Evaluator> evaluator;
    unique_ptr<Decryptor> decryptor;
    Bfv(size_t n, uint64_t t)
    {
        EncryptionParameters bp(scheme_type::BFV);
        bp.set_poly_modulus_degree(n);
        bp.set_coeff_modulus(CoeffModulus::BFVDefault(n));
        bp.set_plain_modulus(t);
        context = SEALContext::Create(bp);
        keygen.reset(new KeyGenerator(context));
        encryptor.reset(new Encryptor(context, keygen->public_key()));
        evaluator.reset(new Evaluator(context));
        decryptor.reset(new Decryptor(context, keygen->secret_key()));
    }
    Plaintext plain(size_t n, uint64_t t, uint64_t seed) const  // n coefficients below t
    {
        Plaintext p;
        p.bfv.resize(n);
        uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
        for (auto &c : p.bfv) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            c = (s >> 11) % t;
        }
        return p;
    }
};

static int time_mode(size_t n, uint64_t t, int reps)
{
    Bfv B(n, t);
    Ciphertext c, sq;
    B.encryptor->encrypt(B.plain(n, t, 1), c);
    Plaintext p;
    auto sync = [&] { (void)hefx_stream_sync(B.context->engine()->live(), nullptr); };
    auto timed = [&](auto f) {
        sync();
        const auto t0 = chrono::steady_clock::now();
        f();
        sync();
        return chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    };
    vector<double> sq_api, dec_api, sq_host, dec_host;
    for (int r = -2; r < reps; ++r) {  // two warm-up rounds
        const double a = timed([&] { B.evaluator->square(c, sq); });
        const double d = timed([&] { B.decryptor->decrypt(c, p); });
        if (r >= 0) sq_api.push_back(a), dec_api.push_back(d);
#ifndef BFV_SELFTEST_PUBLIC_API_ONLY
        int budget = 0;
        const double ah = timed([&] { B.evaluator->shim_multiply_bfv_host(c, c, sq); });
        const double dh = timed([&] { B.decryptor->shim_decrypt_bfv_host(c, p, budget); });
        if (r >= 0) sq_host.push_back(ah), dec_host.push_back(dh);
#endif
    }
    cout << "{\"n\": " << n << ", \"t\": " << t << ", \"reps\": " << reps << ", \"square_ms\": " << median(sq_api)
         << ", \"decrypt_ms\": " << median(dec_api);
#ifndef BFV_SELFTEST_PUBLIC_API_ONLY
    cout << ", \"on_device\": " << (B.decryptor->shim_bfv_on_device(c) ? "true" : "false") << ", \"square_host_ms\": " << median(sq_host)
         << ", \"decrypt_host_ms\": " << median(dec_host);
#endif
    cout << "}" << endl;
    return 0;
}

#ifndef BFV_SELFTEST_PUBLIC_API_ONLY
static vector<uint64_t> words(const Ciphertext &c) { return shim::download(c.buf); }

static void run_case(size_t n, uint64_t t, bool slots)
{
    const string tag = "N = " + to_string(n) + ", t = " + to_string(t) + ": ";
    Bfv B(n, t);
    auto &ev = *B.evaluator;
    auto &dec = *B.decryptor;
    Plaintext px = B.plain(n, t, 1), py = B.plain(n, t, 2);
    Ciphertext cx, cy;
    B.encryptor->encrypt(px, cx);
    B.encryptor->encrypt(py, cy);
    if (!dec.shim_bfv_on_device(cx)) cout << "note: " << tag << "host fall-back (the engine does not serve this shape)" << endl;

    auto same_decrypt = [&](const Ciphertext &c, const string &what) {
        Plaintext pd, ph;
        int bh = -1;
        dec.decrypt(c, pd);
        const int bd = dec.invariant_noise_budget(c);
        dec.shim_decrypt_bfv_host(c, ph, bh);
        CHECK(pd.bfv == ph.bfv, tag + what + ": message of decrypt == decrypt_round_host");
        CHECK(bd == bh && bd > 0, tag + what + ": invariant_noise_budget " + to_string(bd) + " == the host path's " + to_string(bh));
        return pd;
    };
    Plaintext back = same_decrypt(cx, "fresh");
    Plaintext want = px;
    while (want.bfv.size() > 1 && want.bfv.back() == 0) want.bfv.pop_back();
    CHECK(back.bfv == want.bfv, tag + "decrypt(encrypt(x)) == x");

    Ciphertext sq, sqh, m22, m22h, sy, m33, m33h;
    ev.square(cx, sq);
    ev.shim_multiply_bfv_host(cx, cx, sqh);
    CHECK(sq.size() == 3 && words(sq) == words(sqh), tag + "words of square == multiply_host");
    ev.multiply(cx, cy, m22);
    ev.shim_multiply_bfv_host(cx, cy, m22h);
    CHECK(m22.size() == 3 && words(m22) == words(m22h), tag + "words of multiply 2 x 2 == multiply_host");
    ev.square(cy, sy);
    ev.multiply(sq, sy, m33);
    ev.shim_multiply_bfv_host(sq, sy, m33h);
    CHECK(m33.size() == 5 && words(m33) == words(m33h), tag + "words of multiply 3 x 3 == multiply_host");
    same_decrypt(sq, "after square");
    Ciphertext sq_inplace = cx;
    ev.square_inplace(sq_inplace);
    CHECK(words(sq_inplace) == words(sq), tag + "square_inplace == square");

    if (slots) {
        BatchEncoder be(B.context);
        RelinKeys rk = B.keygen->relin_keys();
        const size_t sc = be.slot_count();
        vector<uint64_t> x(sc), y(sc), got;
        for (size_t i = 0; i < sc; ++i) x[i] = (3 * i + 1) % t, y[i] = (i % 7) + 2;
        Plaintext ex, ey, pr;
        be.encode(x, ex);
        be.encode(y, ey);
        Ciphertext a, b;
        B.encryptor->encrypt(ex, a);
        B.encryptor->encrypt(ey, b);
        const int fresh = dec.invariant_noise_budget(a);
        ev.add_inplace(a, b);
        ev.square_inplace(a);
        ev.relinearize_inplace(a, rk);
        pr = same_decrypt(a, "(x + y)^2");
        be.decode(pr, got);
        bool ok = a.size() == 2 && got.size() == sc;
        for (size_t i = 0; ok && i < sc; ++i) ok = got[i] == ((x[i] + y[i]) % t) * ((x[i] + y[i]) % t) % t;
        const int after = dec.invariant_noise_budget(a);
        CHECK(ok && after > 0 && after < fresh, tag + "(x + y)^2 decrypts to the right slots, budget " + to_string(fresh) + " -> " + to_string(after));
    }
}
#endif

int main(int argc, char **argv)
{
    if (argc >= 2 && string(argv[1]) == "--time") {
        if (argc < 5) {
            cerr << "usage: bfv_selftest --time N t reps" << endl;
            return 2;
        }
        return time_mode((size_t)atoll(argv[2]), (uint64_t)strtoull(argv[3], nullptr, 10), atoi(argv[4]));
    }
#ifdef BFV_SELFTEST_PUBLIC_API_ONLY
    cerr << "built with the class API only: --time N t reps" << endl;
    return 2;
#else
    run_case(4096, 65537, true);
    run_case(4096, 1024, false);
    run_case(8192, 1032193, true);
    cout << (failures ? "SELFTEST FAILED" : "SELFTEST PASSED") << endl;
    return failures ? 1 : 0;
#endif
}
