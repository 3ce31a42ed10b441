// ct_sizes_selftest.cpp -- ciphertexts of any size through include/seal/seal.h:
//   * multiply of a size-3 by a size-2 and by a size-3 ciphertext, against hefx_multiply_sizes on the same buffers and
//     against the plaintext product;
//   * relinearize_inplace from size 4 and 5 with relin_keys(3), and "not enough relinearization keys" with relin_keys(1);
//   * a save / load round trip of that key set (every power comes back, bit for bit) and the same evaluation with the
//     loaded keys, bit for bit;
//   * add / sub of ciphertexts of unequal sizes against the padded form;
//   * the whole sequence recorded (lazy) and live: the same words.
// Exit code 0 = all checks passed.  Needs a HIP device.
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <sstream>

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

int main()
{
    EncryptionParameters params(scheme_type::CKKS);
    params.set_poly_modulus_degree(8192);
    params.set_coeff_modulus(CoeffModulus::Create(8192, {50, 30, 30, 30, 30, 50}));
    auto context = SEALContext::Create(params);
    KeyGenerator keygen(context);
    PublicKey pk = keygen.public_key();
    SecretKey sk = keygen.secret_key();
    RelinKeys rk3 = keygen.relin_keys(3);
    Encryptor encryptor(context, pk);
    Evaluator evaluator(context);
    Decryptor decryptor(context, sk);
    CKKSEncoder encoder(context);
    const double scale = pow(2.0, 30);
    const vector<double> vx{0.5, -1.0, 0.25, 0.9}, vy{-0.5, 0.75, 1.0, -0.3}, vz{1.0, 0.5, -0.25, 0.6}, vw{0.8, -0.4, 0.6, 1.0};

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
    auto err4 = [&](const Ciphertext &c, const vector<double> &want) {
        auto r = dec(c);
        double e = 0;
        for (int j = 0; j < 4; j++) e = max(e, fabs(r[j] - want[j]));
        return e;
    };
    const Ciphertext x = enc(vx, scale), y = enc(vy, scale), z = enc(vz, scale), w = enc(vw, scale);
    vector<double> xyz(4), xyzw(4), xy(4);
    for (int j = 0; j < 4; j++) xy[j] = vx[j] * vy[j], xyz[j] = xy[j] * vz[j], xyzw[j] = xyz[j] * vw[j];

    CHECK(rk3.size() == 3 && rk3.has_power(2) && rk3.has_power(3) && rk3.has_power(4) && !rk3.has_power(5) &&
              RelinKeys::get_index(4) == 2 && rk3.key(3).size() == 5,
          "relin_keys(3): the keys of s^2, s^3, s^4 under index power - 2");
    CHECK(keygen.relin_keys().size() == 1 && throws_invalid([&] { keygen.relin_keys(0); }, "invalid count") &&
              throws_invalid([&] { keygen.relin_keys(15); }, "invalid count"),
          "relin_keys(): one key; counts outside 1 .. 14 are refused");

    // the sequence under test, on fixed inputs: every result's words, in order
    auto run = [&](bool lazy, const RelinKeys &keys) {
        context->engine()->lazy = lazy;
        vector<vector<uint64_t>> words;
        Ciphertext p3, p4, p5, r4, r5, s1, s2, d1, d2;
        evaluator.multiply(x, y, p3);        // 2 x 2 (recorded when lazy)
        evaluator.multiply(p3, z, p4);       // 3 x 2
        evaluator.multiply(p3, p3, p5);      // 3 x 3, a square
        r4 = p4;
        evaluator.relinearize_inplace(r4, keys);
        r5 = p5;
        evaluator.relinearize_inplace(r5, keys);
        Ciphertext x3 = x;
        x3.scale() = p4.scale();
        evaluator.add(p4, x3, s1);           // 4 + 2
        evaluator.add(x3, p4, s2);
        evaluator.sub(p4, x3, d1);
        evaluator.sub(x3, p4, d2);           // the tail of the subtrahend is negated
        evaluator.rescale_to_next_inplace(r4);
        for (const Ciphertext *c : {&p3, &p4, &p5, &r4, &r5, &s1, &s2, &d1, &d2}) words.push_back(shim::download(c->buf));
        context->engine()->lazy = true;
        return words;
    };
    const auto live = run(false, rk3), lazy = run(true, rk3);
    CHECK(live == lazy, "recorded and live evaluation give the same words");

    // against the C-ABI on the same buffers and against the plaintext products
    {
        Ciphertext p3, p4, p5;
        evaluator.multiply(x, y, p3);
        evaluator.multiply(p3, z, p4);
        evaluator.square(p3, p5);
        CHECK(p4.size() == 4 && p5.size() == 5 && p4.scale() == scale * scale * scale && p5.parms_id() == x.parms_id(),
              "multiply: size(a) + size(b) - 1 polynomials, product of the scales, same level");
        auto eng = context->engine();
        auto o4 = shim::new_buf(eng, p4.buf->words), o5 = shim::new_buf(eng, p5.buf->words);
        const int rc4 = hefx_multiply_sizes(eng->live(), x.rows, 3, p3.buf->p, 2, z.buf->p, o4->p, nullptr);
        const int rc5 = hefx_multiply_sizes(eng->live(), x.rows, 3, p3.buf->p, 3, p3.buf->p, o5->p, nullptr);
        CHECK(rc4 == HEFX_OK && rc5 == HEFX_OK && shim::download(o4) == shim::download(p4.buf) &&
                  shim::download(o5) == shim::download(p5.buf) && shim::download(p4.buf) == live[1] && shim::download(p5.buf) == live[2],
              "Evaluator::multiply (3,2) and (3,3) == hefx_multiply_sizes, bit for bit");
        CHECK(err4(p4, xyz) < 1e-2, "the size-4 product decrypts to x * y * z");
        vector<double> sq(4);
        for (int j = 0; j < 4; j++) sq[j] = xy[j] * xy[j];
        CHECK(err4(p5, sq) < 1e-2, "the size-5 square decrypts to (x * y)^2");
        Ciphertext r4 = p4, r5 = p5;
        evaluator.relinearize_inplace(r4, rk3);
        evaluator.relinearize_inplace(r5, rk3);
        CHECK(r4.size() == 2 && r5.size() == 2 && err4(r4, xyz) < 1e-2 && err4(r5, sq) < 1e-2,
              "relinearize_inplace from size 4 and 5 with relin_keys(3): size 2, same values");
        Ciphertext t = p4;
        RelinKeys rk1 = keygen.relin_keys();
        CHECK(throws_invalid([&] { evaluator.relinearize_inplace(t, rk1); }, "not enough relinearization keys") && t.size() == 4,
              "relinearize_inplace: a missing power is SEAL's \"not enough relinearization keys\"");
        Ciphertext big = p5, out;
        for (int i = 0; i < 2; i++) {  // 5 -> 7 -> 9 polynomials (the scale is reset: only the size is under test)
            big.scale() = scale;
            evaluator.multiply(big, p3, out);
            big = out;
        }
        big.scale() = scale;
        CHECK(big.size() == 9 && throws_invalid([&] { evaluator.multiply(big, big, out); }, "invalid size"),
              "multiply: a result of 17 polynomials is refused");
        // unequal sizes against the padded form
        Ciphertext x3 = x, s1, d2;
        x3.scale() = p4.scale();
        evaluator.add(p4, x3, s1);
        evaluator.sub(x3, p4, d2);
        auto hp = shim::download(p4.buf), hx = shim::download(x3.buf);
        vector<uint64_t> pad(hp.size(), 0);
        copy(hx.begin(), hx.end(), pad.begin());
        auto dpad = shim::upload(eng, pad);
        auto os = shim::new_buf(eng, hp.size()), od = shim::new_buf(eng, hp.size());
        shim::check(hefx_add(eng->live(), x.rows, 4, 1, p4.buf->p, dpad->p, os->p, nullptr));
        shim::check(hefx_sub(eng->live(), x.rows, 4, 1, dpad->p, p4.buf->p, od->p, nullptr));
        CHECK(s1.size() == 4 && d2.size() == 4 && shim::download(s1.buf) == shim::download(os) && shim::download(d2.buf) == shim::download(od),
              "add / sub of unequal sizes == the operation on the zero-padded operand, bit for bit");
    }

    // save / load of the key set with several powers, and evaluation with the loaded keys
    {
        stringstream ss;
        rk3.save(ss);
        RelinKeys loaded;
        loaded.load(context, ss);
        bool same = loaded.size() == 3 && loaded.parms_id() == rk3.parms_id();
        for (uint32_t i = 0; i < 3 && same; i++)
            same = loaded.has_key(i) && shim::download(loaded.keys.at(i)) == shim::download(rk3.keys.at(i));
        CHECK(same, "RelinKeys of three powers: save / load gives every key back, bit for bit");
        stringstream s2;
        rk3.save(s2);
        RelinKeys unsafe;
        unsafe.unsafe_load(context, s2);
        CHECK(unsafe.size() == 3 && unsafe.has_power(4), "RelinKeys of three powers: unsafe_load");
        CHECK(run(false, loaded) == live && run(true, loaded) == live, "evaluation with the loaded keys is bit-identical");
    }

    // x * y * z * w with one relinearisation at the end
    {
        Ciphertext p, q;
        evaluator.multiply(x, y, p);
        evaluator.multiply(p, z, q);
        evaluator.multiply(q, w, p);
        CHECK(p.size() == 5, "x * y * z * w without relinearisation has size 5");
        evaluator.relinearize_inplace(p, rk3);
        evaluator.rescale_to_next_inplace(p);
        evaluator.rescale_to_next_inplace(p);
        evaluator.rescale_to_next_inplace(p);
        CHECK(p.size() == 2 && err4(p, xyzw) < 1e-2, "... and decrypts to the product after one relinearize_inplace and three rescales");
    }

    cout << (failures ? "SELFTEST FAILED" : "SELFTEST PASSED") << endl;
    return failures ? 1 : 0;
}
