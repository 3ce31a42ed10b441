// bfv_front_selftest.cpp -- the BFV calls of include/seal/seal.h that run on the engine besides multiply and decrypt
// (include/hefx_bfv.h: hefx_bfv_scale_plain_add, hefx_bfv_lift_plain, hefx_bfv_noise_budget, hefx_bfv_batch_encode /
// _decode), against the host functions they replaced (include/seal/seal.h bfv_scaled_plain / bfv_lifted_plain,
// include/seal/shim_bfv.h decrypt_round_host's `worst` and PlainNtt), on the same inputs:
//   * the words of the device entries equal the host functions', with an odd coefficient count and onto a random c0;
//   * the words of Encryptor-independent Evaluator::add_plain / multiply_plain equal the parent's host-built operands
//     pushed through the same engine calls;
//   * invariant_noise_budget is the number decrypt_round_host's `worst` gives, fresh and after each operation;
//   * BatchEncoder::encode / decode give PlainNtt's words, and encode -> encrypt -> add_plain -> multiply_plain ->
//     decrypt -> decode is (x + y) * z modulo t in every slot (without batching: in every coefficient, z a constant);
//   * all of it again one level below the top, after mod_switch_to_next.
// At BFVDefault(4096) with t = 1024 (no batching: BatchEncoder's constructor throws) and BFVDefault(8192) with
// t = 1032193.  Exit code 0 = all checks passed.  Needs a HIP device.
//
//   bfv_front_selftest --time N t reps   times one encrypt, add_plain, multiply_plain, invariant_noise_budget and (with
//                                        batching) BatchEncoder::encode / decode, device idle before and after each, and
//                                        prints one JSON line of median / min / max (tools/bfv_front_bench.py).  Compiled
//                                        with -DBFV_FRONT_PUBLIC_API_ONLY it uses nothing but SEAL's class API, so that
//                                        the same source times an older seal.h.
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
};

static vector<uint64_t> values(size_t n, uint64_t t, uint64_t seed)  // n words below t; 0, t - 1 and both sides of t/2 in front
{
    vector<uint64_t> v(n);
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    for (auto &c : v) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        c = (s >> 11) % t;
    }
    const uint64_t special[] = {0, 1, t - 1, t / 2, min(t / 2 + 1, t - 1)};
    for (size_t i = 0; i < 5 && i < n; ++i) v[i] = special[i];
    if (n) v[n - 1] = t - 1;
    return v;
}
static Plaintext plain_of(const vector<uint64_t> &coeffs)
{
    Plaintext p;
    p.bfv = coeffs;
    return p;
}

struct Stat {
    vector<double> v;
    string json() const
    {
        vector<double> s(v);
        sort(s.begin(), s.end());
        if (s.empty()) return "null";
        return "{\"median_ms\": " + to_string(s[s.size() / 2]) + ", \"min_ms\": " + to_string(s.front()) + ", \"max_ms\": " + to_string(s.back()) + "}";
    }
};

static int time_mode(size_t n, uint64_t t, int reps)
{
    Bfv B(n, t);
    unique_ptr<BatchEncoder> be;
    try {
        be.reset(new BatchEncoder(B.context));
    } catch (const invalid_argument &) {
    }
    const Plaintext px = plain_of(values(n, t, 1)), py = plain_of(values(n, t, 2));
    const vector<uint64_t> slots = values(n, t, 3);
    Ciphertext c, c2, c3;
    Plaintext pe;
    vector<uint64_t> back;
    auto sync = [&] { (void)hefx_stream_sync(B.context->engine()->live(), nullptr); };
    auto timed = [&](auto f) {
        sync();
        const auto t0 = chrono::steady_clock::now();
        f();
        sync();
        return chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    };
    Stat enc, addp, mulp, budget, benc, bdec;
    int bits = 0;
    for (int r = -2; r < reps; ++r) {  // two warm-up rounds
        const double a = timed([&] { B.encryptor->encrypt(px, c); });
        const double b = timed([&] { B.evaluator->add_plain(c, py, c2); });
        const double m = timed([&] { B.evaluator->multiply_plain(c, py, c3); });
        const double nb = timed([&] { bits = B.decryptor->invariant_noise_budget(c); });
        double e = 0, d = 0;
        if (be) {
            e = timed([&] { be->encode(slots, pe); });
            d = timed([&] { be->decode(pe, back); });
        }
        if (r < 0) continue;
        enc.v.push_back(a), addp.v.push_back(b), mulp.v.push_back(m), budget.v.push_back(nb);
        if (be) benc.v.push_back(e), bdec.v.push_back(d);
    }
    cout << "{\"n\": " << n << ", \"t\": " << t << ", \"reps\": " << reps << ", \"batching\": " << (be ? "true" : "false")
         << ", \"fresh_budget_bits\": " << bits;
#ifndef BFV_FRONT_PUBLIC_API_ONLY
    cout << ", \"on_device\": " << (B.decryptor->shim_bfv_on_device(c) ? "true" : "false");
#endif
    cout << ", \"encrypt\": " << enc.json() << ", \"add_plain\": " << addp.json() << ", \"multiply_plain\": " << mulp.json()
         << ", \"noise_budget\": " << budget.json();
    if (be) cout << ", \"batch_encode\": " << benc.json() << ", \"batch_decode\": " << bdec.json();
    cout << "}" << endl;
    return 0;
}

#ifndef BFV_FRONT_PUBLIC_API_ONLY
static vector<uint64_t> words(const Ciphertext &c) { return shim::download(c.buf); }

// the device entries themselves against the host functions, at the level with L data primes
static void entries_against_host(Bfv &B, int L, const string &tag)
{
    auto &ctx = *B.context;
    auto &e = ctx.engine();
    const size_t n = ctx.n();
    const uint64_t t = ctx.plain_modulus_value();
    hefx_bfv *dev = ctx.bfv_device(ctx.bfv(L));
    if (!dev) {
        cout << "note: " << tag << "host fall-back (the engine does not serve this shape)" << endl;
        return;
    }
    const vector<uint64_t> m = values(n - 1, t, 11);  // an odd count: the last 16-byte record is half message
    auto dm = shim::upload(e, m);
    const vector<uint64_t> scaled = shim::bfv_scaled_plain(ctx, m, L), lifted = shim::bfv_lifted_plain(ctx, m, L);
    auto out = shim::new_buf(e, (size_t)L * n);
    shim::check(hefx_bfv_scale_plain_add(dev, dm->p, (int)m.size(), nullptr, out->p, nullptr));
    CHECK(shim::download(out) == scaled, tag + "scale_plain_add onto zeros == bfv_scaled_plain");
    vector<uint64_t> c0((size_t)L * n), want((size_t)L * n);
    for (int j = 0; j < L; ++j) {
        const uint64_t q = ctx.primes()[j];
        const vector<uint64_t> r = values(n, q, 20 + j);
        for (size_t i = 0; i < n; ++i) {
            c0[j * n + i] = i == 7 ? q - 1 : r[i];
            want[j * n + i] = (uint64_t)(((shim::bfv::u128)c0[j * n + i] + scaled[j * n + i]) % q);
        }
    }
    auto dc = shim::upload(e, c0);
    shim::check(hefx_bfv_scale_plain_add(dev, dm->p, (int)m.size(), dc->p, out->p, nullptr));
    CHECK(shim::download(out) == want && shim::download(dc) == c0, tag + "scale_plain_add onto c0 == c0 + bfv_scaled_plain");
    shim::check(hefx_bfv_scale_plain_add(dev, dm->p, (int)m.size(), dc->p, dc->p, nullptr));
    CHECK(shim::download(dc) == want, tag + "scale_plain_add in place");
    shim::check(hefx_bfv_lift_plain(dev, dm->p, (int)m.size(), 0, out->p, nullptr));
    CHECK(shim::download(out) == lifted, tag + "lift_plain == bfv_lifted_plain");
    auto lt = shim::upload(e, lifted);
    shim::check(hefx_ntt_forward(e->ready({}), lt->p, 1, L, 0, nullptr));
    shim::check(hefx_bfv_lift_plain(dev, dm->p, (int)m.size(), 1, out->p, nullptr));
    CHECK(shim::download(out) == shim::download(lt), tag + "lift_plain in NTT form == hefx_ntt_forward(bfv_lifted_plain)");
    CHECK(shim::download(dm) == m, tag + "the message is left as it was");
}

static void run_case(size_t n, uint64_t t, bool batching)
{
    const string top = "N = " + to_string(n) + ", t = " + to_string(t) + ": ";
    Bfv B(n, t);
    auto &ctx = *B.context;
    auto &ev = *B.evaluator;
    auto &dec = *B.decryptor;
    auto &e = ctx.engine();
    const int Ltop = ctx.bfv_top_level();

    unique_ptr<BatchEncoder> be;
    try {
        be.reset(new BatchEncoder(B.context));
    } catch (const invalid_argument &) {
    }
    CHECK((be != nullptr) == batching, top + (batching ? "BatchEncoder is served" : "BatchEncoder's constructor throws as before"));
    CHECK((hefx_bfv_batching(ctx.bfv_device(ctx.bfv())) != 0) == batching, top + "hefx_bfv_batching agrees");

    auto same_budget = [&](const Ciphertext &c, const string &what) {
        Plaintext ph;
        int bh = -1;
        const int bd = dec.invariant_noise_budget(c);
        dec.shim_decrypt_bfv_host(c, ph, bh);
        CHECK(bd == bh && bd > 0, what + ": invariant_noise_budget " + to_string(bd) + " == decrypt_round_host's " + to_string(bh));
    };
    // the plaintexts: slots when the modulus batches, else polynomials and a constant factor
    const vector<uint64_t> x = values(n, t, 1), y = values(n, t, 2);
    vector<uint64_t> z = values(n, t, 3);
    Plaintext px, py, pz;
    if (be) {
        be->encode(x, px), be->encode(y, py), be->encode(z, pz);
        const auto &P = ctx.bfv().pntt;
        int logn = 0;
        while (((size_t)1 << logn) < n) ++logn;
        vector<size_t> index(n);
        uint64_t pos = 1;
        for (size_t i = 0; i < n / 2; ++i) {
            index[i] = shim::bfv::PlainNtt::bitrev((uint32_t)((pos - 1) >> 1), logn);
            index[n / 2 + i] = shim::bfv::PlainNtt::bitrev((uint32_t)((2 * n - pos - 1) >> 1), logn);
            pos = (pos * 3) & (2 * n - 1);
        }
        for (size_t count : {(size_t)1, n / 2 + 1, n}) {
            vector<uint64_t> host(n, 0), part(x.begin(), x.begin() + count), back, fwd;
            for (size_t i = 0; i < count; ++i) host[index[i]] = part[i];
            P.inverse(host);
            Plaintext pd;
            be->encode(part, pd);
            CHECK(pd.bfv == host, top + "BatchEncoder::encode of " + to_string(count) + " values == PlainNtt::inverse");
            be->decode(pd, back);
            fwd = host;
            P.forward(fwd);
            vector<uint64_t> hostback(n);
            for (size_t i = 0; i < n; ++i) hostback[i] = fwd[index[i]];
            part.resize(n, 0);
            CHECK(back == hostback && back == part, top + "BatchEncoder::decode == PlainNtt::forward, and the values again");
        }
    } else {
        px = plain_of(x), py = plain_of(y);
        z.assign(1, t - 3);
        pz = plain_of(z);
    }

    for (int drop = 0; drop <= 1; ++drop) {
        const int L = Ltop - drop;
        if (L < 1) break;
        const string tag = top + (drop ? "one level down: " : "");
        entries_against_host(B, L, tag);
        Ciphertext c, ca, cm;
        B.encryptor->encrypt(px, c);
        if (drop) ev.mod_switch_to_next_inplace(c);
        if (!dec.shim_bfv_on_device(c)) cout << "note: " << tag << "host fall-back (the engine does not serve this shape)" << endl;
        same_budget(c, tag + "fresh");
        if (!drop) {  // encryption is pk * u + e plus Delta m: the difference of two encryptions under one sampler state is not
                      // available, so the message term is checked by decrypting
            Plaintext pd;
            dec.decrypt(c, pd);
            Plaintext w = px;
            while (w.bfv.size() > 1 && w.bfv.back() == 0) w.bfv.pop_back();
            CHECK(pd.bfv == w.bfv, tag + "decrypt(encrypt(x)) == x");
        }
        ev.add_plain(c, py, ca);
        {  // the parent's path: Delta * y built on the host and added by hefx_add_plain
            auto dm = shim::upload(e, shim::bfv_scaled_plain(ctx, py.bfv, L));
            auto ref = shim::new_buf(e, c.buf->words);
            shim::check(hefx_add_plain(e->ready({c.buf.get()}), L, (int)c.size(), c.buf->p, dm->p, ref->p, nullptr));
            CHECK(words(ca) == shim::download(ref), tag + "words of add_plain == bfv_scaled_plain + hefx_add_plain");
        }
        same_budget(ca, tag + "after add_plain");
        ev.multiply_plain(ca, pz, cm);
        {  // the parent's path: the lifted plaintext built on the host, transformed, multiplied in the NTT domain
            auto pt = shim::upload(e, shim::bfv_lifted_plain(ctx, pz.bfv, L));
            auto tmp = shim::new_buf(e, ca.buf->words), ref = shim::new_buf(e, ca.buf->words);
            shim::check(hefx_ntt_forward(e->ready({}), pt->p, 1, L, 0, nullptr));
            shim::check(hefx_copy(e->ready({ca.buf.get()}), tmp->p, ca.buf->p, ca.buf->words * 8, nullptr));
            shim::check(hefx_ntt_forward(e->ready({}), tmp->p, (int)ca.size(), L, 0, nullptr));
            shim::check(hefx_multiply_plain(e->ready({}), L, (int)ca.size(), 1, tmp->p, pt->p, ref->p, nullptr));
            shim::check(hefx_ntt_inverse(e->ready({}), ref->p, (int)ca.size(), L, 0, nullptr));
            CHECK(words(cm) == shim::download(ref), tag + "words of multiply_plain == bfv_lifted_plain through the same engine calls");
        }
        same_budget(cm, tag + "after multiply_plain");
        Plaintext pr;
        dec.decrypt(cm, pr);
        vector<uint64_t> got;
        if (be)
            be->decode(pr, got);
        else
            got = pr.bfv, got.resize(n, 0);
        bool ok = got.size() == n;
        for (size_t i = 0; ok && i < n; ++i)
            ok = got[i] == (uint64_t)((shim::bfv::u128)((x[i] + y[i]) % t) * (be ? z[i] : z[0]) % t);
        CHECK(ok, tag + "encode -> encrypt -> add_plain -> multiply_plain -> decrypt -> decode == (x + y) * z modulo t");
    }
}
#endif

int main(int argc, char **argv)
{
    if (argc >= 2 && string(argv[1]) == "--time") {
        if (argc < 5) {
            cerr << "usage: bfv_front_selftest --time N t reps" << endl;
            return 2;
        }
        return time_mode((size_t)atoll(argv[2]), (uint64_t)strtoull(argv[3], nullptr, 10), atoi(argv[4]));
    }
#ifdef BFV_FRONT_PUBLIC_API_ONLY
    cerr << "built with the class API only: --time N t reps" << endl;
    return 2;
#else
    run_case(4096, 1024, false);
    run_case(8192, 1032193, true);
    cout << (failures ? "SELFTEST FAILED" : "SELFTEST PASSED") << endl;
    return failures ? 1 : 0;
#endif
}
