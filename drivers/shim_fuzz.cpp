// shim_fuzz.cpp -- random evaluator programs against include/seal/seal.h: a program run RECORDED (the recorder and fusion
// planner of seal.h: Engine::record / flush / submit_nodes / plan_fusion / flush_multi) must leave the words that the same
// program leaves when every call runs at once (SEAL_SHIM_LAZY=0).  From a seed the generator builds one program over a pool
// of 8 Ciphertext and 6 Plaintext variables; it draws evaluator calls in both spellings, copies, drops, observations and the
// motifs the planner's use-count conditions were written for -- and their near misses.  It prints one line per live
// variable at every observation; two runs of one seed are compared line by line (tests/test_shim_fuzz_cpu.py against the
// symbolic engine of drivers/hefx_symbolic.cpp, tests/test_gpu_shim_fuzz.py against the real one).
//
//   shim_fuzz --seed S [--ops K] [--steps T] [--lazy 0|1] [--pend-mb M] [--ndev D] [--draw-settings] [--chain N] [--dump] [--decode]
//     --ops K      stop after the first K calls (shrinking by hand: the program of a seed does not depend on K or on the mode)
//     --dump       print every call as readable text ("call 17: c3 = rotate_vector(c1, 5, gk)")
//     --chain N    start with a run of N rotate-by-1 + add_inplace pairs (the 2000-level gradient chains of the LR driver)
//     --decode     decrypt and decode the final variables and compare them with the generator's slot model in doubles
//   exit code: 0 ok, 4 the slot model disagrees, 5 an engine error or a failed submission surfaced, 2 usage
// Lines: "obs", "throw" and "end" lines are the same in every mode; "stat", "motifs" and "call" lines are information.
#include <cinttypes>
#include <cstdarg>
#include <initializer_list>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "seal/seal.h"

using namespace seal;

namespace {

struct Rng {  // splitmix64: the same numbers with every standard library
    std::uint64_t s;
    std::uint64_t next()
    {
        std::uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)(next() % (std::uint64_t)n); }
    bool one_in(int n) { return below(n) == 0; }
};

constexpr int NC = 8, NP = 6, SLOTS = 4096;
struct Stop {};

struct CtVar {
    Ciphertext c;
    std::vector<double> m;  // the slot model
    int depth = 0, terms = 1;
};
struct PtVar {
    Plaintext p;
    std::vector<double> m;
    bool zero = false;
};

std::string fmt(const char *f, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

struct Fuzz {
    std::shared_ptr<SEALContext> ctx;
    Evaluator *ev;
    CKKSEncoder *enc;
    Encryptor *encryptor;
    Decryptor *decryptor;
    RelinKeys rk;
    GaloisKeys gk[2];  // gk[0]: the default keys (powers of two, conjugation); gk[1]: steps 1 2 3 5 -1 -2 8 (other buffers)
    Rng R{0};
    long max_ops = -1, ncalls = 0, nthrows = 0, nobs = 0;
    bool dump = false, long_chain = false, engine_error = false;
    long motif[12] = {0};
    CtVar C[NC];
    PtVar P[NP];
    const double S40 = std::pow(2.0, 40);

    // ---- bookkeeping the generator shares with the shim (read from the objects: the same in every mode)
    bool live(int i) const { return (bool)C[i].c.buf; }
    bool plive(int j) const { return (bool)P[j].p.buf; }
    int rows(int i) const { return C[i].c.rows; }
    int bits(int r) const { return ctx->get_context_data(ctx->id_of_rows(r))->total_coeff_modulus_bit_count(); }
    static bool close(double a, double b) { return a == b || std::fabs(a - b) <= std::max(std::fabs(a), std::fabs(b)) * 9.094947017729282e-13; }
    static double maxabs(const std::vector<double> &m)
    {
        double x = 0;
        for (double v : m) x = std::max(x, std::fabs(v));
        return x;
    }
    bool fits(const std::vector<double> &m) const { return long_chain || maxabs(m) <= 8.0; }
    bool scale_ok(double s, int r) const { return s > 0 && std::log2(s) + 5 <= bits(r); }
    static std::vector<double> rotated(const std::vector<double> &m, int step)
    {
        std::vector<double> o(SLOTS, 0.0);
        if (m.size() != (std::size_t)SLOTS || step <= -SLOTS || step >= SLOTS) return o;
        for (int i = 0; i < SLOTS; ++i) o[i] = m[(std::size_t)((i + step + SLOTS) % SLOTS)];
        return o;
    }
    static std::vector<double> combine(const std::vector<double> &a, const std::vector<double> &b, int op)
    {
        std::vector<double> o(SLOTS, 0.0);
        if (a.size() != (std::size_t)SLOTS || b.size() != (std::size_t)SLOTS) return o;
        for (int i = 0; i < SLOTS; ++i) o[i] = op == 0 ? a[i] + b[i] : (op == 1 ? a[i] - b[i] : a[i] * b[i]);
        return o;
    }

    // ---- one call: counted, printed on request, its exception (type and text) part of the output
    template <class F>
    bool call(const std::string &desc, F &&f)
    {
        if (max_ops >= 0 && ncalls >= max_ops) throw Stop{};
        ++ncalls;
        if (dump) std::printf("call %ld: %s\n", ncalls, desc.c_str());
        const char *type = nullptr;
        std::string what;
        try {
            f();
            return true;
        } catch (const std::invalid_argument &e) {
            type = "invalid_argument", what = e.what();
        } catch (const std::logic_error &e) {
            type = "logic_error", what = e.what();
        } catch (const std::runtime_error &e) {
            type = "runtime_error", what = e.what();
        } catch (const std::exception &e) {
            type = "exception", what = e.what();
        }
        ++nthrows;
        if (what.find("symbolic:") != std::string::npos || what.find("hefx:") != std::string::npos ||
            what.find("deferred evaluator operation failed") != std::string::npos)
            engine_error = true;
        std::printf("throw %ld %s: %s\n", ncalls, type, what.c_str());
        return false;
    }

    // ---- the calls
    bool encode_vec(int pj, int r, double scale, int flavor /* 0 values in +-[0.5, 1.5], 1 in +-[0.25, 0.5], 2 zero */)
    {
        static const int lens[3] = {4, 37, SLOTS};
        const int nv = lens[R.below(3)];
        std::vector<double> v((std::size_t)nv, 0.0);
        for (auto &x : v) {
            const double mag = flavor == 1 ? 0.25 + 0.25 * R.below(2) : 0.5 + 0.25 * R.below(5);
            x = flavor == 2 ? 0.0 : (R.below(2) ? mag : -mag);
        }
        const bool ok = call(fmt("p%d = encode(%d values%s, rows %d, scale 2^%.3f)", pj, nv, flavor == 2 ? " all zero" : "", r, std::log2(scale)),
                             [&] { enc->encode(v, ctx->id_of_rows(r), scale, P[pj].p); });
        if (ok) {
            v.resize(SLOTS, 0.0);
            P[pj].m = v;
            P[pj].zero = flavor == 2;
        }
        return ok;
    }
    bool encode_scalar(int pj, int r, double scale)
    {
        const double mag = 0.5 + 0.25 * R.below(5), v = R.below(2) ? mag : -mag;
        const bool ok = call(fmt("p%d = encode(scalar %.2f, rows %d, scale 2^%.3f)", pj, v, r, std::log2(scale)),
                             [&] { enc->encode(v, ctx->id_of_rows(r), scale, P[pj].p); });
        if (ok) {
            P[pj].m.assign(SLOTS, v);
            P[pj].zero = false;
        }
        return ok;
    }
    bool encrypt(int ci, int pj)
    {
        if (!plive(pj)) return false;
        const bool ok = call(fmt("c%d = encrypt(p%d)", ci, pj), [&] { encryptor->encrypt(P[pj].p, C[ci].c); });
        if (ok) C[ci].m = P[pj].m, C[ci].depth = 0, C[ci].terms = 1;
        return ok;
    }
    bool addsub(int d, int a, int b, bool sub)
    {
        const auto m = combine(C[a].m, C[b].m, sub ? 1 : 0);
        const int depth = std::max(C[a].depth, C[b].depth), terms = C[a].terms + C[b].terms;
        const char *nm = sub ? "sub" : "add";
        const bool ok = d == a ? call(fmt("%s_inplace(c%d, c%d)", nm, a, b), [&] { sub ? ev->sub_inplace(C[a].c, C[b].c) : ev->add_inplace(C[a].c, C[b].c); })
                               : call(fmt("c%d = %s(c%d, c%d)", d, nm, a, b), [&] { sub ? ev->sub(C[a].c, C[b].c, C[d].c) : ev->add(C[a].c, C[b].c, C[d].c); });
        if (ok) C[d].m = m, C[d].depth = depth, C[d].terms = terms;
        return ok;
    }
    bool add_plain(int d, int a, int pj)
    {
        const auto m = combine(C[a].m, P[pj].m, 0);
        const int depth = C[a].depth, terms = C[a].terms + 1;
        const bool ok = d == a ? call(fmt("add_plain_inplace(c%d, p%d)", a, pj), [&] { ev->add_plain_inplace(C[a].c, P[pj].p); })
                               : call(fmt("c%d = add_plain(c%d, p%d)", d, a, pj), [&] { ev->add_plain(C[a].c, P[pj].p, C[d].c); });
        if (ok) C[d].m = m, C[d].depth = depth, C[d].terms = terms;
        return ok;
    }
    bool mulpt(int d, int a, int pj)
    {
        const auto m = combine(C[a].m, P[pj].m, 2);
        const int depth = C[a].depth + 1, terms = C[a].terms;
        const bool ok = d == a ? call(fmt("multiply_plain_inplace(c%d, p%d)", a, pj), [&] { ev->multiply_plain_inplace(C[a].c, P[pj].p); })
                               : call(fmt("c%d = multiply_plain(c%d, p%d)", d, a, pj), [&] { ev->multiply_plain(C[a].c, P[pj].p, C[d].c); });
        if (ok) C[d].m = m, C[d].depth = depth, C[d].terms = terms;
        return ok;
    }
    bool mul(int d, int a, int b)
    {
        const auto m = combine(C[a].m, C[b].m, 2);
        const int depth = std::max(C[a].depth, C[b].depth) + 1, terms = C[a].terms * C[b].terms;
        bool ok;
        if (a == b && d == a) ok = call(fmt("square_inplace(c%d)", a), [&] { ev->square_inplace(C[a].c); });
        else if (a == b) ok = call(fmt("c%d = square(c%d)", d, a), [&] { ev->square(C[a].c, C[d].c); });
        else if (d == a) ok = call(fmt("multiply_inplace(c%d, c%d)", a, b), [&] { ev->multiply_inplace(C[a].c, C[b].c); });
        else ok = call(fmt("c%d = multiply(c%d, c%d)", d, a, b), [&] { ev->multiply(C[a].c, C[b].c, C[d].c); });
        if (ok) C[d].m = m, C[d].depth = depth, C[d].terms = terms;
        return ok;
    }
    bool unary(int d, int a, int what /* 0 relinearize, 1 rescale_to_next, 2 mod_switch_to_next */)
    {
        static const char *nm[3] = {"relinearize", "rescale_to_next", "mod_switch_to_next"};
        const std::vector<double> m = C[a].m;
        const int depth = C[a].depth, terms = C[a].terms;
        bool ok;
        if (d == a)
            ok = call(fmt("%s_inplace(c%d)", nm[what], a), [&] {
                if (what == 0) ev->relinearize_inplace(C[a].c, rk);
                else if (what == 1) ev->rescale_to_next_inplace(C[a].c);
                else ev->mod_switch_to_next_inplace(C[a].c);
            });
        else
            ok = call(fmt("c%d = %s(c%d)", d, nm[what], a), [&] {
                if (what == 0) ev->relinearize(C[a].c, rk, C[d].c);
                else if (what == 1) ev->rescale_to_next(C[a].c, C[d].c);
                else ev->mod_switch_to_next(C[a].c, C[d].c);
            });
        if (ok) C[d].m = m, C[d].depth = depth, C[d].terms = terms;
        return ok;
    }
    bool modswitch_pt(int pj)
    {
        return call(fmt("mod_switch_to_next_inplace(p%d)", pj), [&] { ev->mod_switch_to_next_inplace(P[pj].p); });
    }
    bool rot(int d, int a, int step, int ks)
    {
        const auto m = rotated(C[a].m, step);
        const int depth = C[a].depth, terms = C[a].terms;
        const bool ok = d == a ? call(fmt("rotate_vector_inplace(c%d, %d, gk%d)", a, step, ks), [&] { ev->rotate_vector_inplace(C[a].c, step, gk[ks]); })
                               : call(fmt("c%d = rotate_vector(c%d, %d, gk%d)", d, a, step, ks), [&] { ev->rotate_vector(C[a].c, step, gk[ks], C[d].c); });
        if (ok) C[d].m = m, C[d].depth = depth, C[d].terms = terms;
        return ok;
    }
    bool conj(int d, int a)
    {
        const std::vector<double> m = C[a].m;  // real slot values: conjugation leaves them
        const int depth = C[a].depth, terms = C[a].terms;
        const bool ok = d == a ? call(fmt("complex_conjugate_inplace(c%d, gk0)", a), [&] { ev->complex_conjugate_inplace(C[a].c, gk[0]); })
                               : call(fmt("c%d = complex_conjugate(c%d, gk0)", d, a), [&] { ev->complex_conjugate(C[a].c, gk[0], C[d].c); });
        if (ok) C[d].m = m, C[d].depth = depth, C[d].terms = terms;
        return ok;
    }
    bool add_many(int d, const std::vector<int> &ids)
    {
        std::vector<Ciphertext> v;
        std::vector<double> m(SLOTS, 0.0);
        int depth = 0, terms = 0;
        std::string s;
        for (int i : ids) {
            v.push_back(C[i].c);
            m = combine(m, C[i].m, 0);
            depth = std::max(depth, C[i].depth);
            terms += C[i].terms;
            s += fmt("%sc%d", s.empty() ? "" : ", ", i);
        }
        const bool ok = call(fmt("c%d = add_many({%s})", d, s.c_str()), [&] { ev->add_many(v, C[d].c); });
        if (ok) C[d].m = m, C[d].depth = depth, C[d].terms = terms;
        return ok;
    }
    bool copy(int d, int a)
    {
        if (d == a) return false;
        return call(fmt("c%d = c%d", d, a), [&] { C[d] = C[a]; });
    }
    bool drop(int i)
    {
        return call(fmt("c%d = Ciphertext()", i), [&] { C[i] = CtVar(); });
    }
    static std::uint64_t digest(const std::vector<std::uint64_t> &w)
    {
        std::uint64_t h = 0xCBF29CE484222325ull;
        for (std::uint64_t x : w) {
            h ^= x;
            h *= 0x100000001B3ull;
            h ^= h >> 29;
        }
        return h;
    }
    bool observe()
    {
        return call("observe every live variable", [&] {
            ++nobs;
            for (int i = 0; i < NC; ++i) {
                if (!live(i)) continue;
                const auto w = shim::download(C[i].c.buf);
                std::printf("obs %ld c%d size=%zu rows=%d id=%016" PRIx64 " scale=%a digest=%016" PRIx64 "\n", nobs, i, C[i].c.size(), C[i].c.rows,
                            C[i].c.parms_id()[0], C[i].c.scale(), digest(w));
            }
            for (int j = 0; j < NP; ++j) {
                if (!plive(j)) continue;
                const auto w = shim::download(P[j].p.buf, P[j].p.view_words_);
                std::printf("obs %ld p%d rows=%d id=%016" PRIx64 " scale=%a digest=%016" PRIx64 "\n", nobs, j, P[j].p.rows, P[j].p.parms_id()[0],
                            P[j].p.scale(), digest(w));
            }
            const auto &st = ctx->engine()->stats;
            std::printf("stat %ld calls=%zu flushes=%zu nodes=%zu\n", nobs, st.calls, st.flushes, st.nodes);
        });
    }

    // ---- choosing operands
    template <class Pred>
    int pick_ct(Pred pred)
    {
        int cand[NC], n = 0;
        for (int i = 0; i < NC; ++i)
            if (live(i) && pred(i)) cand[n++] = i;
        return n ? cand[R.below(n)] : -1;
    }
    int other(std::initializer_list<int> excl)
    {
        int cand[NC], n = 0;
        for (int i = 0; i < NC; ++i) {
            bool x = false;
            for (int e : excl) x = x || e == i;
            if (!x) cand[n++] = i;
        }
        return cand[R.below(n)];
    }
    int fresh(int ci, int flavor = 0)
    {
        const int pj = R.below(NP);
        encode_vec(pj, ctx->k() - 1, S40, flavor);
        encrypt(ci, pj);
        return ci;
    }
    bool rotatable(int i) const { return C[i].c.size() == 2; }
    int need_ct2()  // a size-2 ciphertext with room above it
    {
        const int i = pick_ct([&](int x) { return rotatable(x) && rows(x) >= 2 && C[x].depth <= 1 && maxabs(C[x].m) <= 2.0 && close(C[x].c.scale(), S40); });
        return i >= 0 ? i : fresh(R.below(NC));
    }
    bool can_mulpt(int a, int pj) const
    {
        return live(a) && plive(pj) && !P[pj].zero && C[a].c.parms_id() == P[pj].p.parms_id() && C[a].depth + 1 <= 2 &&
               scale_ok(C[a].c.scale() * P[pj].p.scale(), rows(a)) && fits(combine(C[a].m, P[pj].m, 2));
    }
    bool can_mul(int a, int b) const
    {
        return live(a) && live(b) && C[a].c.parms_id() == C[b].c.parms_id() && C[a].c.size() + C[b].c.size() - 1 <= 4 &&
               std::max(C[a].depth, C[b].depth) + 1 <= 2 && scale_ok(C[a].c.scale() * C[b].c.scale(), rows(a)) && fits(combine(C[a].m, C[b].m, 2));
    }
    bool can_add(int a, int b, bool sub = false) const
    {
        return live(a) && live(b) && C[a].c.parms_id() == C[b].c.parms_id() && close(C[a].c.scale(), C[b].c.scale()) &&
               fits(combine(C[a].m, C[b].m, sub ? 1 : 0));
    }
    int need_pt(int a)  // a plaintext multiply_plain(c_a, .) accepts; half of the time a new (recorded) encode
    {
        int cand[NP], n = 0;
        for (int j = 0; j < NP; ++j)
            if (can_mulpt(a, j)) cand[n++] = j;
        if (n && R.below(2)) return cand[R.below(n)];
        const int pj = R.below(NP);
        if (R.one_in(4)) encode_scalar(pj, rows(a), S40);
        else encode_vec(pj, rows(a), S40, 0);
        return can_mulpt(a, pj) ? pj : -1;
    }
    void draw_step(int &step, int &ks)
    {
        static const int direct[] = {1, 2, 4, 8, -1, -2, 64, 1, 1}, chained[] = {3, 5, 6, 7, -3, 12, 100, -5}, second[] = {1, 2, 3, 5, -1, -2, 8, 6, 7};
        const int r = R.below(10);
        ks = r >= 8;
        step = r < 6 ? direct[R.below(9)] : (r < 8 ? chained[R.below(8)] : second[R.below(9)]);
    }
    // a submission forced while c_t is still held by its variable: add_plain reads it at once
    void force_flush(int t)
    {
        if (!live(t)) return;
        if (R.below(2)) {
            observe();
            return;
        }
        const int pj = R.below(NP);
        encode_scalar(pj, rows(t), C[t].c.scale());
        if (plive(pj) && fits(combine(C[t].m, P[pj].m, 0))) add_plain(other({t}), t, pj);
    }

    // ---- motifs (a) .. (l) of the planner
    void rot_mul(int variant /* 0 (a) temporary dropped, 1 (b) a copy kept, 2 (c) also read by an add */)
    {
        ++motif[variant];
        const int a = need_ct2(), p = need_pt(a);
        if (p < 0) return;
        int step, ks;
        draw_step(step, ks);
        const int t = other({a}), d = other({a, t});
        rot(t, a, step, ks);
        if (!live(t) || !can_mulpt(t, p)) return;
        if (R.one_in(6)) force_flush(t);
        if (variant == 1) copy(other({a, t, d}), t);
        if (variant == 2 && R.below(2) && can_add(t, a)) addsub(other({a, t, d}), t, a, false);
        if (variant == 0 && R.below(2)) {
            mulpt(t, t, p);  // in place: the variable lets go of the rotation
            return;
        }
        mulpt(d, t, p);
        if (variant == 2 && can_add(t, a)) addsub(other({a, t, d}), a, t, false);
        if (live(t)) drop(t);
    }
    // rotate-by-s + add_inplace pairs (helper.h:472-476): flavour 0 (d), 1 (e) an intermediate copied out, 2 (f) another step
    // or key in the middle, 3 (g) the accumulator produced at the depth of the first rotation, 4 (l) a sub in place of an add
    void run(int n, int flavour)
    {
        static const int ids[5] = {3, 4, 5, 6, 11};
        ++motif[ids[flavour]];
        const int src = n >= 12 ? fresh(R.below(NC), 1) : need_ct2();
        if (!live(src)) return;
        const int dup = other({src}), acc = other({src, dup});
        int step = 1, ks = 0;
        if (n < 100 && R.one_in(3)) draw_step(step, ks);  // (the long chains of --chain: rotate by 1 with its direct key)
        copy(dup, src);
        if (flavour == 3) {
            if (R.below(2)) rot(acc, src, step == 2 ? 4 : 2, 0);
            else if (can_add(src, src)) addsub(acc, src, src, false);
            else copy(acc, src);
        } else
            copy(acc, src);
        const int mid = n / 2;
        for (int s = 0; s < n; ++s) {
            int st = step, k = ks;
            if (flavour == 2 && s == mid) {
                if (R.below(2)) st = step == 1 ? 2 : 1, k = 0;
                else st = 1, k = ks ? 0 : 1;
            }
            if (!live(dup) || !live(acc) || !rotatable(dup)) break;
            const bool sub = flavour == 4 && (s == mid || R.one_in(4));
            if (!fits(combine(C[acc].m, rotated(C[dup].m, st), sub ? 1 : 0))) break;
            if (!rot(dup, dup, st, k)) break;
            if (!can_add(acc, dup, sub)) break;
            if (!sub && R.one_in(8)) {
                if (!call(fmt("c%d = add(c%d, c%d)", acc, dup, acc), [&] { ev->add(C[dup].c, C[acc].c, C[acc].c); })) break;  // the rotation first
                C[acc].m = combine(C[acc].m, C[dup].m, 0), C[acc].depth = std::max(C[acc].depth, C[dup].depth), C[acc].terms += C[dup].terms;
            } else if (!addsub(acc, acc, dup, sub))
                break;
            if (flavour == 1 && s == mid) copy(other({src, dup, acc}), R.below(2) ? dup : acc);
        }
    }
    void same_rotation_twice()  // (h)
    {
        ++motif[7];
        const int a = need_ct2(), p = need_pt(a);
        int step, ks;
        draw_step(step, ks);
        const int t1 = other({a}), t2 = other({a, t1});
        rot(t1, a, step, ks);
        if (R.one_in(8)) force_flush(t1);
        rot(t2, a, step, ks);
        const int t = R.below(2) ? t1 : t2;
        if (p >= 0 && live(t) && can_mulpt(t, p)) mulpt(t, t, p);
    }
    void add_of_two_rotations()  // (i)
    {
        ++motif[8];
        const int a = need_ct2();
        int b = pick_ct([&](int x) { return rotatable(x) && can_add(a, x); });
        if (b < 0) b = a;
        int s1, k1, s2, k2;
        draw_step(s1, k1);
        draw_step(s2, k2);
        const int t1 = other({a, b}), t2 = other({a, b, t1});
        rot(t1, a, s1, k1);
        rot(t2, b, s2, k2);
        if (can_add(t1, t2)) addsub(R.below(2) ? t1 : other({a, b, t1, t2}), t1, t2, R.one_in(4));
    }
    void add_x_x()  // (j)
    {
        ++motif[9];
        const int x = pick_ct([&](int i) { return can_add(i, i); });
        if (x >= 0) addsub(R.below(3) ? other({x}) : x, x, x, false);
    }
    void recorded_encode_product()  // (k)
    {
        ++motif[10];
        int a = need_ct2();
        const bool with_switch = R.below(2);
        if (with_switch && rows(a) >= ctx->k() - 1) {  // the plaintext is encoded one level above the ciphertext
            const int t = other({a});
            if (!unary(t, a, 2)) return;
            a = t;
        }
        const int pj = R.below(NP);
        encode_vec(pj, rows(a) + (with_switch ? 1 : 0), S40, 0);
        if (with_switch && plive(pj)) modswitch_pt(pj);
        if (can_mulpt(a, pj)) mulpt(R.below(2) ? a : other({a}), a, pj);
    }

    void single()
    {
        const int d = R.below(NC);
        switch (R.below(20)) {
            case 0: fresh(d); break;
            case 1: encode_vec(R.below(NP), 1 + R.below(ctx->k() - 1), S40, 0); break;
            case 2: encode_scalar(R.below(NP), 1 + R.below(ctx->k() - 1), S40); break;
            case 3: {
                int cand[NP], n = 0;
                for (int j = 0; j < NP; ++j)
                    if (plive(j) && close(P[j].p.scale(), S40)) cand[n++] = j;
                if (n) encrypt(d, cand[R.below(n)]);
                break;
            }
            case 4: case 5: case 6: {
                const int a = pick_ct([](int) { return true; });
                if (a < 0) break;
                const bool sub = R.one_in(3);
                const int b = pick_ct([&](int x) { return can_add(a, x, sub); });
                if (b >= 0) addsub(R.below(3) ? d : a, a, b, sub);
                break;
            }
            case 7: {  // add_plain: a reader the recorder does not record -- it forces a submission
                const int a = pick_ct([](int) { return true; });
                if (a < 0) break;
                const int pj = R.below(NP);
                if (R.below(2)) encode_scalar(pj, rows(a), C[a].c.scale());
                else encode_vec(pj, rows(a), C[a].c.scale(), 0);
                if (plive(pj) && P[pj].p.parms_id() == C[a].c.parms_id() && fits(combine(C[a].m, P[pj].m, 0))) add_plain(R.below(2) ? d : a, a, pj);
                break;
            }
            case 8: case 9: {  // multiply_plain, on size-3 inputs too
                const int a = pick_ct([&](int x) { return C[x].depth <= 1; });
                if (a < 0) break;
                const int p = need_pt(a);
                if (p >= 0) mulpt(R.below(2) ? d : a, a, p);
                break;
            }
            case 10: case 11: {
                const int a = pick_ct([&](int x) { return C[x].depth == 0 || R.one_in(3); });
                if (a < 0) break;
                const int b = R.below(3) ? pick_ct([&](int x) { return can_mul(a, x); }) : a;
                if (b >= 0 && can_mul(a, b)) mul(R.below(2) ? d : a, a, b);
                break;
            }
            case 12: {
                const int a = pick_ct([&](int x) { return C[x].c.size() > 2; });
                if (a >= 0) unary(R.below(2) ? d : a, a, 0);
                break;
            }
            case 13: {
                const int a = pick_ct([&](int x) { return rows(x) >= 2 && std::log2(C[x].c.scale()) >= 75; });
                if (a >= 0) unary(R.below(2) ? d : a, a, 1);
                break;
            }
            case 14: {
                const int a = pick_ct([&](int x) { return rows(x) >= 2 && scale_ok(C[x].c.scale(), rows(x) - 1); });
                if (a >= 0) unary(R.below(2) ? d : a, a, 2);
                break;
            }
            case 15: {
                int cand[NP], n = 0;
                for (int j = 0; j < NP; ++j)
                    if (plive(j) && P[j].p.rows >= 2) cand[n++] = j;
                if (n) modswitch_pt(cand[R.below(n)]);
                break;
            }
            case 16: {
                const int a = pick_ct([&](int x) { return rotatable(x); });
                int step, ks;
                draw_step(step, ks);
                if (a >= 0) rot(R.below(2) ? d : a, a, step, ks);
                break;
            }
            case 17: {
                const int a = pick_ct([&](int x) { return rotatable(x); });
                if (a >= 0) conj(R.below(2) ? d : a, a);
                break;
            }
            case 18: {
                const int a = pick_ct([](int) { return true; });
                if (a < 0) break;
                std::vector<int> ids{a};
                std::vector<double> m = C[a].m;
                for (int i = 0; i < NC && ids.size() < 4; ++i)
                    if (i != a && live(i) && C[i].c.parms_id() == C[a].c.parms_id() && close(C[i].c.scale(), C[a].c.scale()) &&
                        (C[i].c.size() == C[a].c.size() || R.one_in(4)) && fits(combine(m, C[i].m, 0))) {
                        ids.push_back(i);
                        m = combine(m, C[i].m, 0);
                    }
                if (R.one_in(3)) ids.push_back(a);  // one ciphertext twice
                if (ids.size() >= 2 && fits(m)) add_many(d, ids);
                break;
            }
            default: {
                const int a = pick_ct([](int) { return true; });
                if (a < 0) break;
                if (R.below(3)) copy(d, a);
                else drop(a);
                break;
            }
        }
    }

    // the calls SEAL refuses: same exception in every mode, and the recording goes on undisturbed
    void illegal()
    {
        const int a = fresh(R.below(NC)), t = other({a}), d = other({a, t});
        if (!live(a)) return;
        const int pj = R.below(NP);
        switch (R.below(8)) {
            case 0:  // level mismatch
                if (unary(t, a, 2)) addsub(d, a, t, false);
                break;
            case 1:  // scale mismatch
                encode_scalar(pj, rows(a), S40);
                if (plive(pj) && mulpt(t, a, pj)) addsub(d, a, t, false);
                break;
            case 2: rot(d, a, R.below(2) ? SLOTS : -SLOTS - 3, 0); break;        // step count too large
            case 3: rot(d, a, R.below(2) ? 4 : 16, 1); break;                      // Galois key not present
            case 4:                                                                // zero plaintext: transparent result
                if (encode_vec(pj, rows(a), S40, 2)) mulpt(R.below(2) ? d : a, a, pj);
                break;
            case 5:  // scale out of bounds
                if (R.below(2)) encode_vec(pj, rows(a), std::pow(2.0, 150), 0);
                else if (unary(t, a, 2) && unary(t, t, 2) && encode_vec(pj, 1, S40, 0)) mulpt(d, t, pj);
                break;
            case 6:  // rotate on a size-3 ciphertext
                if (mul(t, a, a)) rot(d, t, 1, 0);
                break;
            default:  // rescale at the last level
                if (unary(t, a, 2) && unary(t, t, 2)) unary(R.below(2) ? t : d, t, 1);
                break;
        }
    }

    void program(int steps, int chain)
    {
        for (int i = 0; i < 3; ++i) fresh(i);
        if (chain > 0) {
            long_chain = true;
            run(chain, 0);
            observe();
        }
        for (int s = 0; s < steps; ++s) {
            const int r = R.below(100);
            if (r < 50) {
                static const int runs[4] = {1, 2, 3, 12}, longer[3] = {3, 3, 12};
                switch (R.below(12)) {
                    case 0: rot_mul(0); break;
                    case 1: rot_mul(1); break;
                    case 2: rot_mul(2); break;
                    case 3: run(runs[R.below(4)], 0); break;
                    case 4: run(longer[R.below(3)], 1); break;
                    case 5: run(longer[R.below(3)], 2); break;
                    case 6: run(longer[R.below(3)], 3); break;
                    case 7: same_rotation_twice(); break;
                    case 8: add_of_two_rotations(); break;
                    case 9: add_x_x(); break;
                    case 10: recorded_encode_product(); break;
                    default: run(runs[R.below(4)], 4); break;
                }
            } else
                single();
            if (R.one_in(8)) illegal();
            if (R.one_in(10)) observe();
        }
    }

    // the final variables against the slot model: catches a wrong operand, does not measure precision
    int decode_check()
    {
        int bad = 0;
        for (int i = 0; i < NC; ++i) {
            if (!live(i) || C[i].m.size() != (std::size_t)SLOTS) continue;
            Plaintext p;
            std::vector<double> v;
            decryptor->decrypt(C[i].c, p);
            enc->decode(p, v);
            double err = 0;
            for (int s = 0; s < SLOTS; ++s) err = std::max(err, std::fabs(v[(std::size_t)s] - C[i].m[(std::size_t)s]));
            const double thr = C[i].terms > 2 ? 1e-3 : 1e-5;  // single products / sums of many
            std::printf("model c%d terms=%d depth=%d maxabs=%.3f err=%.3e thr=%.0e %s\n", i, C[i].terms, C[i].depth, maxabs(C[i].m), err, thr,
                        err <= thr ? "ok" : "FAIL");
            bad += !(err <= thr);
        }
        return bad;
    }
};

}  // namespace

int main(int argc, char **argv)
{
    std::uint64_t seed = 1;
    long ops = -1;
    int steps = 24, lazy = -1, ndev = 0, chain = 0;
    long pend_mb = 0;
    bool dump = false, decode = false, draw = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> const char * {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "%s needs a value\n", a.c_str());
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "--seed") seed = std::strtoull(val(), nullptr, 0);
        else if (a == "--ops") ops = std::atol(val());
        else if (a == "--steps") steps = std::atoi(val());
        else if (a == "--lazy") lazy = std::atoi(val());
        else if (a == "--pend-mb") pend_mb = std::atol(val());
        else if (a == "--ndev") ndev = std::atoi(val());
        else if (a == "--chain") chain = std::atoi(val());
        else if (a == "--dump") dump = true;
        else if (a == "--decode") decode = true;
        else if (a == "--draw-settings") draw = true;
        else {
            std::fprintf(stderr, "usage: shim_fuzz --seed S [--ops K] [--steps T] [--lazy 0|1] [--pend-mb M] [--ndev D] [--draw-settings] [--chain N] [--dump] [--decode]\n");
            return 2;
        }
    }
    if (draw) {  // per-run settings from the seed (a stream of their own: the program stays the seed's)
        Rng s{seed ^ 0x5E771465ull};
        lazy = s.below(4) ? 1 : 0;
        pend_mb = s.below(2) ? 0 : 1 + s.below(8);
        ndev = 1 + s.below(3);
    }
    setenv("SEAL_SHIM_SEED", "20240229", 0);  // the key generator and the encryptor draw the same keys in every run
    Fuzz fz;
    int rc = 0;
    try {
        EncryptionParameters params(scheme_type::CKKS);
        params.set_poly_modulus_degree(8192);
        params.set_coeff_modulus(CoeffModulus::Create(8192, {60, 40, 40, 60}));
        fz.ctx = SEALContext::Create(params);
        auto &e = fz.ctx->engine();
        if (lazy >= 0) e->lazy = lazy != 0;
        if (pend_mb > 0) e->pend_budget = e->pend_check = (std::size_t)pend_mb << 20;
        if (ndev > 0) e->ndev = ndev;
        std::printf("settings seed=%" PRIu64 " lazy=%d pend_mb=%ld ndev=%d steps=%d chain=%d ops=%ld\n", seed, (int)e->lazy, pend_mb, e->ndev, steps, chain, ops);
        KeyGenerator keygen(fz.ctx);
        PublicKey pk = keygen.public_key();
        SecretKey sk = keygen.secret_key();
        fz.rk = keygen.relin_keys(2);
        fz.gk[0] = keygen.galois_keys();
        fz.gk[1] = keygen.galois_keys(std::vector<int>{1, 2, 3, 5, -1, -2, 8});
        Encryptor encryptor(fz.ctx, pk);
        Evaluator evaluator(fz.ctx);
        Decryptor decryptor(fz.ctx, sk);
        CKKSEncoder encoder(fz.ctx);
        fz.ev = &evaluator, fz.enc = &encoder, fz.encryptor = &encryptor, fz.decryptor = &decryptor;
        fz.R.s = seed * 0x2545F4914F6CDD1Dull + 0x1234567ull;
        fz.max_ops = ops;
        fz.dump = dump;
        try {
            fz.program(steps, chain);
        } catch (const Stop &) {
        }
        fz.max_ops = -1;
        fz.observe();
        std::printf("motifs");
        for (int i = 0; i < 12; ++i) std::printf(" %c=%ld", 'a' + i, fz.motif[i]);
        std::printf("\nend calls=%ld throws=%ld observations=%ld\n", fz.ncalls, fz.nthrows, fz.nobs);
        if (decode && fz.decode_check()) rc = 4;
        if (fz.engine_error) rc = 5;
        for (auto &c : fz.C) c = CtVar();  // payloads go before the evaluator objects do
        for (auto &p : fz.P) p = PtVar();
    } catch (const std::exception &ex) {
        std::printf("FATAL %s\n", ex.what());
        return 5;
    }
    return rc;
}
