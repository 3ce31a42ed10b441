// hefx_poly_plan.h -- the planner of polynomial evaluation on ciphertexts as host-only code: the weight rounding rule, the
// depth-optimal Paterson-Stockmeyer plan in the power and the Chebyshev basis, its scale bookkeeping.  No HIP in here:
// drivers/poly_plan_selftest.cpp compiles it with g++ under the sanitizers; tests/test_poly_plan_cpu.py executes its step
// list over exact rationals; hefx_capi.cpp hands it out as hefx_poly_plan (include/hefx_poly.h, where the steps are
// specified); include/seal/shim_poly.h includes it directly.
//
// SHAPE OF A PLAN.  With k baby steps (k a power of two) the powers are P_1 .. P_(k-1) and the giant steps P_k, P_2k, P_4k ..
// (P_n = x^n or T_n), each made on demand at depth ceil(log2 n) from P_ceil(n/2) and P_floor(n/2): one MUL and one COMBINE
// (power basis: the COMBINE is the bare rescale, weight 1; Chebyshev: T_2i = 2 T_i^2 - 1 and T_(i+j) = 2 T_i T_j - T_(i-j)
// with i - j = 1, weights 2 and -round(s_i s_j / s_1) -- coefficient -1 at the weight scale s_i s_j / s_1 -- and the constant
// -1 at s_i s_j).
// A polynomial p that must arrive at (level, S) is peeled from the top:  p = Q_j P_(k 2^j) + ... + Q_0 P_k + leaf, every Q_i
// of degree below k 2^i and the leaf below k.  ALL of it goes into ONE COMBINE at level + 1 rows and scale S q_level: a
// product Q_i P_g (MUL, its quotient evaluated one level up at S q_level / scale(P_g)) enters with weight 1, a quotient that
// is only a constant c enters as the weight c on P_g, the leaf as weights on the baby steps, the constant term as the
// constant.  One rescale then lands on (level, S).  A node's remainder therefore never exists as a ciphertext of its own and
// the planner emits no ADD (the op stays in the step list for executors and for planners to come).
// DEPTH.  k = 2 always fits ceil(log2(d + 1)) levels; a larger k fits when the degree leaves room (a leaf's COMBINE costs a
// level on top of its highest baby step).  Every k = 2, 4, .. up to the first power of two above d is planned top-down from
// the mandated result level; a k that would need a power below the level it has is dropped; the fewest MULs win, the smaller
// k on a tie.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

namespace hefx_poly {

enum Op { MUL = 0, COMBINE = 1, ADD = 2 };
enum Basis { POWER = 0, CHEBYSHEV = 1 };
constexpr int COMBINE_MAX_IN = 256;  // HEFX_COMBINE_MAX_IN

struct Term {
    int src;
    double coef, wscale;
};
struct Step {
    int op, dst, a, b, level, has_const;
    double constant, cscale, scale;
};
struct Plan {
    std::vector<Step> steps;
    std::vector<Term> terms;
    int nslots = 1, muls = 0, depth = 0, baby = 0;
};

// round_half_away(value * scale) mod q, canonical: the word hefx_ckks_encode_scalar writes (hefx_encode.hip: wide_residue).
// Below 2^63 the rounded magnitude is a 64-bit integer; from there up a float64 has no fraction bits and is m * 2^e with
// m < 2^53, reduced as (m mod q) * (2^e mod q).
inline uint64_t weight_residue(double value, double scale, uint64_t q)
{
    typedef unsigned __int128 u128;
    const double co = std::round(value * scale);
    if (!std::isfinite(co) || q == 0) return 0;
    const double a = std::fabs(co);
    uint64_t r;
    if (a < 0x1p63) {
        r = (uint64_t)a % q;
    } else {
        uint64_t bits;
        std::memcpy(&bits, &a, sizeof bits);
        int e = (int)(bits >> 52) - 1075;  // a = m * 2^e, e >= 11
        const uint64_t m = (bits & ((1ull << 52) - 1)) | (1ull << 52);
        uint64_t p2 = 1 % q, b = 2 % q;
        for (; e; e >>= 1) {
            if (e & 1) p2 = (uint64_t)((u128)p2 * b % q);
            b = (uint64_t)((u128)b * b % q);
        }
        r = (uint64_t)((u128)(m % q) * p2 % q);
    }
    return co < 0.0 && r ? q - r : r;
}

inline int ceil_log2(int n)  // n >= 1
{
    int b = 0;
    while ((1 << b) < n) ++b;
    return b;
}

struct Builder {
    int basis, L0, k;
    const uint64_t *q;
    Plan P;
    struct Slot {
        int level;
        double scale;
    };
    std::vector<Slot> slots;
    std::map<int, int> power;  // n -> slot of P_n
    bool ok = true;

    Builder(int basis_, int L0_, const uint64_t *q_, double in_scale, int k_) : basis(basis_), L0(L0_), k(k_), q(q_)
    {
        slots.push_back(Slot{L0, in_scale});
        power[1] = 0;
        P.baby = k;
    }
    int new_slot(int level, double scale)
    {
        slots.push_back(Slot{level, scale});
        return (int)slots.size() - 1;
    }
    int mul(int a, int b)
    {
        const int level = slots[(size_t)a].level < slots[(size_t)b].level ? slots[(size_t)a].level : slots[(size_t)b].level;
        const int t = new_slot(level, slots[(size_t)a].scale * slots[(size_t)b].scale);
        P.steps.push_back(Step{MUL, t, a, b, level, 0, 0.0, 0.0, slots[(size_t)t].scale});
        ++P.muls;
        return t;
    }
    // hefx_scalar_combine at L rows and scale S, then the rescale: the result has L - 1 rows and S / q_(L-1)
    int combine(int L, double S, const std::vector<Term> &tms, bool has_const, double constant)
    {
        if (L < 2 || L > L0 || tms.empty() || (int)tms.size() > COMBINE_MAX_IN) {
            ok = false;
            return -1;
        }
        const int dst = new_slot(L - 1, S / (double)q[L - 1]);
        P.steps.push_back(Step{COMBINE, dst, (int)P.terms.size(), (int)tms.size(), L, has_const ? 1 : 0, has_const ? constant : 0.0,
                               S, slots[(size_t)dst].scale});
        P.terms.insert(P.terms.end(), tms.begin(), tms.end());
        return dst;
    }
    int get_power(int n)
    {
        auto it = power.find(n);
        if (it != power.end()) return it->second;
        const int a = (n + 1) / 2, b = n / 2;  // (a giant step k 2^j is the square of the one before it: a == b)
        const int sa = get_power(a), sb = ok ? get_power(b) : -1;
        if (!ok) return -1;
        const int t = mul(sa, sb);
        const int L = slots[(size_t)t].level;
        const double S = slots[(size_t)t].scale;
        std::vector<Term> tms;
        bool has_const = false;
        if (basis == POWER) {
            tms.push_back(Term{t, 1.0, 1.0});
        } else {
            tms.push_back(Term{t, 2.0, 1.0});
            if (a == b)
                has_const = true;  // T_2a = 2 T_a^2 - 1
            else  // T_(a+b) = 2 T_a T_b - T_1 (a - b == 1); slot 0 is read through its row prefix.  The weight is
                  // round(-1 * wscale) = -round(s_a s_b / s_1), an integer either way: wscale stays the exact ratio
                tms.push_back(Term{0, -1.0, S / slots[0].scale});
        }
        const int dst = combine(L, S, tms, has_const, -1.0);
        if (ok) power[n] = dst;
        return dst;
    }
    static int top(const std::vector<double> &c)
    {
        int d = (int)c.size() - 1;
        while (d >= 0 && c[(size_t)d] == 0.0) --d;
        return d;
    }
    // c (degree >= 1 after trimming) -> a slot at (level, S)
    int eval(std::vector<double> c, int level, double S)
    {
        const int L = level + 1;
        if (level < 1 || L > L0) {
            ok = false;
            return -1;
        }
        const double Sc = S * (double)q[level];
        std::vector<Term> tms;
        int deg = top(c);
        while (ok && deg >= k) {
            int g = k;
            while (2 * g <= deg) g *= 2;  // the largest giant step <= deg, so deg < 2g
            std::vector<double> Q((size_t)(deg - g + 1));
            if (basis == POWER) {
                for (int i = g; i <= deg; ++i) Q[(size_t)(i - g)] = c[(size_t)i];
            } else {  // p = Q T_g + r:  T_i T_g = (T_(i+g) + T_(g-i)) / 2
                Q[0] = c[(size_t)g];
                for (int i = g + 1; i <= deg; ++i) {
                    Q[(size_t)(i - g)] = 2.0 * c[(size_t)i];
                    c[(size_t)(2 * g - i)] -= c[(size_t)i];
                }
            }
            c.resize((size_t)g);
            const int sg = get_power(g);
            if (!ok || slots[(size_t)sg].level < L) {
                ok = false;
                return -1;
            }
            const int qdeg = top(Q);
            if (qdeg == 0) {  // only a constant: a weight on the giant step, no product
                tms.push_back(Term{sg, Q[0], Sc / slots[(size_t)sg].scale});
            } else if (qdeg > 0) {
                const int sq = eval(Q, level + 1, Sc / slots[(size_t)sg].scale);
                if (!ok) return -1;
                const int t = mul(sq, sg);
                tms.push_back(Term{t, 1.0, Sc / slots[(size_t)t].scale});
            }
            deg = top(c);
        }
        for (int i = 1; ok && i <= deg; ++i) {
            if (c[(size_t)i] == 0.0) continue;
            const int sb = get_power(i);
            if (!ok || slots[(size_t)sb].level < L) {
                ok = false;
                return -1;
            }
            tms.push_back(Term{sb, c[(size_t)i], Sc / slots[(size_t)sb].scale});
        }
        if (!ok) return -1;
        const bool has_const = deg >= 0 && c[0] != 0.0;
        return combine(L, Sc, tms, has_const, has_const ? c[0] : 0.0);
    }
};

// nullptr on success, else why not.  target_scale <= 0: in_scale.
inline const char *plan(int degree, const double *coeffs, int basis, int nprimes, const uint64_t *primes, double in_scale,
                        double target_scale, Plan &out)
{
    if (degree < 0 || !coeffs || !primes || nprimes < 1) return "bad polynomial plan arguments";
    if (basis != POWER && basis != CHEBYSHEV) return "unknown basis";
    if (!(in_scale > 0) || !std::isfinite(in_scale)) return "scale out of bounds";
    for (int i = 0; i <= degree; ++i)
        if (!std::isfinite(coeffs[i])) return "coefficients must be finite";
    std::vector<double> c(coeffs, coeffs + degree + 1);
    const int d = Builder::top(c);
    if (d < 1) return "a constant polynomial has no ciphertext term";
    if (d > 1023) return "degree out of range";
    c.resize((size_t)d + 1);
    const int depth = ceil_log2(d + 1);
    if (nprimes - depth < 1) return "not enough levels for this degree";
    if (!(target_scale > 0)) target_scale = in_scale;
    bool found = false;
    for (int k = 2;; k *= 2) {
        Builder B(basis, nprimes, primes, in_scale, k);
        B.eval(c, nprimes - depth, target_scale);
        if (B.ok && (!found || B.P.muls < out.muls)) {
            out = B.P;
            out.nslots = (int)B.slots.size();
            out.depth = depth;
            found = true;
        }
        if (k > d) break;
    }
    return found ? nullptr : "no plan of minimal depth";
}

}  // namespace hefx_poly
