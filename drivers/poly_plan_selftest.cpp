// poly_plan_selftest.cpp -- csrc/hefx_poly_plan.h (the polynomial planner and the weight rounding rule) alone, as a
// stand-alone host program: g++ -std=c++17 -fsanitize=address,undefined, no HIP, no library.
//   no arguments   the planner's invariants over degrees 1 .. 63 in both bases and several coefficient patterns (depth, slot
//                  discipline, levels, scale bookkeeping, the plan's value at a point), the refusals, the residue rule against
//                  128-bit integer arithmetic; ends with "POLY PLAN SELFTEST PASSED"
//   basis degree in_scale target_scale nprimes p_0 .. p_(nprimes-1) c_0 .. c_degree
//                  (basis: power | chebyshev; floats in any strtod form, hex floats included; target_scale 0: in_scale)
//                  prints the plan in the format of seal_fyp_logistic_regression_amd/poly.py format_plan, which
//                  tests/test_poly_plan_cpu.py compares with the plan read through the library, line for line
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../seal_fyp_logistic_regression_amd/csrc/hefx_poly_plan.h"

using namespace hefx_poly;

static int g_fail = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            ++g_fail;                      \
            printf("FAIL %s: ", #cond);    \
            printf(__VA_ARGS__);           \
            printf("\n");                  \
        }                                  \
    } while (0)

static void print_plan(const Plan &P)
{
    printf("slots %d steps %zu\n", P.nslots, P.steps.size());
    for (const Step &s : P.steps) {
        if (s.op == MUL) {
            printf("MUL %d = %d * %d level %d scale %.17g\n", s.dst, s.a, s.b, s.level, s.scale);
        } else if (s.op == ADD) {
            printf("ADD %d = %d + %d level %d scale %.17g\n", s.dst, s.a, s.b, s.level, s.scale);
        } else {
            printf("COMBINE %d level %d S %.17g scale %.17g ", s.dst, s.level, s.cscale, s.scale);
            if (s.has_const)
                printf("const %.17g terms", s.constant);
            else
                printf("const none terms");
            for (int i = 0; i < s.b; ++i) {
                const Term &t = P.terms[(size_t)(s.a + i)];
                printf(" (%d %.17g %.17g)", t.src, t.coef, t.wscale);
            }
            printf("\n");
        }
    }
}

static bool close_rel(double a, double b, double tol) { return std::fabs(a - b) <= tol * std::fmax(std::fabs(a), std::fabs(b)); }

static double reference_value(int basis, const std::vector<double> &c, double x)
{
    double t0 = 1.0, t1 = x, acc = c[0];
    for (size_t i = 1; i < c.size(); ++i) {
        acc += c[i] * t1;
        const double t2 = basis == POWER ? t1 * x : 2.0 * x * t1 - t0;
        t0 = t1, t1 = t2;
    }
    return acc;
}

// the invariants of one plan; returns its MUL count
static int check_plan(const char *what, int basis, const std::vector<double> &c, const std::vector<uint64_t> &q, double s0, double target)
{
    Plan P;
    const int d = (int)c.size() - 1;
    const char *err = plan(d, c.data(), basis, (int)q.size(), q.data(), s0, target, P);
    CHECK(err == nullptr, "%s d=%d: %s", what, d, err ? err : "");
    if (err) return 0;
    const int L0 = (int)q.size(), depth = ceil_log2(Builder::top(c) + 1);
    std::vector<int> level((size_t)P.nslots, -1);
    std::vector<double> scale((size_t)P.nslots, 0.0), value((size_t)P.nslots, 0.0);
    const double x = 0.3125;
    level[0] = L0, scale[0] = s0, value[0] = x;
    int muls = 0;
    for (const Step &s : P.steps) {
        CHECK(s.dst > 0 && s.dst < P.nslots && level[(size_t)s.dst] < 0, "%s d=%d: slot %d written twice or out of range", what, d, s.dst);
        if (s.dst <= 0 || s.dst >= P.nslots) return 0;
        if (s.op == MUL || s.op == ADD) {
            CHECK(s.a >= 0 && s.b >= 0 && s.a < P.nslots && s.b < P.nslots && level[(size_t)s.a] > 0 && level[(size_t)s.b] > 0, "%s d=%d: operand not ready", what, d);
            if (!(s.a >= 0 && s.b >= 0 && s.a < P.nslots && s.b < P.nslots)) return 0;
            const int la = level[(size_t)s.a], lb = level[(size_t)s.b];
            if (s.op == MUL) {
                ++muls;
                CHECK(s.level == (la < lb ? la : lb), "%s d=%d: MUL level", what, d);
                CHECK(s.scale == scale[(size_t)s.a] * scale[(size_t)s.b], "%s d=%d: MUL scale", what, d);
                value[(size_t)s.dst] = value[(size_t)s.a] * value[(size_t)s.b];
            } else {
                CHECK(la == lb && s.level == la, "%s d=%d: ADD levels", what, d);
                CHECK(close_rel(scale[(size_t)s.a], scale[(size_t)s.b], 1e-12), "%s d=%d: ADD scales", what, d);
                value[(size_t)s.dst] = value[(size_t)s.a] + value[(size_t)s.b];
            }
            level[(size_t)s.dst] = s.level, scale[(size_t)s.dst] = s.scale;
        } else {
            CHECK(s.op == COMBINE && s.b >= 1 && s.b <= COMBINE_MAX_IN && s.a >= 0 && (size_t)(s.a + s.b) <= P.terms.size(), "%s d=%d: COMBINE terms", what, d);
            CHECK(s.level >= 2 && s.level <= L0, "%s d=%d: COMBINE level %d", what, d, s.level);
            if (!(s.b >= 1 && s.a >= 0 && (size_t)(s.a + s.b) <= P.terms.size() && s.level >= 2 && s.level <= L0)) return 0;
            double v = s.has_const ? s.constant : 0.0;
            for (int i = 0; i < s.b; ++i) {
                const Term &t = P.terms[(size_t)(s.a + i)];
                CHECK(t.src >= 0 && t.src < P.nslots && level[(size_t)t.src] >= s.level, "%s d=%d: term source above its level", what, d);
                if (!(t.src >= 0 && t.src < P.nslots)) return 0;
                CHECK(close_rel(scale[(size_t)t.src] * t.wscale, s.cscale, 1e-12), "%s d=%d: scale(src) * wscale != S", what, d);
                CHECK(std::round(t.coef * t.wscale) != 0.0, "%s d=%d: a weight of zero (transparent term)", what, d);
                v += t.coef * value[(size_t)t.src];
            }
            CHECK(s.scale == s.cscale / (double)q[(size_t)s.level - 1], "%s d=%d: COMBINE scale", what, d);
            level[(size_t)s.dst] = s.level - 1, scale[(size_t)s.dst] = s.scale, value[(size_t)s.dst] = v;
        }
    }
    const int res = P.steps.back().dst;
    CHECK(level[(size_t)res] == L0 - depth, "%s d=%d: depth %d, wanted %d", what, d, L0 - level[(size_t)res], depth);
    CHECK(close_rel(scale[(size_t)res], target > 0 ? target : s0, 1e-12), "%s d=%d: result scale", what, d);
    const double want = reference_value(basis, c, x);
    CHECK(std::fabs(value[(size_t)res] - want) <= 1e-9 * (1.0 + std::fabs(want)), "%s d=%d: value %.17g, wanted %.17g", what, d, value[(size_t)res], want);
    CHECK(muls == P.muls, "%s d=%d: MUL count", what, d);
    return muls;
}

static uint64_t residue_int(bool neg, unsigned __int128 mag, uint64_t q)
{
    const uint64_t r = (uint64_t)(mag % q);
    return neg && r ? q - r : r;
}

static void check_residues()
{
    const uint64_t qs[] = {0x1fffffffffe00001ull, 0xffffffffffc0001ull, 1099511590913ull, 12289ull, 97ull};
    for (uint64_t q : qs) {
        CHECK(weight_residue(0.5, 1.0, q) == 1 % q, "tie 0.5");
        CHECK(weight_residue(-0.5, 1.0, q) == residue_int(true, 1, q), "tie -0.5");
        CHECK(weight_residue(2.5, 1.0, q) == 3 % q, "tie 2.5");
        CHECK(weight_residue(0.49999999999999994, 1.0, q) == 0, "just below a half");
        CHECK(weight_residue(1.0, 0x1p62, q) == residue_int(false, (unsigned __int128)1 << 62, q), "2^62");
        CHECK(weight_residue(-1.0, 0x1p63, q) == residue_int(true, (unsigned __int128)1 << 63, q), "-2^63");
        CHECK(weight_residue(1.0, 0x1p63 - 1024.0, q) == residue_int(false, ((unsigned __int128)1 << 63) - 1024, q), "just below 2^63");
        CHECK(weight_residue(3.0, 0x1p80, q) == residue_int(false, (unsigned __int128)3 << 80, q), "3 * 2^80");
        CHECK(weight_residue(-1.20069, 0x1p80, q) == residue_int(true, (unsigned __int128)std::round(1.20069 * 0x1p80), q), "-1.20069 * 2^80");
        CHECK(weight_residue(0.0, 0x1p40, q) == 0, "zero");
    }
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        if (argc < 6) return fprintf(stderr, "usage: %s basis degree in_scale target_scale nprimes primes.. coeffs..\n", argv[0]), 2;
        const int basis = !strcmp(argv[1], "chebyshev") ? CHEBYSHEV : POWER, d = atoi(argv[2]), np = atoi(argv[5]);
        const double s0 = strtod(argv[3], nullptr), target = strtod(argv[4], nullptr);
        if (d < 0 || np < 1 || argc != 6 + np + d + 1) return fprintf(stderr, "argument count\n"), 2;
        std::vector<uint64_t> q;
        std::vector<double> c;
        for (int i = 0; i < np; ++i) q.push_back(strtoull(argv[6 + i], nullptr, 0));
        for (int i = 0; i <= d; ++i) c.push_back(strtod(argv[6 + np + i], nullptr));
        Plan P;
        if (const char *err = plan(d, c.data(), basis, np, q.data(), s0, target, P)) return printf("REFUSED %s\n", err), 0;
        print_plan(P);
        return 0;
    }
    // 40-bit primes under a 60-bit one, as the engine's parameter sets are laid out (values only: nothing is reduced here)
    std::vector<uint64_t> q = {0xffffffffffc0001ull};
    for (int i = 0; i < 7; ++i) q.push_back(1099511590913ull - 2 * 16384ull * (uint64_t)i);
    const double s0 = 0x1p40;
    for (int basis = POWER; basis <= CHEBYSHEV; ++basis) {
        for (int d = 1; d <= 63; ++d) {
            std::vector<double> dense, odd, ends, nocst;
            for (int i = 0; i <= d; ++i) {
                const double v = (double)((i * 7 + 3) % 11 - 5) / 8.0;
                dense.push_back(v == 0.0 ? 0.375 : v);
                odd.push_back(i % 2 ? dense.back() : 0.0);
                ends.push_back(i == 0 ? 0.5 : i == d ? -1.25 : 0.0);
                nocst.push_back(i == 0 ? 0.0 : dense.back());
            }
            const int m_dense = check_plan("dense", basis, dense, q, s0, 0.0);
            if (d % 2) check_plan("odd", basis, odd, q, s0, 0.0);
            check_plan("ends", basis, ends, q, s0, 0.0);
            check_plan("no constant", basis, nocst, q, s0, 0x1p38);
            if (d == 7 || d == 15 || d == 31 || d == 63) printf("%s degree %d: %d MULs\n", basis == POWER ? "power" : "chebyshev", d, m_dense);
        }
    }
    {   // refusals
        Plan P;
        const double c3[] = {0.5, 1.0, 0.0, -1.0}, c0[] = {0.5, 0.0, 0.0};
        CHECK(plan(3, c3, POWER, 2, q.data(), s0, 0.0, P) != nullptr, "degree 3 needs two levels under the input");
        CHECK(plan(3, c3, POWER, 3, q.data(), s0, 0.0, P) == nullptr, "degree 3 fits three rows");
        CHECK(plan(2, c0, POWER, 5, q.data(), s0, 0.0, P) != nullptr, "a constant polynomial is refused");
        CHECK(plan(3, c3, 2, 5, q.data(), s0, 0.0, P) != nullptr, "unknown basis");
        CHECK(plan(3, c3, POWER, 5, q.data(), 0.0, 0.0, P) != nullptr, "scale 0");
    }
    check_residues();
    if (g_fail) return printf("%d FAILURES\n", g_fail), 1;
    printf("POLY PLAN SELFTEST PASSED\n");
    return 0;
}
