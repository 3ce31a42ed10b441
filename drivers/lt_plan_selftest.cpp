// lt_plan_selftest.cpp -- csrc/hefx_lt_plan.h (the rotation planner of the linear transforms) held to its invariants:
// every plan's elements have a key and compose to the step's Galois element, the refusals carry SEAL's texts, the flat plan
// store equals the plans one by one, the node forest is a de-duplicated prefix tree of the plans in both modes, and the lane
// dealing keeps subtrees whole, balances the loads and reports the widest batch a brute-force count finds.
// Host only: no HIP, no device, no libhefx.  tests/test_lt_plan_cpu.py builds it with g++ -fsanitize=address,undefined, runs
// it, and compares the PLAN / NODE lines it prints with the Python planner (seal.py, algorithms.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../seal_fyp_logistic_regression_amd/csrc/hefx_lt_plan.h"

using namespace hefx_lt;

namespace {

int failures = 0;
#define CHECK(cond, ...)                               \
    do {                                               \
        if (!(cond)) {                                 \
            ++failures;                                \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                       \
            printf("\n");                              \
        }                                              \
    } while (0)

const uint64_t some_key = 1;  // every key of a set points here: the planner only asks whether a key is there

enum KeySet { DEFAULT, DIRECT, NO_PLUS_4 };
const char *name_of(KeySet k) { return k == DEFAULT ? "default" : k == DIRECT ? "direct" : "no+4"; }

// SEAL's default keys: steps +-2^i for 2^i <= N/4, plus the conjugation; DIRECT: a key for every step of `steps`
LtKeys make_keys(KeySet which, size_t n, const std::vector<int> &steps)
{
    std::set<uint32_t> elts;
    if (which == DIRECT) {
        for (int s : steps) elts.insert(lt_elt_from_step(s, n));
    } else {
        elts.insert((uint32_t)(2 * n - 1));
        for (int p = 1; (size_t)p <= n / 4; p *= 2) elts.insert(lt_elt_from_step(p, n)), elts.insert(lt_elt_from_step(-p, n));
        if (which == NO_PLUS_4) elts.erase(lt_elt_from_step(4, n));
    }
    std::vector<uint32_t> e(elts.begin(), elts.end());
    std::vector<const uint64_t *> k(e.size(), &some_key);
    LtKeys K;
    K.set((int)e.size(), e.data(), k.data());
    return K;
}

bool contains(const std::vector<uint32_t> &v, uint32_t e)
{
    for (uint32_t x : v)
        if (x == e) return true;
    return false;
}

void check_plans(size_t n, const std::vector<int> &steps, bool print)
{
    const LtKeys dflt = make_keys(DEFAULT, n, steps);
    for (KeySet which : {DEFAULT, DIRECT, NO_PLUS_4}) {
        const LtKeys K = make_keys(which, n, steps);
        for (int step : steps) {
            std::vector<uint32_t> plan, with_default;
            const char *err = lt_plan(step, n, K, plan);
            CHECK(lt_plan(step, n, dflt, with_default) == nullptr, "N=%zu step %d: the default keys serve every step", n, step);
            if (print && which != DIRECT) {
                printf("PLAN %zu %s %d %s", n, name_of(which), step, err ? "!" : ":");
                if (err) printf(" %s", err);
                for (size_t i = 0; !err && i < plan.size(); ++i) printf(" %u", plan[i]);
                printf("\n");
            }
            // a step is refused exactly when its plan needs the removed key, and then with SEAL's text
            const bool needs_removed = which == NO_PLUS_4 && contains(with_default, lt_elt_from_step(4, n));
            CHECK((err != nullptr) == needs_removed, "N=%zu %s step %d: refused = %d, needs the removed key = %d", n, name_of(which), step,
                  err != nullptr, needs_removed);
            if (err) {
                CHECK(!strcmp(err, "Galois key not present"), "N=%zu %s step %d: refused with '%s'", n, name_of(which), step, err);
                continue;
            }
            CHECK(!plan.empty() && (which != DIRECT || plan.size() == 1), "N=%zu %s step %d: %zu elements", n, name_of(which), step, plan.size());
            uint64_t product = 1;  // rotations compose: the elements multiply to the step's element (3^(N/2) = 1 mod 2N)
            for (uint32_t e : plan) {
                CHECK(K.has(e), "N=%zu %s step %d: element %u has no key", n, name_of(which), step, e);
                product = product * e % (2 * n);
            }
            CHECK(product == lt_elt_from_step(step, n), "N=%zu %s step %d: the plan composes to %llu, not to %u", n, name_of(which), step,
                  (unsigned long long)product, lt_elt_from_step(step, n));
        }
        for (int big : {(int)(n / 2), -(int)(n / 2), (int)(n / 2) + 3}) {
            std::vector<uint32_t> plan;
            const char *err = lt_plan(big, n, K, plan);
            CHECK(err && !strcmp(err, "step count too large") && plan.empty(), "N=%zu %s step %d is not refused as too large", n, name_of(which), big);
        }
    }
}

// the flat store against the plans one by one, and the refusals of lt_plans itself
void check_store(size_t n, int d)
{
    std::vector<int> direct_steps{-d};
    for (int l = 1; l < d; ++l) direct_steps.push_back(l);
    for (KeySet which : {DEFAULT, DIRECT}) {
        const LtKeys K = make_keys(which, n, direct_steps);
        LtPlans P;
        const char *err = lt_plans(n, K, d, d, nullptr, nullptr, P);
        CHECK(!err && P.off.size() == (size_t)d + 1 && P.off[0] == 0 && P.off.back() == P.elts.size(), "N=%zu d=%d %s: the store is not whole", n, d, name_of(which));
        if (err) continue;
        bool chains = false;  // some term 1 .. d-1 needs more than one key switch
        for (int i = 0; i < d; ++i) {
            std::vector<uint32_t> plan;
            lt_plan(i == 0 ? -d : i, n, K, plan);
            chains = chains || (i > 0 && plan.size() > 1);
            CHECK(plan == std::vector<uint32_t>(P.plan(i), P.plan(i) + P.size(i)), "N=%zu d=%d %s: plan %d of the store differs", n, d, name_of(which), i);
        }
        err = lt_plans(n, K, d, d, nullptr, "direct keys only", P);
        CHECK(chains ? err && !strcmp(err, "direct keys only") : err == nullptr, "N=%zu d=%d %s: direct_only gave '%s'", n, d, name_of(which), err ? err : "");
        CHECK(which != DIRECT || !chains, "N=%zu d=%d: a chain under direct keys", n, d);
        const int steps[] = {0, 0};
        err = lt_plans(n, K, d, 2, steps, nullptr, P);
        CHECK(err && !strcmp(err, "only term 0 may be unrotated"), "N=%zu d=%d %s: an unrotated term 1 gave '%s'", n, d, name_of(which), err ? err : "");
    }
    LtPlans P;
    const char *err = lt_plans(n, make_keys(NO_PLUS_4, n, {}), d, d, nullptr, nullptr, P);
    CHECK(d <= 3 ? err == nullptr : err && !strcmp(err, "Galois key not present"), "N=%zu d=%d no+4: lt_plans gave '%s'", n, d, err ? err : "");
    err = lt_plans(n, make_keys(DEFAULT, n, {}), (int)(n / 2), 1, nullptr, nullptr, P);
    CHECK(err && !strcmp(err, "step count too large"), "N=%zu: rotate(-N/2) gave '%s'", n, err ? err : "");
}

int check_forest(size_t n, int d, KeySet which, bool fuse, bool print)
{
    std::vector<int> direct_steps{-d};
    for (int l = 1; l < d; ++l) direct_steps.push_back(l);
    const LtKeys K = make_keys(which, n, direct_steps);
    LtPlans P;
    if (const char *err = lt_plans(n, K, d, d, nullptr, nullptr, P)) {
        if (print) printf("FOREST_REFUSED %zu %s %d ! %s\n", n, name_of(which), d, err);
        return 0;
    }
    std::vector<LtNode> nodes;
    std::vector<int> leaf;
    const int max_depth = lt_forest(P, d, fuse, nodes, leaf);
    const char *mode = fuse ? "fused" : "unfused";
    std::set<std::tuple<int, uint32_t, int>> seen;
    int deepest = 0;
    for (size_t i = 0; i < nodes.size(); ++i) {
        const LtNode &nd = nodes[i];
        if (print) printf("NODE %zu %s %d %zu %d %u %d\n", n, name_of(which), d, i, nd.parent, nd.elt, nd.fused);
        CHECK(nd.parent >= -1 && nd.parent < (int)i, "d=%d %s %s: node %zu precedes its parent %d", d, name_of(which), mode, i, nd.parent);
        CHECK(nd.depth == (nd.parent < 0 ? 0 : nodes[(size_t)nd.parent].depth + 1), "d=%d %s %s: depth of node %zu", d, name_of(which), mode, i);
        CHECK(seen.insert({nd.parent, nd.elt, nd.fused}).second, "d=%d %s %s: node %zu repeats (parent, element, diagonal)", d, name_of(which), mode, i);
        CHECK(fuse || nd.fused == -1, "d=%d %s unfused: node %zu carries a diagonal", d, name_of(which), i);
        // a node carries diagonal l only as the last node of plan l
        CHECK(nd.fused == -1 || (nd.fused >= 1 && nd.fused < d && leaf[(size_t)nd.fused] == (int)i), "d=%d %s %s: node %zu carries diagonal %d", d,
              name_of(which), mode, i, nd.fused);
        deepest = nd.depth + 1 > deepest ? nd.depth + 1 : deepest;
    }
    CHECK(max_depth == deepest && leaf.size() == (size_t)d, "d=%d %s %s: depth %d, deepest node %d", d, name_of(which), mode, max_depth, deepest);
    for (int l = 1; l < d; ++l) {  // from the leaf to the root: plan l, last element first
        std::vector<uint32_t> path;
        for (int i = leaf[(size_t)l]; i >= 0; i = nodes[(size_t)i].parent) path.insert(path.begin(), nodes[(size_t)i].elt);
        CHECK(path == std::vector<uint32_t>(P.plan(l), P.plan(l) + P.size(l)), "d=%d %s %s: the path of leaf %d is not plan %d", d, name_of(which), mode, l, l);
        CHECK(!fuse || nodes[(size_t)leaf[(size_t)l]].fused == l, "d=%d %s fused: leaf %d does not carry its diagonal", d, name_of(which), l);
    }
    if (!fuse && which == DEFAULT && d == 6)  // 5 = 1 + 4: the rotation by 1 is shared
        CHECK(nodes[(size_t)leaf[5]].parent == leaf[1] && nodes[(size_t)leaf[1]].parent == -1, "unfused d=6: the leaf of step 1 is not inside step 5's path");
    return (int)nodes.size();
}

void check_lanes(const std::vector<LtNode> &nodes, const char *what)
{
    const size_t n = nodes.size();
    const LtLaneDeal D = lt_deal_lanes(nodes.data(), n, 2, 1 << 30);
    std::vector<int> weight(n, 0), root_of(n);
    int load[2] = {0, 0}, heaviest = 0, roots = 0, max_depth = 0;
    for (size_t i = 0; i < n; ++i) {
        root_of[i] = nodes[i].parent < 0 ? (int)i : root_of[(size_t)nodes[i].parent];
        roots += nodes[i].parent < 0;
        heaviest = std::max(heaviest, ++weight[(size_t)root_of[i]]);
        max_depth = std::max(max_depth, nodes[i].depth + 1);
    }
    CHECK(D.lane_of.size() == n && D.used == (roots >= 2), "%s: %d roots, lanes used = %d", what, roots, D.used);
    int widest = 0;
    for (int depth = 0; depth < max_depth; ++depth)
        for (int lane = 0; lane < 2; ++lane) {
            int cnt = 0;
            for (size_t i = 0; i < n; ++i) cnt += nodes[i].depth == depth && D.lane_of[i] == lane;
            widest = std::max(widest, cnt);
        }
    if (D.used) CHECK(D.widest == widest, "%s: widest %d, counted %d", what, D.widest, widest);
    for (size_t i = 0; i < n; ++i) {
        CHECK(D.lane_of[i] < 2 && D.lane_of[i] == D.lane_of[(size_t)root_of[i]], "%s: node %zu left its subtree's lane", what, i);
        ++load[D.lane_of[i]];
    }
    if (D.used) CHECK(std::abs(load[0] - load[1]) <= heaviest && load[0] > 0 && load[1] > 0, "%s: loads %d and %d, heaviest subtree %d", what, load[0], load[1], heaviest);
    // a cap below the widest batch: one lane
    const LtLaneDeal C = lt_deal_lanes(nodes.data(), n, 2, D.widest - 1);
    CHECK(!C.used && C.widest == D.widest && std::set<uint8_t>(C.lane_of.begin(), C.lane_of.end()) == std::set<uint8_t>{0}, "%s: a cap of %d still uses the lanes",
          what, D.widest - 1);
    CHECK(lt_deal_lanes(nodes.data(), n, 2, D.widest).used == D.used, "%s: a cap of exactly the widest batch", what);
}

}  // namespace

int main()
{
    std::vector<int> all32, to160{-160};
    for (int s = 1; s < 16; ++s) all32.push_back(s), all32.push_back(-s);
    for (int s = 1; s <= 160; ++s) to160.push_back(s);
    check_plans(32, all32, true);
    check_plans(4096, to160, true);
    std::vector<int> naf;
    lt_naf(-7, naf);  // -7 = 1 - 8: least significant term first, signed like the value
    CHECK(naf == (std::vector<int>{1, -8}), "naf(-7)");
    for (int d : {1, 2, 6, 160}) check_store(4096, d);
    for (int d : {1, 2, 6, 160})
        for (KeySet which : {DEFAULT, DIRECT})
            for (bool fuse : {true, false}) check_forest(4096, d, which, fuse, false);
    for (KeySet which : {DEFAULT, NO_PLUS_4}) {  // what the Python planner is compared with
        check_forest(32, 15, which, true, true);
        check_forest(4096, 160, which, true, true);
    }
    // the lanes: the forests the GPU tests rely on are above the 96-node bound of run_forest
    for (bool fuse : {true, false}) {
        LtPlans P;
        std::vector<LtNode> nodes;
        std::vector<int> leaf;
        CHECK(lt_plans(4096, make_keys(DEFAULT, 4096, {}), 160, 160, nullptr, nullptr, P) == nullptr, "plans of d = 160");
        const int depth = lt_forest(P, 160, fuse, nodes, leaf);
        CHECK(nodes.size() >= 96 && depth >= 2, "the d = 160 default-key forest (%s) has %zu nodes, depth %d", fuse ? "fused" : "unfused", nodes.size(), depth);
        printf("d = 160, default keys, %s: %zu nodes, depth %d\n", fuse ? "fused" : "unfused", nodes.size(), depth);
        check_lanes(nodes, fuse ? "d=160 fused" : "d=160 unfused");
        std::vector<LtNode> chain;  // a single root: nothing to deal
        for (int i = 0; i < 100; ++i) chain.push_back(LtNode{i - 1, 3u, -1, i});
        check_lanes(chain, "one chain");
        std::vector<LtNode> two{LtNode{-1, 3u, -1, 0}, LtNode{-1, 9u, -1, 0}, LtNode{1, 3u, -1, 1}};
        check_lanes(two, "two roots");
    }
    if (failures) {
        printf("LT PLAN SELFTEST: %d FAILURES\n", failures);
        return 1;
    }
    printf("LT PLAN SELFTEST PASSED\n");
    return 0;
}
