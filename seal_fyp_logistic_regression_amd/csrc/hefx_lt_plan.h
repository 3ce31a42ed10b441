// hefx_lt_plan.h -- the rotation planner of the linear transforms as host-only integer code: the Galois-key lookup, SEAL's
// rotation plans (rotate_internal: the direct key if present, else the NAF terms of the step, App. A.7), the plans of one
// whole transform, the forest of key-switch nodes they share, and the dealing of its subtrees onto lanes.  No HIP in here:
// drivers/lt_plan_selftest.cpp compiles it with g++ under the sanitizers; tests/test_lt_plan_cpu.py holds it to seal.py.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <utility>
#include <vector>

namespace hefx_lt {

// Galois element -> key payload.  A sorted vector (callers hand the elements over in increasing order: one pass, no
// allocation per key), looked up by binary search: building an unordered_map of 512 keys was 30 us in front of the first
// launch of every direct-key linear transform.
struct LtKeys {
    std::vector<std::pair<uint32_t, const uint64_t *>> v;
    void set(int n, const uint32_t *elts, const uint64_t *const *keys)
    {
        v.resize((size_t)n);
        bool sorted = true;
        for (int i = 0; i < n; ++i) {
            v[(size_t)i] = {elts[i], keys[i]};
            sorted = sorted && (i == 0 || elts[i - 1] < elts[i]);
        }
        if (!sorted) {  // later entries of an element win, like repeated assignment to a map
            std::stable_sort(v.begin(), v.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
            size_t w = 0;
            for (size_t i = 0; i < v.size(); ++i) {
                if (i + 1 < v.size() && v[i + 1].first == v[i].first) continue;
                v[w++] = v[i];
            }
            v.resize(w);
        }
    }
    const uint64_t *at(uint32_t e) const
    {
        auto it = std::lower_bound(v.begin(), v.end(), e, [](const auto &a, uint32_t x) { return a.first < x; });
        return it != v.end() && it->first == e ? it->second : nullptr;
    }
    bool has(uint32_t e) const { return at(e) != nullptr; }
};
inline uint32_t lt_elt_from_step(int step, size_t n)
{
    const uint64_t m = 2 * n;
    if (step == 0) return (uint32_t)(m - 1);
    uint64_t pos = step > 0 ? (uint64_t)step : (uint64_t)((long long)(n / 2) + step);
    uint64_t r = 1, b = 3;
    while (pos) {
        if (pos & 1) r = (r * b) & (m - 1);
        b = (b * b) & (m - 1);
        pos >>= 1;
    }
    return (uint32_t)r;
}
inline void lt_naf(int value, std::vector<int> &out)  // SEAL util::naf: least significant term first, signed like value
{
    const bool neg = value < 0;
    unsigned v = (unsigned)(neg ? -value : value);
    for (int i = 0; v; ++i) {
        const int zi = (v & 1) ? 2 - (int)(v & 3) : 0;
        v = (unsigned)((int)v - zi) >> 1;
        if (zi) out.push_back((neg ? -zi : zi) * (1 << i));
    }
}
// Galois elements rotate_vector(steps) applies, in order, appended to `plan`; nullptr on success, else SEAL's exception text
inline const char *lt_plan(int steps, size_t n, const LtKeys &keys, std::vector<uint32_t> &plan)
{
    if (steps == 0) return nullptr;
    if ((size_t)(steps < 0 ? -steps : steps) >= n / 2) return "step count too large";
    const uint32_t e = lt_elt_from_step(steps, n);
    if (keys.has(e)) {
        plan.push_back(e);
        return nullptr;
    }
    std::vector<int> terms;
    lt_naf(steps, terms);
    if (terms.size() == 1) return "Galois key not present";
    for (int t : terms) {
        if ((size_t)(t < 0 ? -t : t) == n / 2) continue;
        if (const char *err = lt_plan(t, n, keys, plan)) return err;
    }
    return nullptr;
}
// The plans of a whole transform as one flat store: plan 0 is that of rotate(-d) (term 0 of a transform is the unrotated one
// and has none), plan i = 1 .. nterms-1 that of term i; plan i is elts[off[i] .. off[i + 1]).  No vector per term.
struct LtPlans {
    std::vector<uint32_t> elts, off;
    size_t size(int i) const { return off[(size_t)i + 1] - off[(size_t)i]; }
    const uint32_t *plan(int i) const { return elts.data() + off[(size_t)i]; }
};
// rotate(-d), then term i = 1 .. nterms-1 (step steps[i], or i when steps is null).  direct_only: the text a step without a
// direct Galois key (a plan of more than one element) is refused with, by the forms that need one.  A missing key or a step
// too large is reported here, before anything runs, with SEAL's text, like the op-by-op sequence would.  nullptr on success.
inline const char *lt_plans(size_t n, const LtKeys &K, int d, int nterms, const int *steps, const char *direct_only, LtPlans &P)
{
    P.elts.clear(), P.off.assign(1, 0u);
    P.off.reserve((size_t)(nterms > 0 ? nterms : 1) + 1);
    for (int i = 0; i == 0 || i < nterms; ++i) {
        const int step = i == 0 ? -d : steps ? steps[i] : i;
        if (i && step == 0) return "only term 0 may be unrotated";
        if (const char *err = lt_plan(step, n, K, P.elts)) return err;
        P.off.push_back((uint32_t)P.elts.size());
        if (i && direct_only && P.size(i) != 1) return direct_only;
    }
    return nullptr;
}
// plans 1 .. d-1 -> a forest of key-switch nodes rooted at ct_new; leaf[l] = the node that holds rotate(ct_new, l).
// fuse_diagonals (the plain transform): a plan's last node carries diagonal l's product, so nodes de-duplicate per
// (parent, element, fused diagonal); without (the cipher transform) per (parent, element) alone, and the leaf of one
// step may be the prefix of another.  Parents precede their children.  Returns the forest's depth.
struct LtNode {
    int parent;  // -1: ct_new
    uint32_t elt;
    int fused;   // diagonal index whose plaintext multiplies this node's output, or -1
    int depth;
};
inline int lt_forest(const LtPlans &plans, int d, bool fuse_diagonals, std::vector<LtNode> &nodes, std::vector<int> &leaf)
{
    // (parent node + 1, element, fused diagonal + 1) packed into 64 bits: parent < 2^22 nodes, element < 2^16 (N <= 32768),
    // diagonal < 2^22
    std::unordered_map<uint64_t, int> index;
    index.reserve((size_t)d * 2);
    nodes.reserve((size_t)d * 2);
    leaf.assign((size_t)d, -1);
    int max_depth = 0;
    for (int l = 1; l < d; ++l) {
        const uint32_t *plan = plans.plan(l);
        const size_t len = plans.size(l);
        int cur = -1;
        for (size_t t = 0; t < len; ++t) {
            const int fused = fuse_diagonals && t + 1 == len ? l : -1;
            const uint64_t key = ((uint64_t)(cur + 1) << 42) | ((uint64_t)plan[t] << 24) | (uint64_t)(fused + 1);
            auto it = index.find(key);
            if (it == index.end()) {
                nodes.push_back(LtNode{cur, plan[t], fused, (int)t});
                it = index.emplace(key, (int)nodes.size() - 1).first;
                if ((int)t + 1 > max_depth) max_depth = (int)t + 1;
            }
            cur = it->second;
        }
        leaf[(size_t)l] = cur;
    }
    return max_depth;
}
// A depth of a forest is a barrier only inside a subtree, so the subtrees are dealt onto `lanes` (<= 8) lanes of about equal
// size: heaviest subtree first, each onto the lightest lane, equal weights in node order.  A lane's nodes of one depth run as
// one batch of at most `cap` items: the lanes are used only when every lane got a subtree and the widest such batch fits;
// else every node is on lane 0.  Node: anything with `parent` (< 0: a root; a node's parent precedes it) and `depth`.
struct LtLaneDeal {
    std::vector<uint8_t> lane_of;
    int widest = 0;  // the largest number of nodes of one depth on one lane
    bool used = false;
};
template <class Node>
LtLaneDeal lt_deal_lanes(const Node *nodes, size_t n, int lanes, int cap)
{
    LtLaneDeal D;
    D.lane_of.assign(n, 0);
    std::vector<int> root_of(n), weight(n, 0), roots, cnt;
    for (size_t i = 0; i < n; ++i) {
        root_of[i] = nodes[i].parent < 0 ? (int)i : root_of[(size_t)nodes[i].parent];
        ++weight[(size_t)root_of[i]];
        if (nodes[i].parent < 0) roots.push_back((int)i);
    }
    std::stable_sort(roots.begin(), roots.end(), [&](int a, int b) { return weight[(size_t)a] > weight[(size_t)b]; });
    int load[8] = {};
    for (int r : roots) {
        const int ln = (int)(std::min_element(load, load + lanes) - load);  // (the first of equally light lanes)
        D.lane_of[(size_t)r] = (uint8_t)ln;
        load[ln] += weight[(size_t)r];
    }
    for (size_t i = 0; i < n; ++i) {
        D.lane_of[i] = D.lane_of[(size_t)root_of[i]];
        const size_t slot = (size_t)nodes[i].depth * lanes + D.lane_of[i];
        if (cnt.size() <= slot) cnt.resize(slot + 1, 0);
        D.widest = std::max(D.widest, ++cnt[slot]);
    }
    D.used = lanes > 1 && D.widest <= cap && *std::min_element(load, load + lanes) > 0;
    if (!D.used) std::fill(D.lane_of.begin(), D.lane_of.end(), 0);
    return D;
}

}  // namespace hefx_lt
