// ranges_selftest.cpp -- csrc/hefx_ranges.h (the byte-range aliasing check of the C-ABI) against a plain O(n^2) interval
// comparison written here, on a few thousand seeded random layouts: views of one slab, exactly adjacent blocks, one-byte
// overlaps, repeated inputs, equal outputs, and the exact-in-place clause on the right and on the wrong item.  Then layouts
// with TWO output lists back to back (a key-switch batch's rotations and its sums), the second list's inputs carrying
// In::out0 = n: the exact alias on the right item, on the wrong item, and on the right index of the wrong list.
// Host only: no HIP, no device.  tests/test_aliasing_cpu.py builds it with g++ -fsanitize=address,undefined and runs it.
// The addresses are numbers inside an imaginary slab; nothing is dereferenced.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../seal_fyp_logistic_regression_amd/csrc/hefx_ranges.h"

namespace {

uint64_t rng_state;
uint64_t rnd()  // splitmix64
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
size_t below(size_t n) { return (size_t)(rnd() % n); }
bool chance(int percent) { return (int)below(100) < percent; }

struct List {
    std::vector<uintptr_t> at;
    size_t bytes;
    bool in_place;
    size_t per_out;
    size_t out0 = 0;
};

bool meet(uintptr_t a, size_t alen, uintptr_t b, size_t blen) { return a < b + blen && b < a + alen; }

// the rule, stated the slow way
hefx_ranges::Verdict slow(const std::vector<uintptr_t> &outs, size_t out_b, const std::vector<List> &lists,
                          std::vector<std::pair<size_t, size_t>> &offenders)
{
    for (size_t i = 0; i < outs.size(); ++i)
        for (size_t j = i + 1; j < outs.size(); ++j)
            if (meet(outs[i], out_b, outs[j], out_b)) return hefx_ranges::OUTPUTS_OVERLAP;
    for (size_t l = 0; l < lists.size(); ++l)
        for (size_t i = 0; i < lists[l].at.size(); ++i) {
            const uintptr_t x = lists[l].at[i];
            if (!x) continue;
            for (size_t j = 0; j < outs.size(); ++j) {
                if (!meet(x, lists[l].bytes, outs[j], out_b)) continue;
                const bool own = lists[l].in_place && x == outs[j] && lists[l].bytes == out_b && j == lists[l].out0 + i / lists[l].per_out;
                if (!own) {
                    offenders.push_back({l, i});
                    break;
                }
            }
        }
    return offenders.empty() ? hefx_ranges::FINE : hefx_ranges::OUTPUT_OVERLAPS_INPUT;
}

// the header's answer against the slow one: the verdict both give, or -1 (printed) when they differ
int compare(int round, const std::vector<uintptr_t> &outs, size_t out_b, const std::vector<List> &lists)
{
    const size_t n = outs.size();
    std::vector<uint64_t *> op(n);
    for (size_t i = 0; i < n; ++i) op[i] = reinterpret_cast<uint64_t *>(outs[i]);
    std::vector<std::vector<const uint64_t *>> ip(lists.size());
    hefx_ranges::In in[3] = {};
    for (size_t l = 0; l < lists.size(); ++l) {
        for (uintptr_t a : lists[l].at) ip[l].push_back(reinterpret_cast<const uint64_t *>(a));
        in[l] = hefx_ranges::In{ip[l].data(), ip[l].size(), lists[l].bytes, lists[l].in_place, lists[l].per_out, lists[l].out0};
    }
    std::pair<size_t, size_t> which{(size_t)-1, (size_t)-1};
    hefx_ranges::Verdict got;
    switch (lists.size()) {
        case 0: got = hefx_ranges::check(n, op.data(), out_b, {}, &which); break;
        case 1: got = hefx_ranges::check(n, op.data(), out_b, {in[0]}, &which); break;
        case 2: got = hefx_ranges::check(n, op.data(), out_b, {in[0], in[1]}, &which); break;
        default: got = hefx_ranges::check(n, op.data(), out_b, {in[0], in[1], in[2]}, &which); break;
    }
    std::vector<std::pair<size_t, size_t>> offenders;
    const hefx_ranges::Verdict want = slow(outs, out_b, lists, offenders);
    bool ok = got == want;
    if (ok && want == hefx_ranges::OUTPUT_OVERLAPS_INPUT) {  // the input it names is one that does overlap
        ok = false;
        for (const auto &f : offenders) ok = ok || f == which;
    }
    if (ok) return (int)want;
    const uintptr_t slab = outs.empty() ? 0 : outs[0];
    printf("FAIL round %d: header says %d (list %zu, input %zu), the interval comparison says %d; n = %zu, out_b = %zu\n", round,
           (int)got, which.first, which.second, (int)want, n, out_b);
    for (size_t i = 0; i < n; ++i) printf("  out[%zu] = out[0] + %lld\n", i, (long long)(outs[i] - slab));
    for (size_t l = 0; l < lists.size(); ++l)
        for (size_t i = 0; i < lists[l].at.size(); ++i)
            printf("  in%zu[%zu] = out[0] + %lld, %zu bytes, in_place %d, per_out %zu, out0 %zu\n", l, i,
                   lists[l].at[i] ? (long long)(lists[l].at[i] - slab) : -1ll, lists[l].bytes, (int)lists[l].in_place,
                   lists[l].per_out, lists[l].out0);
    return -1;
}

}  // namespace

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 6000;
    const uintptr_t slab = (uintptr_t)1 << 32;  // the imaginary allocation every view lies in
    size_t seen[3] = {0, 0, 0}, in_place_served = 0, wrong_item = 0, adjacent_fine = 0, one_byte = 0, repeats = 0;
    for (int round = 0; round < rounds; ++round) {
        rng_state = 0x5eed0000ull + (uint64_t)round;
        const size_t sizes[] = {1, 8, 24, 64, 4096};
        const size_t out_b = sizes[below(5)];
        const size_t n = 1 + below(chance(30) ? 1 : 9);
        std::vector<uintptr_t> outs(n);
        std::vector<List> lists(below(4));
        const bool soup = chance(25);   // random places in a small slab: mostly overlapping
        const bool clean = chance(50);  // only the forms the rule serves are planted (what the layout is, the slow way decides)
        uintptr_t cursor = slab + below(3) * 8;
        auto place = [&](size_t bytes) {
            if (soup) return slab + below(6 * (out_b + 8));
            cursor += chance(50) ? 0 : below(3 * bytes);  // exactly adjacent to the block before it, or after a gap
            const uintptr_t at = cursor;
            cursor += bytes;
            return at;
        };
        for (size_t i = 0; i < n; ++i) outs[i] = place(out_b);
        bool planted_adjacent_only = !soup, planted_one_byte = false, planted_wrong = false, planted_own = false, planted_repeat = false;
        for (List &ls : lists) {
            const size_t same = chance(60);
            ls.bytes = same ? out_b : sizes[below(5)];
            ls.in_place = chance(50);
            const size_t cnt = chance(50) ? n : 1 + below(12);
            ls.per_out = chance(70) ? 1 : cnt;
            ls.at.resize(cnt);
            for (size_t i = 0; i < cnt; ++i) {
                int kind = (int)below(100);
                const size_t own = i / ls.per_out;
                if (clean) kind = kind < 40 ? 0 : kind < 65 ? 45 : kind < 80 ? 84 : kind < 95 ? 90 : 99;
                if (kind < 45 || soup) {
                    ls.at[i] = place(ls.bytes);
                } else if (kind < 60 && own < n) {  // in place on its own output
                    ls.at[i] = outs[own];
                    planted_own = true;
                } else if (kind < 68 && n > 1) {    // "in place" on another item's output
                    size_t j = below(n);
                    if (j == own) j = (j + 1) % n;
                    ls.at[i] = outs[j];
                    planted_wrong = true;
                } else if (kind < 76) {             // last byte of an output
                    ls.at[i] = outs[below(n)] + out_b - 1;
                    planted_one_byte = true;
                } else if (kind < 84) {             // first byte of an output
                    const uintptr_t o = outs[below(n)];
                    ls.at[i] = o - (ls.bytes - 1);
                    planted_one_byte = true;
                } else if (kind < 90) {             // exactly behind / in front of an output (may still meet a neighbour)
                    const uintptr_t o = outs[below(n)];
                    ls.at[i] = chance(50) ? o + out_b : o - ls.bytes;
                } else if (kind < 97 && i > 0) {    // an input that repeats
                    ls.at[i] = ls.at[below(i)];
                    planted_repeat = true;
                } else {
                    ls.at[i] = 0;  // optional operand left out
                }
            }
        }
        if (!soup && !clean && n > 1 && chance(25)) {  // two outputs sharing one byte, or equal
            const size_t i = below(n - 1);
            outs[i + 1] = chance(50) ? outs[i] : outs[i] + out_b - 1;
        }
        const int verdict = compare(round, outs, out_b, lists);
        if (verdict < 0) return 1;
        const hefx_ranges::Verdict want = (hefx_ranges::Verdict)verdict;
        ++seen[want];
        if (want == hefx_ranges::FINE) {
            in_place_served += planted_own;
            adjacent_fine += planted_adjacent_only && !lists.empty();
            repeats += planted_repeat;
        } else {
            wrong_item += planted_wrong;
            one_byte += planted_one_byte;
        }
    }
    printf("%d layouts: %zu fine (%zu with an exact in-place input, %zu of adjacent views, %zu with repeated inputs), "
           "%zu with overlapping outputs, %zu with an output on an input (%zu beside a wrong-item alias, %zu beside a one-byte overlap)\n",
           rounds, seen[0], in_place_served, adjacent_fine, repeats, seen[1], seen[2], wrong_item, one_byte);
    // every kind of layout must have been drawn often enough for the agreement above to mean something
    const size_t floor_ = (size_t)rounds / 100;
    if (seen[0] < 5 * floor_ || seen[1] < 5 * floor_ || seen[2] < 5 * floor_ || in_place_served < floor_ || wrong_item < floor_ ||
        adjacent_fine < floor_ || one_byte < floor_ || repeats < floor_) {
        printf("FAIL: a kind of layout is missing from the draw\n");
        return 1;
    }
    // ---- two output lists back to back (n rotations, then n sums; hefx_capi.cpp's ks_run): list 0 belongs to the first n outputs
    // (out0 = 0), list 1 to the second n (out0 = n).  A quarter as many layouts again, seeded apart from the ones above.
    size_t two_seen[3] = {0, 0, 0}, right_item = 0, wrong_item2 = 0, wrong_list = 0;
    for (int round = 0; round < rounds / 4; ++round) {
        rng_state = 0x2715750000ull + (uint64_t)round;
        const size_t out_b = 8 * (1 + below(8)), n = 1 + below(6);
        std::vector<uintptr_t> outs(2 * n);
        uintptr_t cursor = slab;
        auto place = [&] {
            cursor += chance(50) ? 0 : below(3 * out_b);
            const uintptr_t at = cursor;
            cursor += out_b;
            return at;
        };
        for (uintptr_t &o : outs) o = place();
        std::vector<List> lists(2);
        const int plant = (int)below(4);  // what this layout may hold beside fresh blocks: 0 only own aliases, 1 .. 3 one offender kind
        bool planted_right = false, planted_wrong = false, planted_list = false;
        for (size_t l = 0; l < 2; ++l) {
            List &ls = lists[l];
            ls.bytes = out_b, ls.in_place = plant == 0 || chance(70), ls.per_out = 1, ls.out0 = l * n;
            ls.at.resize(n);
            for (size_t i = 0; i < n; ++i) {
                const int kind = (int)below(100);
                if (kind < 40) {
                    ls.at[i] = place();
                } else if (kind < 50) {
                    ls.at[i] = 0;
                } else if (plant == 0 || kind < 70) {  // its own output, exactly
                    ls.at[i] = outs[ls.out0 + i];
                    planted_right = planted_right || ls.in_place;
                } else if (plant == 1 && n > 1) {      // another item's output of its own list
                    ls.at[i] = outs[ls.out0 + (i + 1 + below(n - 1)) % n];
                    planted_wrong = true;
                } else if (plant == 2) {               // its own index, in the other list
                    ls.at[i] = outs[(n - ls.out0) + i];
                    planted_list = true;
                } else {
                    ls.at[i] = place();
                }
            }
        }
        const int verdict = compare(rounds + round, outs, out_b, lists);
        if (verdict < 0) return 1;
        ++two_seen[verdict];
        if (verdict == hefx_ranges::OUTPUTS_OVERLAP) {
            printf("FAIL: a two-list layout was generated with overlapping outputs\n");
            return 1;
        }
        if (verdict == hefx_ranges::FINE) {
            right_item += planted_right;
            if (planted_wrong || planted_list) {
                printf("FAIL round %d: an alias on the wrong item or the wrong list was served\n", rounds + round);
                return 1;
            }
        } else {
            wrong_item2 += planted_wrong;
            wrong_list += planted_list;
        }
    }
    printf("%d layouts with two output lists: %zu fine (%zu with an exact in-place input on its own output), %zu with an output on an "
           "input (%zu on another item of its list, %zu on its own index of the other list)\n",
           rounds / 4, two_seen[0], right_item, two_seen[2], wrong_item2, wrong_list);
    if (right_item < floor_ || wrong_item2 < floor_ || wrong_list < floor_) {
        printf("FAIL: a kind of two-list layout is missing from the draw\n");
        return 1;
    }
    printf("RANGES SELFTEST PASSED\n");
    return 0;
}
