// hefx_ranges.h -- the aliasing rule of the C-ABI (include/hefx.h, INTEGRATION.md "Aliasing") as one host-only check.
// No HIP in here: drivers/ranges_selftest.cpp compiles it with g++ under the sanitizers and holds it to a plain O(n^2)
// interval comparison.
//
// A call writes n outputs of out_b bytes each and reads lists of inputs, each list with its own block size.  The call is
// fine when
//   - no two outputs share a byte, and
//   - no input shares a byte with an output -- except, for a list that says so (In::in_place), the EXACT in-place form:
//     input i starts where ITS OWN output starts and has the output's size.  Input i's own output is output
//     out0 + i / per_out (per_out = 1: item i's output; per_out = the list's length: the one output of a sum; out0 = n for
//     the inputs of the second of two output lists handed over back to back -- a key-switch batch's rotations, then its sums).
// Adjacent blocks share no byte.  Null entries of an input list are skipped (optional operands); outputs are non-null.
// O((n + inputs) log n) on the host, nothing is submitted.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <utility>
#include <vector>

namespace hefx_ranges {

struct In {
    const uint64_t *const *ptrs;  // host array of `count` pointers
    size_t count;
    size_t bytes;           // size of every block of the list
    bool in_place = false;  // input i may be output out0 + i / per_out, exactly
    size_t per_out = 1;
    size_t out0 = 0;        // index of input 0's own output
};

enum Verdict { FINE = 0, OUTPUTS_OVERLAP = 1, OUTPUT_OVERLAPS_INPUT = 2 };

// the texts the entries report (kept from the first user of the rule, hefx_multiply_sizes: tests match "overlap")
inline const char *text(Verdict v)
{
    return v == OUTPUTS_OVERLAP ? "two outputs overlap" : v == OUTPUT_OVERLAPS_INPUT ? "an output overlaps an input" : nullptr;
}

// which: when non-null and the verdict is OUTPUT_OVERLAPS_INPUT, receives (index of the list, index in the list)
inline Verdict check(size_t n, uint64_t *const *outs, size_t out_b, std::initializer_list<In> ins,
                     std::pair<size_t, size_t> *which = nullptr)
{
    std::vector<std::pair<uintptr_t, size_t>> o(n);
    for (size_t i = 0; i < n; ++i) o[i] = {(uintptr_t)outs[i], i};
    std::sort(o.begin(), o.end());
    if (out_b)
        for (size_t i = 1; i < n; ++i)
            if (o[i - 1].first + out_b > o[i].first) return OUTPUTS_OVERLAP;
    size_t li = 0;
    for (const In &in : ins) {
        for (size_t i = 0; i < in.count && in.bytes && out_b; ++i) {
            const uintptr_t x = (uintptr_t)in.ptrs[i];
            if (!x) continue;
            // the outputs are disjoint: only the last one starting at or before x and the first one after x can meet
            // [x, x + bytes)
            auto it = std::upper_bound(o.begin(), o.end(), std::make_pair(x, (size_t)-1));
            bool hit = it != o.end() && it->first < x + in.bytes;
            if (!hit && it != o.begin()) {
                const auto &p = *(it - 1);
                const bool own = in.in_place && p.first == x && in.bytes == out_b && p.second == in.out0 + i / (in.per_out ? in.per_out : 1);
                hit = p.first + out_b > x && !own;
            }
            if (hit) {
                if (which) *which = {li, i};
                return OUTPUT_OVERLAPS_INPUT;
            }
        }
        ++li;
    }
    return FINE;
}

}  // namespace hefx_ranges
