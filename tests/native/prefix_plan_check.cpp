// prefix_plan_check.cpp -- osss-gasnet_amd/csrc/prefix_plan.h on the CPU
// (tests/test_prefix_plan.py builds it with g++ -fsanitize=address,undefined):
// the chained launches of a prefix fold are RUN on a symbolic memory -- every
// buffer holds "source k" or "prefix k" -- over every source count and
// thousands of output patterns (NULL slots, in-place outputs), and every
// output must end up holding its prefix, every source that no output aliases
// its own value, and every launch must read only values that are still there.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "prefix_plan.h"

namespace {

struct Value {
    int kind;  // 0: untouched output buffer, 1: source k, 2: prefix k
    int k;
    bool operator==(const Value &o) const { return kind == o.kind && k == o.k; }
};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

long violations = 0, cases = 0, rejected = 0, launches = 0;

void fail(const char *what, int nsrc, int c) {
    if (violations < 20) fprintf(stderr, "violation: %s (nsrc %d, chunk %d)\n", what, nsrc, c);
    ++violations;
}

// One pattern: dsts[j] NULL, a buffer of its own, or (alias) srcs[j] itself.
void run_case(int nsrc, const std::vector<int> &mode) {
    ++cases;
    std::vector<char> src_buf(nsrc), dst_buf(nsrc);   // identities only; never dereferenced by the plan
    std::vector<const void *> srcs(nsrc);
    std::vector<void *> dsts(nsrc);
    std::map<const void *, Value> mem;
    for (int k = 0; k < nsrc; ++k) {
        srcs[k] = &src_buf[k];
        mem[srcs[k]] = Value{1, k};
        dsts[k] = mode[k] == 0 ? nullptr : mode[k] == 1 ? (void *)&dst_buf[k] : (void *)&src_buf[k];
        if (mode[k] == 1) mem[dsts[k]] = Value{0, k};
    }
    const int used = mi355_prefix_trim(dsts.data(), nsrc);
    int last = 0;
    for (int k = 0; k < nsrc; ++k)
        if (dsts[k] != nullptr) last = k + 1;
    if (used != last) fail("trim", nsrc, -1);
    if (used < 2) return;   // nothing, or a copy: no chain
    const int chunks = mi355_prefix_chunk_count(used);
    void *carry = nullptr;
    int next_source = 0;   // sources consumed so far
    for (int c = 0; c < chunks; ++c) {
        mi355_prefix_chunk ch;
        memset(&ch, 0x5A, sizeof ch);
        const void *carry_in = carry;
        const int rc = mi355_prefix_chunk_at(dsts.data(), srcs.data(), used, c, carry_in, &ch, &carry);
        if (rc != 0) {
            // allowed only when no later output could hold the carry
            const int slot = next_source + (ch.nsrc - (c ? 1 : 0)) - 1;
            bool any = false;
            for (int j = slot + 1; j < used; ++j) any |= mode[j] == 1;
            if (dsts[slot] != nullptr || any) fail("rejected although a carry buffer exists", nsrc, c);
            ++rejected;
            return;
        }
        ++launches;
        if (ch.nsrc < 2 || ch.nsrc > MI355_PREFIX_LAUNCH_SOURCES) fail("launch width", nsrc, c);
        if ((ch.final != 0) != (c == chunks - 1)) fail("final flag", nsrc, c);
        // the launch: every load of a position precedes every store to it
        std::vector<Value> in(ch.nsrc);
        for (int k = 0; k < ch.nsrc; ++k) {
            if (ch.src[k] == nullptr) {
                fail("null source", nsrc, c);
                return;
            }
            in[k] = mem[ch.src[k]];
        }
        int first_new = 0;
        if (c == 0) {
            if (!(in[0] == Value{1, 0})) fail("first source", nsrc, c);
            first_new = 1;
            next_source = 1;
        } else {
            if (ch.src[0] != carry_in || !(in[0] == Value{2, next_source - 1})) fail("carry is not the prefix so far", nsrc, c);
            if (ch.dst[0] != nullptr) fail("the carry's slot is stored again", nsrc, c);
            first_new = 1;
        }
        int prefix = next_source - 1;
        if (c == 0 && ch.dst[0] != nullptr) mem[ch.dst[0]] = Value{2, 0};
        for (int k = first_new; k < ch.nsrc; ++k) {
            if (!(in[k] == Value{1, next_source})) fail("a source was overwritten before its launch read it", nsrc, c);
            ++next_source;
            ++prefix;
            if (ch.dst[k] != nullptr) mem[ch.dst[k]] = Value{2, prefix};
        }
        for (int k = ch.nsrc; k < MI355_PREFIX_LAUNCH_SOURCES; ++k)
            if (ch.src[k] != nullptr || ch.dst[k] != nullptr) fail("entries past nsrc not cleared", nsrc, c);
        if (!ch.final && (carry == nullptr || !(mem[carry] == Value{2, prefix}))) fail("carry out", nsrc, c);
        if (ch.final && carry != nullptr) fail("carry after the final launch", nsrc, c);
    }
    if (next_source != used) fail("sources consumed", nsrc, chunks);
    for (int k = 0; k < used; ++k) {
        if (dsts[k] != nullptr && !(mem[dsts[k]] == Value{2, k})) fail("an output does not hold its prefix", nsrc, k);
        if (mode[k] != 2 && !(mem[srcs[k]] == Value{1, k})) fail("a source changed", nsrc, k);
    }
}

}  // namespace

int main() {
    // the scan collectives' slots
    for (int size = 1; size <= 64; ++size) {
        for (int excl = 0; excl <= 1; ++excl) {
            const int nsrc = mi355_scan_sources(excl, size);
            if (nsrc != size - excl) fail("scan sources", size, excl);
            int seen = 0;
            for (int q = 0; q < size; ++q) {
                const int j = mi355_scan_slot(excl, q);
                if (j != q - excl || j >= nsrc) fail("scan slot", size, q);
                seen += j >= 0;
            }
            if (seen != nsrc) fail("every computed prefix has exactly one taker", size, excl);
        }
    }
    for (int nsrc = 1; nsrc <= 32; ++nsrc) {
        const int want = nsrc <= 8 ? 1 : 1 + (nsrc - 8 + 6) / 7;
        if (mi355_prefix_chunk_count(nsrc) != want) fail("chunk count", nsrc, -1);
        std::vector<int> mode(nsrc);
        // every output set; every output in place; the exscan shapes; one output only
        for (int fill = 1; fill <= 2; ++fill) {
            for (int k = 0; k < nsrc; ++k) mode[k] = fill;
            run_case(nsrc, mode);
            mode[nsrc - 1] = 0;
            run_case(nsrc, mode);
            mode[nsrc - 1] = fill;
            mode[0] = 0;
            run_case(nsrc, mode);
        }
        for (int only = 0; only < nsrc; ++only) {
            for (int k = 0; k < nsrc; ++k) mode[k] = k == only ? 1 : 0;
            run_case(nsrc, mode);
            for (int k = 0; k < nsrc; ++k) mode[k] = k == only ? 2 : 0;
            run_case(nsrc, mode);
        }
        for (int r = 0; r < 4000; ++r) {
            const uint32_t density = rnd() % 4;
            for (int k = 0; k < nsrc; ++k) {
                const uint32_t x = rnd() % 8;
                mode[k] = x <= density ? 0 : x == 7 ? 2 : 1;
            }
            run_case(nsrc, mode);
        }
    }
    printf("%ld cases, %ld launches, %ld rejected, %ld violations\n", cases, launches, rejected, violations);
    return violations == 0 ? 0 : 1;
}
