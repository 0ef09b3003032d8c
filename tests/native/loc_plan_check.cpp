// loc_plan_check.cpp -- the value-and-location fold's host arithmetic
// (osss-gasnet_amd/csrc/loc_plan.h) enumerated on the CPU: built with g++ and
// the address and undefined-behaviour sanitizers and run as an ordinary
// program (tests/test_loc_plan.py).
//
// 1. The chain: for every source count 1 .. 100 and several explicit /
//    implicit location patterns, the planned calls are executed on a symbolic
//    memory -- a call appends the sources it reads to what its entry 0 carried
//    -- and the result must list every source exactly once, in ascending
//    order, each with the location the one-call fold would give it.
// 2. The launch: for every n in 0 .. 5000 and at the edges of the grid passes,
//    both forms and every element size, the index arithmetic of the kernels
//    (loc_kernels.h: lane t of block b takes units b * 256 + t + k * pass, the
//    first `tail` lanes of block 0 one tail element each) must touch every
//    element of [0, n) exactly once and none outside.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "loc_plan.h"

static long violations = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            ++violations;                 \
            if (violations <= 20) {       \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
        }                                 \
    } while (0)

struct Seen {
    int source;
    long loc;  // the location the source's candidates carry (explicit ones: a tag of their own)
};

static long explicit_tag(int source) { return -1000000L - source; }

// pattern: 0 all explicit, 1 all implicit (src_locs == NULL), 2 alternating, 3.. pseudo-random
static bool is_explicit(int pattern, int j, unsigned seed) {
    if (pattern == 0) return true;
    if (pattern == 1) return false;
    if (pattern == 2) return (j & 1) != 0;
    return ((seed * 2654435761u + (unsigned)j * 40503u) >> 7 & 1) != 0;
}

static long chain_calls = 0;

static void check_chain(int nsrc, int pattern, long loc_base) {
    const unsigned seed = (unsigned)(nsrc * 131 + pattern);
    std::vector<Seen> carry;  // what the previous call's output stands for
    const int chunks = mi355_loc_chunk_count(nsrc);
    CHECK(chunks >= 1, "nsrc %d: %d chunks", nsrc, chunks);
    for (int c = 0; c < chunks; ++c) {
        const mi355_loc_chunk k = mi355_loc_chunk_at(nsrc, c);
        ++chain_calls;
        const int entries = k.lead + k.take;
        CHECK(entries >= 1 && entries <= MI355_LOC_MAX_SOURCES, "nsrc %d chunk %d: %d entries", nsrc, c, entries);
        CHECK(k.take >= 1, "nsrc %d chunk %d takes %d", nsrc, c, k.take);
        CHECK((k.lead == 0) == (c == 0), "nsrc %d chunk %d: lead %d", nsrc, c, k.lead);
        CHECK(k.final == (c == chunks - 1), "nsrc %d chunk %d: final %d of %d chunks", nsrc, c, k.final, chunks);
        CHECK(k.first >= 0 && k.first + k.take <= nsrc, "nsrc %d chunk %d: sources %d + %d", nsrc, c, k.first, k.take);
        std::vector<Seen> out;
        if (k.lead) out = carry;  // entry 0: the carry with its explicit location array
        else CHECK(carry.empty(), "nsrc %d: first chunk after a carry", nsrc);
        if (k.first + k.take > nsrc || k.first < 0) return;
        for (int i = 0; i < k.take; ++i) {
            const int source = k.first + i, entry = k.lead + i;
            // the call's implicit location of entry `entry`: its loc_base + entry
            const long loc = is_explicit(pattern, source, seed) ? explicit_tag(source) : loc_base + k.loc_shift + entry;
            out.push_back({source, loc});
        }
        carry = out;
    }
    CHECK((int)carry.size() == nsrc, "nsrc %d pattern %d: %zu sources visited", nsrc, pattern, carry.size());
    for (int j = 0; j < (int)carry.size() && j < nsrc; ++j) {
        CHECK(carry[j].source == j, "nsrc %d pattern %d: position %d holds source %d", nsrc, pattern, j, carry[j].source);
        const long want = is_explicit(pattern, j, seed) ? explicit_tag(j) : loc_base + j;
        CHECK(carry[j].loc == want, "nsrc %d pattern %d: source %d has location %ld, want %ld", nsrc, pattern, j,
              carry[j].loc, want);
    }
}

static long launches = 0;

static void check_launch(size_t es, int aligned, uint64_t n, int cus) {
    const mi355_loc_plan p = mi355_loc_plan_launch(es, aligned, n, cus);
    ++launches;
    if (n == 0) {
        CHECK(p.grid == 0, "n 0: grid %u", p.grid);
        return;
    }
    const unsigned V = aligned ? (unsigned)(16 / es) : 1;
    CHECK(p.form == (aligned ? MI355_LOC_VECTOR : MI355_LOC_ELEMENT), "es %zu aligned %d: form %d", es, aligned, p.form);
    CHECK(p.per_lane == V, "es %zu aligned %d: %u per lane", es, aligned, p.per_lane);
    CHECK(p.nvec * V + p.tail == n && p.tail < V, "n %llu: %llu x %u + %u", (unsigned long long)n,
          (unsigned long long)p.nvec, V, p.tail);
    CHECK(p.grid >= 1 && p.grid <= (unsigned)cus * MI355_LOC_BLOCKS_PER_CU, "n %llu cus %d: grid %u",
          (unsigned long long)n, cus, p.grid);
    CHECK(p.pass == (uint64_t)p.grid * MI355_LOC_BLOCK, "pass %llu of grid %u", (unsigned long long)p.pass, p.grid);
    // no more blocks than units (beyond the one a tail needs)
    CHECK(p.grid == 1 || (uint64_t)(p.grid - 1) * MI355_LOC_BLOCK < p.nvec, "n %llu: grid %u for %llu units",
          (unsigned long long)n, p.grid, (unsigned long long)p.nvec);
    std::vector<unsigned char> hit(n, 0);
    for (unsigned b = 0; b < p.grid; ++b)
        for (unsigned t = 0; t < MI355_LOC_BLOCK; ++t) {
            const uint64_t g = (uint64_t)b * MI355_LOC_BLOCK + t;
            for (uint64_t i = g; i < p.nvec; i += p.pass)
                for (unsigned e = 0; e < V; ++e) {
                    const uint64_t x = i * V + e;
                    CHECK(x < n, "n %llu: element %llu out of range", (unsigned long long)n, (unsigned long long)x);
                    if (x < n) ++hit[x];
                }
            if (p.form == MI355_LOC_VECTOR && g < p.tail) {
                const uint64_t x = p.nvec * V + g;
                CHECK(x < n, "n %llu: tail element %llu out of range", (unsigned long long)n, (unsigned long long)x);
                if (x < n) ++hit[x];
            }
        }
    for (uint64_t x = 0; x < n; ++x)
        if (hit[x] != 1) {
            CHECK(false, "es %zu aligned %d n %llu cus %d: element %llu touched %d times", es, aligned,
                  (unsigned long long)n, cus, (unsigned long long)x, (int)hit[x]);
            break;
        }
}

int main() {
    long chains = 0;
    for (int nsrc = 1; nsrc <= 100; ++nsrc)
        for (int pattern = 0; pattern < 8; ++pattern)
            for (long base : {0L, 7L, -40L}) {
                check_chain(nsrc, pattern, base);
                ++chains;
            }
    // the counts the chunks must have: 32, then 31 more per call
    CHECK(mi355_loc_chunk_count(32) == 1 && mi355_loc_chunk_count(33) == 2 && mi355_loc_chunk_count(63) == 2 &&
              mi355_loc_chunk_count(64) == 3 && mi355_loc_chunk_count(100) == 4,
          "chunk counts");

    // the form: vectors only when every given pointer is 16-byte aligned; a NULL location entry reads nothing
    {
        alignas(16) static char buf[256];
        const void *sv[3] = {buf, buf + 16, buf + 32};
        const long *sl[3] = {(const long *)(buf + 48), nullptr, (const long *)(buf + 64)};
        CHECK(mi355_loc_aligned(buf + 80, buf + 96, sv, sl, 3) == 1, "aligned pointers");
        CHECK(mi355_loc_aligned(buf + 80, buf + 96, sv, nullptr, 3) == 1, "aligned pointers, implicit locations");
        CHECK(mi355_loc_aligned(buf + 82, buf + 96, sv, sl, 3) == 0, "dst_val off by 2");
        CHECK(mi355_loc_aligned(buf + 80, buf + 104, sv, sl, 3) == 0, "dst_loc off by 8");
        sv[2] = buf + 36;
        CHECK(mi355_loc_aligned(buf + 80, buf + 96, sv, sl, 3) == 0, "a value source off by 4");
        CHECK(mi355_loc_aligned(buf + 80, buf + 96, sv, sl, 2) == 1, "... which a shorter call does not read");
        sv[2] = buf + 32;
        sl[0] = (const long *)(buf + 56);
        CHECK(mi355_loc_aligned(buf + 80, buf + 96, sv, sl, 3) == 0, "a location source off by 8");
        CHECK(mi355_loc_aligned(buf + 80, buf + 96, sv, nullptr, 3) == 1, "... which an implicit call does not read");
    }

    const size_t sizes[] = {2, 4, 8};
    for (size_t es : sizes)
        for (int aligned = 0; aligned <= 1; ++aligned) {
            for (uint64_t n = 0; n <= 5000; ++n) check_launch(es, aligned, n, 2);
            for (int cus : {1, 3, 256}) {
                const uint64_t V = aligned ? 16 / es : 1;
                const uint64_t full = (uint64_t)cus * MI355_LOC_BLOCKS_PER_CU * MI355_LOC_BLOCK * V;  // one full pass
                for (uint64_t k : {(uint64_t)1, (uint64_t)2})
                    for (long d = -(long)V - 1; d <= (long)V + 1; ++d) check_launch(es, aligned, k * full + d, cus);
            }
        }
    std::printf("%ld chains, %ld calls, %ld launches, %ld violations\n", chains, chain_calls, launches, violations);
    return violations == 0 ? 0 : 1;
}
