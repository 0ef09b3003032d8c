// launch_plan_check.cpp -- csrc/launch_plan.h on the host: every combination
// of output and source phases the launchers can meet, the plan's invariants
// checked on each, and a digest of every plan for tests/test_launch_plan.py to
// hold against the constant recorded from the rules the planner replaced.
//
//   launch_plan_check                  enumerate: "<cases> cases (.. per kind), digest <hex>, <n> violations"
//   launch_plan_check plan CASE...     one line "KIND head nvec tail" per case,
//                                      CASE = es:shiftable:n:out,out,..:src,src,..
//                                      (byte addresses; "-" for no outputs)
//   launch_plan_check caps CAP...      the grid of each, one per line: CAP =
//                                      stream:units:per_pass:cus:blocks_per_cu (streaming_grid) or
//                                      resident:occupancy:cus:share:want (coresident_cap)
//   launch_plan_check capsweep         the two caps' sweep: "<cases> cases, digest <hex>, <n> violations"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "launch_plan.h"

using mi355k::LaunchPlan;
using mi355k::plan_launch;

static const char *kind_name(int k) {
    return k == mi355k::PLAN_ALIGNED ? "ALIGNED" : k == mi355k::PLAN_SHIFT ? "SHIFT" : "ELEMENTS";
}

static uint64_t g_digest = 1469598103934665603ull;  // FNV-1a, 64 bits
static void digest_u64(uint64_t v, int bytes) {
    for (int i = 0; i < bytes; ++i) {
        g_digest ^= (v >> (8 * i)) & 0xFF;
        g_digest *= 1099511628211ull;
    }
}

static long g_cases = 0, g_bad = 0, g_kinds[3] = {0, 0, 0};

static void fail(const char *what, size_t es, bool shiftable, const std::vector<uintptr_t> &outs,
                 const std::vector<uintptr_t> &srcs, size_t n, const LaunchPlan &p) {
    if (++g_bad > 20) return;
    printf("VIOLATION %s: es %zu shiftable %d n %zu -> %s head %zu nvec %zu tail %zu; outs", what, es, (int)shiftable, n,
           kind_name(p.kind), p.head, p.nvec, p.tail);
    for (uintptr_t o : outs) printf(" %#zx", (size_t)o);
    printf("; srcs");
    for (uintptr_t s : srcs) printf(" %#zx", (size_t)s);
    printf("\n");
}

static LaunchPlan plan_of(size_t es, bool shiftable, const std::vector<uintptr_t> &outs,
                          const std::vector<uintptr_t> &srcs, size_t n) {
    const void *o[8], *s[8];
    for (size_t k = 0; k < outs.size(); ++k) o[k] = (const void *)outs[k];
    for (size_t k = 0; k < srcs.size(); ++k) s[k] = (const void *)srcs[k];
    return plan_launch(es, shiftable, o, (int)outs.size(), s, (int)srcs.size(), n);
}

static void check(size_t es, bool shiftable, const std::vector<uintptr_t> &outs, const std::vector<uintptr_t> &srcs,
                  size_t n) {
    const size_t V = 16 / es;
    const LaunchPlan p = plan_of(es, shiftable, outs, srcs, n);
    ++g_cases;
    const int kind = p.kind == mi355k::PLAN_ALIGNED ? 0 : p.kind == mi355k::PLAN_SHIFT ? 1 : 2;
    ++g_kinds[kind];
    digest_u64((uint64_t)kind, 1);
    digest_u64(p.head, 8);
    digest_u64(p.nvec, 8);
    digest_u64(p.tail, 8);
#define REQUIRE(c) \
    if (!(c)) fail(#c, es, shiftable, outs, srcs, n, p)
    if (kind == 2) {
        REQUIRE(p.head == 0 && p.tail == 0 && p.nvec == n);
        return;
    }
    REQUIRE(p.head + p.nvec * V + p.tail == n);
    REQUIRE(p.tail < V);
    bool line = true;
    for (uintptr_t o : outs) {
        REQUIRE(((o + p.head * es) & 15) == 0);
        line = line && (o & 127) == (outs[0] & 127);
    }
    // whole-line outputs whenever they share a line offset and n reaches past the line head
    // (16-byte elements are never peeled: the kernels fold a head only for V > 1)
    if (V > 1 && !outs.empty() && line && n > ((128 - (outs[0] & 127)) & 127) / es)
        for (uintptr_t o : outs) REQUIRE(((o + p.head * es) & 127) == 0);
    bool srcs_aligned = true;
    for (uintptr_t s : srcs) srcs_aligned = srcs_aligned && ((s + p.head * es) & 15) == 0;
    if (kind == 0) REQUIRE(srcs_aligned);
    if (kind == 1) REQUIRE(!srcs_aligned && shiftable && p.nvec >= 1 && !outs.empty());
#undef REQUIRE
}

// every n around the vector and head boundaries of one pointer set
static void sizes(size_t es, bool shiftable, const std::vector<uintptr_t> &outs, const std::vector<uintptr_t> &srcs) {
    const long V = 16 / (long)es;
    const long h = outs.empty() ? 0 : (long)(((128 - (outs[0] & 127)) & 127) / es);
    const long ns[] = {0, 1, V - 1, V, V + 1, h - 1, h, h + 1, h + V - 1, h + V, h + V + 1, 1000};
    for (long n : ns)
        if (n >= 0) check(es, shiftable, outs, srcs, (size_t)n);
}

// 1-8 sources, each at phase 0 or at one other phase q, in five mixes
static void sources(size_t es, bool shiftable, const std::vector<uintptr_t> &outs) {
    for (int nsrc = 1; nsrc <= 8; ++nsrc) {
        for (unsigned q = 0; q < 16; ++q) {
            for (int mix = 0; mix < (q == 0 ? 1 : 5); ++mix) {
                std::vector<uintptr_t> srcs;
                for (int k = 0; k < nsrc; ++k) {
                    const bool at_q = mix == 0 ? true : mix == 1 ? k == 0 : mix == 2 ? k == nsrc - 1
                                    : mix == 3 ? k % 2 == 1 : k != 0;
                    srcs.push_back(0x20000000u + (uintptr_t)k * 0x100000u + (at_q ? q : 0));
                }
                sizes(es, shiftable, outs, srcs);
            }
        }
    }
}

static std::vector<uintptr_t> outputs(int nout, uintptr_t off_even, uintptr_t off_odd) {
    std::vector<uintptr_t> outs;
    for (int k = 0; k < nout; ++k) outs.push_back(0x10000000u + (uintptr_t)k * 0x100000u + (k % 2 ? off_odd : off_even));
    return outs;
}

static void enumerate() {
    struct { size_t es; bool shiftable; } types[] = {{2, true}, {4, true}, {8, true}, {16, true}, {16, false}};
    for (auto t : types) {
        const size_t es = t.es;
        const uintptr_t step = es < 16 ? es : 8;   // an element-aligned offset off the 16-byte phase
        for (int nout : {1, 2, 8}) {
            // every output at one offset within its line: every multiple of the element size, and one that is none
            for (uintptr_t pl = 0; pl < 128; pl += es) sources(es, t.shiftable, outputs(nout, pl, pl));
            sources(es, t.shiftable, outputs(nout, 1, 1));
            if (nout == 1) continue;
            // different line offsets at one 16-byte phase; different 16-byte phases
            sources(es, t.shiftable, outputs(nout, 16 + es % 16, 48 + es % 16));
            sources(es, t.shiftable, outputs(nout, 0, step));
        }
        sources(es, t.shiftable, {});
    }
}

static std::vector<uintptr_t> parse_list(const std::string &s) {
    std::vector<uintptr_t> v;
    if (s == "-") return v;
    size_t at = 0;
    while (at <= s.size()) {
        const size_t comma = s.find(',', at);
        const std::string item = s.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        v.push_back((uintptr_t)strtoull(item.c_str(), nullptr, 0));
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    return v;
}

// The two grid caps over every combination of the values below: 1 <= grid <=
// max(cap, 1) with the cap worked out here from the rule, never fewer blocks
// for more work, and a digest of every grid.
static int cap_sweep() {
    long cases = 0, bad = 0;
    auto require = [&](bool ok, const char *what, uint64_t a, uint64_t b, uint64_t c, uint64_t d, unsigned grid) {
        if (!ok && ++bad <= 20)
            printf("VIOLATION %s: %llu %llu %llu %llu -> %u\n", what, (unsigned long long)a, (unsigned long long)b,
                   (unsigned long long)c, (unsigned long long)d, grid);
    };
    const int cus_of[] = {1, 4, 256, 304};
    for (uint64_t per_pass : {1ull, 256ull, 1024ull, 4096ull})
        for (int cus : cus_of)
            for (int bpc : {1, 2, 4, 8, 1 << 20}) {
                const uint64_t cap = (uint64_t)cus * bpc, full = cap * per_pass;
                const uint64_t units[] = {0, 1, per_pass - 1, per_pass, per_pass + 1, full - 1, full, full + 1,
                                          1ull << 31, 1ull << 40, 1ull << 62};
                for (uint64_t u : units) {   // not sorted: monotonicity is checked against every smaller one
                    const unsigned g = mi355k::streaming_grid(u, per_pass, cus, bpc);
                    ++cases;
                    digest_u64(g, 4);
                    require(g >= 1 && g <= cap, "streaming range", u, per_pass, cus, bpc, g);
                    const uint64_t cover = (u + per_pass - 1) / per_pass;
                    require(g == (cover < 1 ? 1 : cover < cap ? cover : cap), "streaming rule", u, per_pass, cus, bpc, g);
                    for (uint64_t v : units)
                        if (v <= u)
                            require(mi355k::streaming_grid(v, per_pass, cus, bpc) <= g, "streaming monotone", u, v, cus,
                                    bpc, g);
                }
            }
    for (int occ = 0; occ <= 10; ++occ)
        for (int cus : cus_of)
            for (int share : {-1, 0, 1, 2, 3, 8, 9, 16, 64}) {
                const int n = occ < MI355_FUSED_RESIDENT_PER_CU ? occ : MI355_FUSED_RESIDENT_PER_CU;
                const uint64_t per_cu = n - 1 > 1 ? n - 1 : 1;
                uint64_t cap = per_cu * (uint64_t)cus / (uint64_t)(share > 1 ? share : 1);
                if (cap < 1) cap = 1;
                const uint64_t wants[] = {0, 1, 2, 5, 255, 256, 257, cap - 1, cap, cap + 1, 1000000, 1ull << 40};
                for (uint64_t w : wants) {
                    const unsigned g = mi355k::coresident_cap(occ, cus, share, w);
                    ++cases;
                    digest_u64(g, 4);
                    require(g >= 1 && g <= cap, "co-residency range", occ, cus, (uint64_t)(int64_t)share, w, g);
                    require(g == (w < 1 ? 1 : w < cap ? w : cap), "co-residency rule", occ, cus, (uint64_t)(int64_t)share,
                            w, g);
                    for (uint64_t v : wants)
                        if (v <= w)
                            require(mi355k::coresident_cap(occ, cus, share, v) <= g, "co-residency monotone", occ, cus,
                                    w, v, g);
                }
            }
    printf("%ld cases, digest %016llx, %ld violations\n", cases, (unsigned long long)g_digest, bad);
    return bad == 0 ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "capsweep") == 0) return cap_sweep();
    if (argc > 1 && strcmp(argv[1], "caps") == 0) {
        // stream:UNITS:PER_PASS:CUS:BLOCKS_PER_CU | resident:OCCUPANCY:CUS:SHARE:WANT -> the grid
        for (int i = 2; i < argc; ++i) {
            char kind[16];
            long long v[4];
            if (sscanf(argv[i], "%15[a-z]:%lld:%lld:%lld:%lld", kind, &v[0], &v[1], &v[2], &v[3]) != 5) return 2;
            if (strcmp(kind, "stream") == 0)
                printf("%u\n", mi355k::streaming_grid((uint64_t)v[0], (uint64_t)v[1], (int)v[2], (int)v[3]));
            else if (strcmp(kind, "resident") == 0)
                printf("%u\n", mi355k::coresident_cap((int)v[0], (int)v[1], (int)v[2], (uint64_t)v[3]));
            else
                return 2;
        }
        return 0;
    }
    if (argc > 1 && strcmp(argv[1], "plan") == 0) {
        for (int i = 2; i < argc; ++i) {
            std::vector<std::string> f;
            std::string s = argv[i];
            size_t at = 0;
            for (size_t colon; (colon = s.find(':', at)) != std::string::npos; at = colon + 1) f.push_back(s.substr(at, colon - at));
            f.push_back(s.substr(at));
            if (f.size() != 5) return 2;
            const std::vector<uintptr_t> outs = parse_list(f[3]), srcs = parse_list(f[4]);
            if (outs.size() > 8 || srcs.empty() || srcs.size() > 8) return 2;
            const LaunchPlan p = plan_of((size_t)atoi(f[0].c_str()), atoi(f[1].c_str()) != 0, outs, srcs,
                                         (size_t)strtoull(f[2].c_str(), nullptr, 0));
            printf("%s %zu %zu %zu\n", kind_name(p.kind), p.head, p.nvec, p.tail);
        }
        return 0;
    }
    enumerate();
    printf("%ld cases (%ld aligned, %ld shift, %ld elements), digest %016llx, %ld violations\n", g_cases, g_kinds[0],
           g_kinds[1], g_kinds[2], (unsigned long long)g_digest, g_bad);
    return g_bad == 0 ? 0 : 1;
}
