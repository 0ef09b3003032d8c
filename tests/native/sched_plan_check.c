/* sched_plan_check.c -- osss-gasnet_amd/csrc/sched_plan.h on the CPU
 * (tests/test_sched_plan.py builds it with gcc -fsanitize=address,undefined).
 *
 *   sched_plan_check                  plans every request of the enumeration
 *                                     below, holds each plan to the invariants
 *                                     and prints the case count, the violations
 *                                     and an FNV-1a digest of all the plans
 *   sched_plan_check plan ARG...      one line per request. NAME=VALUE sets a
 *                                     field of the job's settings for the
 *                                     requests after it; a request is
 *                                     COLL:ENTRY:OP:TYPE:SIZE:ME:DST:SRC:N
 *                                     (offsets in bytes, N in elements) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sched_plan.h"

static const char *const op_names[MI355_NUM_OPS] = {"sum", "prod", "and", "or", "xor", "min", "max"};
static const struct { const char *name; size_t es; } types[MI355_NUM_DTYPES] = {
    {"short", 2}, {"int", 4}, {"long", 8}, {"longlong", 8}, {"float", 4}, {"double", 8},
    {"longdouble", 16}, {"complexf", 8}, {"complexd", 16}, {"half", 2}, {"bfloat16", 2}};
static const char *const legs_names[] = {"FOLD", "ORDERS", "PAIR", "INSCAN", "EXSCAN"};
static const char *const sync_names[] = {"HOST", "DEV", "STREAM"};
static const char *const err_names[] = {"ok", "order-area", "p2p-broken", "stream-members", "stream-peers",
                                        "stream-overlap", "stream-order"};

/* the 52 pairs of *_to_all (and of each scan): sum and prod of every type,
 * the bitwise operators of the integers, min and max of all but complex */
static int supported (int op, int dtype)
{
    if (op == MI355_OP_SUM || op == MI355_OP_PROD)
        return 1;
    if (op == MI355_OP_AND || op == MI355_OP_OR || op == MI355_OP_XOR)
        return dtype <= MI355_LONGLONG;
    return dtype != MI355_COMPLEXF && dtype != MI355_COMPLEXD;
}

static int is_float (int dtype) { return dtype >= MI355_FLOAT; }

static int is_shards (enum sched_id s)
{
    return (s >= SCHED_P2P && s <= SCHED_P2P_HOST_ROUNDS) || s == SCHED_STREAM_P2P || s == SCHED_STREAM_P2P_ROUNDS ||
           (s >= SCHED_SCAN_P2P && s <= SCHED_SCAN_P2P_HOST_ROUNDS);
}

static int is_fused (enum sched_id s)
{
    return s == SCHED_FUSED_ONESHOT || s == SCHED_FUSED_TWOSHOT || s == SCHED_STREAM_FUSED_ONESHOT ||
           s == SCHED_STREAM_FUSED_TWOSHOT;
}

static long long cases, violations;
static uint64_t digest = 0xcbf29ce484222325ull;

static void mix (uint64_t v)
{
    for (int i = 0; i < 8; ++i) {
        digest ^= (v >> (8 * i)) & 0xff;
        digest *= 0x100000001b3ull;
    }
}

static void print_plan (const struct sched_plan *p)
{
    if (p->err != SCHED_OK) {
        printf ("error %s\n", err_names[p->err]);
        return;
    }
    printf ("%s", sched_name (p->sched));
    if (is_shards (p->sched))
        printf (" %s %s round=%zu", legs_names[p->legs], sync_names[p->sync], p->round);
    printf ("%s%s%s%s", p->ordered ? " ordered" : "", p->oneshot ? " oneshot" : "", p->noop ? " noop" : "",
            p->servable ? " servable" : "");
    if (p->via_scratch)
        printf (" scratch-%s chunk=%zu", p->down ? "down" : "up", p->chunk_elems);
    printf ("%s\n", p->receives ? "" : " no-target");
}

static void fail (const char *what, const struct sched_env *e, const struct sched_req *r, const struct sched_plan *p)
{
    if (violations++ < 20) {
        fprintf (stderr, "violation: %s: coll %d entry %d %s %s size %d me %d dst %zu src %zu n %zu; order %d alg %d "
                         "fused_max %zu oneshot_max %zu order_chunk %zu npes %d flags %d%d%d%d%d%d: ",
                 what, r->coll, r->entry, op_names[r->op], types[r->dtype].name, r->size, r->me, r->dst_off, r->src_off,
                 r->n, e->order, e->algorithm, e->fused_max, e->oneshot_max, e->order_chunk, e->npes, e->have_sigmem,
                 e->sig_broken, e->dev_wait_slow, e->p2p_broken, e->persistent, e->scan_direct);
        fflush (stderr);
        print_plan (p);
    }
}

static void check (const struct sched_env *e, const struct sched_req *r)
{
    const struct sched_plan p = plan_schedule (e, r);
    const size_t nbytes = r->n * r->es;
    const int same = r->dst_off == r->src_off;
    const int partial = !same && ranges_overlap (r->dst_off, r->src_off, nbytes);
    ++cases;
    mix (p.err), mix (p.sched), mix (p.legs), mix (p.sync), mix (p.ordered), mix (p.oneshot), mix (p.round);
    mix (p.noop), mix (p.servable), mix (p.receives), mix (p.via_scratch), mix (p.down), mix (p.chunk_elems);
#define REQUIRE(cond, what) do { if (!(cond)) fail (what, e, r, &p); } while (0)
    REQUIRE ((p.err != SCHED_OK) == (p.sched == SCHED_NONE), "an error names no schedule, a plan names one");
    if (p.err != SCHED_OK) {
        REQUIRE (!p.ordered && !p.oneshot && !p.round && !p.via_scratch && !p.servable, "an error carries a plan");
        return;
    }
    REQUIRE (!p.ordered || r->size <= MI355_ORDERS_MAX_SOURCES, "ordered beyond MI355_ORDERS_MAX_SOURCES");
    REQUIRE (!p.ordered || r->size > 1, "ordered with one member");
    if (is_fused (p.sched)) {
        REQUIRE (((r->dst_off | r->src_off) & 15) == 0, "fused off 16-byte alignment");
        REQUIRE (fused_dtype (r->dtype), "fused 16-bit type");
        REQUIRE (nbytes <= e->fused_max, "fused above fused_max");
        REQUIRE (!partial && !p.via_scratch, "fused with partial overlap");
        REQUIRE (r->size > 1 && r->size <= MI355_FUSED_MAX_MEMBERS && e->have_sigmem, "fused set");
        REQUIRE (p.oneshot == (p.sched == SCHED_FUSED_ONESHOT || p.sched == SCHED_STREAM_FUSED_ONESHOT),
                 "one-shot flag and name");
        REQUIRE (r->entry == ENTRY_STREAM || e->algorithm != SHMEMX_REDUCE_EXACT, "fused under EXACT");
    }
    REQUIRE (r->dtype != MI355_HALF && r->dtype != MI355_BFLOAT16 ? 1 : !is_fused (p.sched) && !p.servable,
             "16-bit type on the fused path");
    REQUIRE (!p.oneshot || (!same && nbytes <= e->oneshot_max), "one-shot in place or above oneshot_max");
    REQUIRE (!p.oneshot || is_fused (p.sched) || p.servable, "one-shot outside the fused path");
    REQUIRE (!p.servable || (e->persistent && r->entry == ENTRY_BLOCKING && r->in_heap), "servable");
    if (r->entry == ENTRY_STREAM) {
        REQUIRE (!is_shards (p.sched) || p.sync == SYNC_STREAM, "a stream plan's sync");
        REQUIRE (!p.via_scratch, "a stream plan through scratch");
        REQUIRE (p.sched == SCHED_BARRIER_ONLY || (p.sched >= SCHED_STREAM_IDENTITY && p.sched <= SCHED_STREAM_P2P_ROUNDS),
                 "a stream plan's name");
    } else {
        REQUIRE (!is_shards (p.sched) || p.sync != SYNC_STREAM, "a blocking plan's sync");
        REQUIRE (!(p.sched >= SCHED_STREAM_IDENTITY && p.sched <= SCHED_STREAM_P2P_ROUNDS), "a blocking plan's name");
    }
    if (is_shards (p.sched)) {
        const size_t align = r->es >= 256 ? 1 : 256 / r->es;
        REQUIRE (p.round > 0, "round size");
        REQUIRE (!p.ordered || p.round % ((size_t) r->size * align) == 0, "ordered round size");
        REQUIRE (p.ordered || p.via_scratch || p.round == r->n, "an order-free plan in rounds");
        REQUIRE (p.via_scratch || (r->n > p.round) == (p.sched == SCHED_P2P_ROUNDS || p.sched == SCHED_P2P_HOST_ROUNDS ||
                                                        p.sched == SCHED_STREAM_P2P_ROUNDS ||
                                                        p.sched == SCHED_SCAN_P2P_ROUNDS ||
                                                        p.sched == SCHED_SCAN_P2P_HOST_ROUNDS), "rounds and name");
        REQUIRE (p.ordered == (p.legs != LEGS_FOLD && p.legs != LEGS_PAIR), "ordered and legs");
        REQUIRE (p.legs != LEGS_PAIR || (r->size == 2 && (r->dtype == MI355_FLOAT || r->dtype == MI355_DOUBLE) &&
                                         (r->op == MI355_OP_SUM || r->op == MI355_OP_PROD) &&
                                         e->order == SHMEMX_ORDER_REFERENCE && r->coll == COLL_REDUCE), "LEGS_PAIR");
        REQUIRE ((p.legs >= LEGS_INSCAN) == (r->coll != COLL_REDUCE), "scan legs");
        REQUIRE (p.sync != SYNC_DEV || (!e->sig_broken && !e->dev_wait_slow && e->have_sigmem), "device barriers");
        REQUIRE (r->size > 1, "shards of one member");
    }
    REQUIRE (!(p.ordered && r->coll == COLL_REDUCE) || (is_float (r->dtype) && e->order == SHMEMX_ORDER_REFERENCE),
             "ordered integers or pe_start order");
    REQUIRE (p.sched != SCHED_EXACT || (r->coll == COLL_REDUCE && r->entry == ENTRY_BLOCKING &&
                                        (r->size > 1 || (p.via_scratch && e->algorithm == SHMEMX_REDUCE_EXACT))),
             "EXACT");
    REQUIRE (p.sched != SCHED_SCAN_DIRECT || (r->size > MI355_ORDERS_MAX_SOURCES || e->scan_direct), "direct scan");
    REQUIRE (r->size == 1 || !e->p2p_broken || r->n == 0, "peer reads planned although broken");
    REQUIRE (!p.via_scratch || partial || (same && (r->coll != COLL_REDUCE || p.sched == SCHED_EXACT)),
             "scratch without an overlap");
    REQUIRE (!partial || p.via_scratch || p.noop, "a partial overlap not through scratch");
    REQUIRE (!p.via_scratch || (p.chunk_elems > 0 && p.down == (r->dst_off > r->src_off)), "scratch walk");
    REQUIRE (!p.noop || r->size == 1, "noop");
    REQUIRE (p.receives == !(r->coll == COLL_EXSCAN && r->me == 0), "receives");
    REQUIRE ((r->n == 0) == (p.sched == SCHED_BARRIER_ONLY), "barrier-only");
#undef REQUIRE
}

static struct sched_env base_env (void)
{
    struct sched_env e;
    memset (&e, 0, sizeof e);
    e.order = SHMEMX_ORDER_REFERENCE;
    e.algorithm = SHMEMX_REDUCE_AUTO;
    e.fused_max = (size_t) 2 << 20;
    e.oneshot_max = (size_t) 64 << 10;
    e.order_chunk = (size_t) 256 << 20;
    e.scratch_chunk = (size_t) 256 << 20;
    e.npes = 64;
    e.have_sigmem = 1;
    return e;
}

/* every request against one env */
static void enumerate_requests (const struct sched_env *e)
{
    static const int sizes[] = {1, 2, 3, 5, 8, 9, 16, 17, 33};
    const size_t base = (size_t) 1 << 20, far = (size_t) 1 << 36;
    for (int coll = COLL_REDUCE; coll <= COLL_EXSCAN; ++coll)
        for (int entry = ENTRY_BLOCKING; entry <= (coll == COLL_REDUCE ? ENTRY_STREAM : ENTRY_BLOCKING); ++entry)
            for (int op = 0; op < MI355_NUM_OPS; ++op)
                for (int dtype = 0; dtype < MI355_NUM_DTYPES; ++dtype) {
                    if (!supported (op, dtype))
                        continue;
                    const size_t es = types[dtype].es, align = 256 / es;
                    for (unsigned si = 0; si < sizeof sizes / sizeof sizes[0]; ++si) {
                        const int size = sizes[si];
                        /* n on both sides of every boundary of the plan */
                        size_t ns[24];
                        int nn = 0;
                        ns[nn++] = 0, ns[nn++] = 1, ns[nn++] = 2; /* one shard empty */
                        ns[nn++] = size > 1 ? (size_t) size - 1 : 1, ns[nn++] = (size_t) size;
                        ns[nn++] = size > 1 ? align * (size_t) (size - 1) : 1; /* the last shard empty */
                        ns[nn++] = align * (size_t) (size - 1) + 1;
                        if (e->oneshot_max)
                            ns[nn++] = e->oneshot_max / es, ns[nn++] = e->oneshot_max / es + 1;
                        if (e->fused_max)
                            ns[nn++] = e->fused_max / es, ns[nn++] = e->fused_max / es + 1;
                        if (size > 1) {
                            const size_t round = ordered_round_elems (e, es, size);
                            if (round)
                                ns[nn++] = round, ns[nn++] = round + 1;
                            /* the largest n whose versions fit the version area, for the fused kernel */
                            const size_t fit = e->order_chunk / ((size_t) (size - 1) * es) / align * align * (size_t) size;
                            if (fit)
                                ns[nn++] = fit, ns[nn++] = fit + 1;
                        }
                        ns[nn++] = e->scratch_chunk / es, ns[nn++] = e->scratch_chunk / es + 1; /* one chunk, two */
                        for (int me = 0; me < size; me += size - 1 ? size - 1 : 1) {
                            if (me && coll != COLL_EXSCAN)
                                break; /* only exscan's member 0 differs */
                            for (int k = 0; k < nn; ++k)
                                for (int where = 0; where < 5; ++where) {
                                    struct sched_req r;
                                    memset (&r, 0, sizeof r);
                                    r.coll = (enum sched_coll) coll;
                                    r.entry = (enum sched_entry) entry;
                                    r.op = op, r.dtype = dtype, r.es = es;
                                    r.n = ns[k], r.size = size, r.me = me;
                                    r.in_heap = 1;
                                    r.src_off = base;
                                    r.dst_off = where == 0   ? base           /* in place */
                                                : where == 1 ? base + far     /* disjoint */
                                                : where == 2 ? base + far + es /* disjoint, one element off (16 bytes for some) */
                                                : where == 3 ? base + es * (r.n > 4 ? r.n / 2 : 1) /* overlapping from above */
                                                             : base - es;     /* overlapping from below */
                                    check (e, &r);
                                    if (where == 1 && coll == COLL_REDUCE && entry == ENTRY_BLOCKING) {
                                        r.in_heap = 0; /* staged host buffers, mapped device buffers */
                                        check (e, &r);
                                    }
                                }
                        }
                    }
                }
}

static void enumerate (void)
{
    static const int orders[] = {SHMEMX_ORDER_REFERENCE, SHMEMX_ORDER_PE_START};
    static const int algs[] = {SHMEMX_REDUCE_P2P, SHMEMX_REDUCE_EXACT, SHMEMX_REDUCE_RCCL};
    static const size_t fmax[] = {0, (size_t) 1 << 20, (size_t) 2 << 20}, omax[] = {0, (size_t) 64 << 10};
    static const size_t ochunk[] = {(size_t) 64 << 10, (size_t) 256 << 20};
    for (int o = 0; o < 2; ++o)
        for (int a = 0; a < 3; ++a)
            for (int oc = 0; oc < 2; ++oc) {
                struct sched_env e = base_env ();
                e.order = orders[o], e.algorithm = algs[a], e.order_chunk = ochunk[oc];
                for (int f = 0; f < 3; ++f)
                    for (int s = 0; s < 2; ++s) {
                        e.fused_max = fmax[f], e.oneshot_max = omax[s];
                        enumerate_requests (&e);
                    }
                /* each flag on its own (and a job beyond the signal region's PEs) */
                e.fused_max = fmax[1], e.oneshot_max = omax[1];
                for (int flag = 0; flag < 7; ++flag) {
                    struct sched_env g = e;
                    switch (flag) {
                    case 0: g.have_sigmem = 0; break;
                    case 1: g.sig_broken = 1; break;
                    case 2: g.dev_wait_slow = 1; break;
                    case 3: g.p2p_broken = 1; break;
                    case 4: g.persistent = 1; break;
                    case 5: g.scan_direct = 1; break;
                    default: g.npes = 2048; break;
                    }
                    enumerate_requests (&g);
                }
            }
}

static int lookup (const char *s, const char *const *names, int n)
{
    for (int i = 0; i < n; ++i)
        if (strcmp (s, names[i]) == 0)
            return i;
    fprintf (stderr, "unknown name: %s\n", s);
    exit (2);
}

static int plan_mode (int argc, char **argv)
{
    static const char *const colls[] = {"reduce", "inscan", "exscan"}, *const entries[] = {"blocking", "stream"};
    static const char *const order_names[] = {"reference", "pe_start"}, *const alg_names[] = {"auto", "p2p", "exact", "rccl"};
    struct sched_env e = base_env ();
    for (int i = 0; i < argc; ++i) {
        char buf[256];
        snprintf (buf, sizeof buf, "%s", argv[i]);
        char *eq = strchr (buf, '=');
        if (eq != NULL) {
            *eq++ = '\0';
            const unsigned long long v = strtoull (eq, NULL, 0);
            if (!strcmp (buf, "order")) e.order = lookup (eq, order_names, 2);
            else if (!strcmp (buf, "algorithm")) e.algorithm = lookup (eq, alg_names, 4);
            else if (!strcmp (buf, "fused_max")) e.fused_max = v;
            else if (!strcmp (buf, "oneshot_max")) e.oneshot_max = v;
            else if (!strcmp (buf, "order_chunk")) e.order_chunk = v;
            else if (!strcmp (buf, "scratch_chunk")) e.scratch_chunk = v;
            else if (!strcmp (buf, "npes")) e.npes = (int) v;
            else if (!strcmp (buf, "have_sigmem")) e.have_sigmem = (int) v;
            else if (!strcmp (buf, "sig_broken")) e.sig_broken = (int) v;
            else if (!strcmp (buf, "dev_wait_slow")) e.dev_wait_slow = (int) v;
            else if (!strcmp (buf, "p2p_broken")) e.p2p_broken = (int) v;
            else if (!strcmp (buf, "persistent")) e.persistent = (int) v;
            else if (!strcmp (buf, "scan_direct")) e.scan_direct = (int) v;
            else { fprintf (stderr, "unknown setting: %s\n", buf); return 2; }
            continue;
        }
        char *f[9];
        int nf = 0;
        for (char *t = strtok (buf, ":"); t != NULL && nf < 9; t = strtok (NULL, ":"))
            f[nf++] = t;
        if (nf != 9) { fprintf (stderr, "not COLL:ENTRY:OP:TYPE:SIZE:ME:DST:SRC:N: %s\n", argv[i]); return 2; }
        struct sched_req r;
        memset (&r, 0, sizeof r);
        r.coll = (enum sched_coll) lookup (f[0], colls, 3);
        r.entry = (enum sched_entry) lookup (f[1], entries, 2);
        r.op = lookup (f[2], op_names, MI355_NUM_OPS);
        for (r.dtype = 0; r.dtype < MI355_NUM_DTYPES && strcmp (f[3], types[r.dtype].name); ++r.dtype) {}
        if (r.dtype == MI355_NUM_DTYPES || !supported (r.op, r.dtype)) { fprintf (stderr, "no such pair: %s\n", argv[i]); return 2; }
        r.es = types[r.dtype].es;
        r.size = atoi (f[4]), r.me = atoi (f[5]);
        r.dst_off = strtoull (f[6], NULL, 0), r.src_off = strtoull (f[7], NULL, 0), r.n = strtoull (f[8], NULL, 0);
        r.in_heap = 1;
        if (r.size < 1 || r.me < 0 || r.me >= r.size) { fprintf (stderr, "no such member: %s\n", argv[i]); return 2; }
        const struct sched_plan p = plan_schedule (&e, &r);
        print_plan (&p);
    }
    return 0;
}

int main (int argc, char **argv)
{
    if (argc > 1 && strcmp (argv[1], "plan") == 0)
        return plan_mode (argc - 2, argv + 2);
    enumerate ();
    printf ("%lld cases, %lld violations, digest %016llx, over\n", cases, violations, (unsigned long long) digest);
    return violations != 0;
}
