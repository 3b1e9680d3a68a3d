/* Stand-alone check of cueball_amd/_native/lathist.h, built with
 * -fsanitize=address,undefined by tests/test_lathist_native.py.
 * Includes nothing of the project but the header; exits 0 when every
 * check holds, 1 (after naming the failed checks) otherwise. */

#include <cmath>
#include <cstdio>
#include <limits>

#include "lathist.h"

static int failures = 0;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__,     \
                         __LINE__, #cond);                            \
            failures++;                                               \
        }                                                             \
    } while (0)

using lathist::Hist;
using lathist::index_us;
using lathist::lower_bound;
using lathist::to_us;

/* index of the single occupied bucket, -1 unless exactly one sample */
static int
only_bucket(const Hist &h)
{
    int found = -1;
    uint64_t total = 0;
    for (int i = 0; i < lathist::NBUCKETS; i++) {
        total += h.counts[i];
        if (h.counts[i] != 0)
            found = i;
    }
    return total == 1 ? found : -1;
}

static int
bucket_of_ms(double ms)
{
    Hist *h = new Hist();
    h->reset();
    h->record_ms(ms);
    int idx = only_bucket(*h);
    delete h;
    return idx;
}

int
main()
{
    CHECK(lathist::REGULAR == 272);
    CHECK(lathist::NBUCKETS == 273);
    const uint64_t LIM = (uint64_t)1 << 36;

    /* round trip over every regular bucket, through record_ms too */
    Hist *all = new Hist();
    all->reset();
    for (int i = 0; i < lathist::REGULAR; i++) {
        uint64_t lo = lower_bound(i), hi = lower_bound(i + 1);
        CHECK(lo < hi);
        CHECK(index_us(lo) == i);
        CHECK(index_us(hi - 1) == i);
        if (i >= 16)
            CHECK((hi - lo) * 8 <= lo);
        all->record_ms((double)lo / 1000.0);
        all->record_ms((double)(hi - 1) / 1000.0);
    }
    CHECK(lower_bound(lathist::REGULAR) == LIM);
    for (int i = 0; i < lathist::REGULAR; i++)
        CHECK(all->counts[i] == 2);
    CHECK(all->counts[lathist::OVERFLOW_IDX] == 0);
    CHECK(all->count == 2 * 272);
    CHECK(all->min_us == 0);
    CHECK(all->max_us == LIM - 1);
    CHECK(all->percentile_us(1.0) == LIM - 1);
    delete all;

    /* spot values */
    static const struct { uint64_t us; int idx; } spots[] = {
        {0, 0}, {1, 1}, {15, 15}, {16, 16}, {17, 16}, {30, 23},
        {31, 23}, {32, 24}, {LIM - 1, 271}, {LIM, 272},
    };
    for (const auto &s : spots) {
        CHECK(index_us(s.us) == s.idx);
        CHECK(bucket_of_ms((double)s.us / 1000.0) == s.idx);
    }

    /* negative, overflow, non-finite */
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(to_us(-5.0) == 0);
    CHECK(bucket_of_ms(-5.0) == 0);
    CHECK(bucket_of_ms(-1e300) == 0);
    CHECK(bucket_of_ms(nan) == lathist::OVERFLOW_IDX);
    CHECK(bucket_of_ms(inf) == lathist::OVERFLOW_IDX);
    CHECK(bucket_of_ms(-inf) == lathist::OVERFLOW_IDX);
    CHECK(bucket_of_ms(1e300) == lathist::OVERFLOW_IDX);
    CHECK(bucket_of_ms((double)LIM / 1000.0) == lathist::OVERFLOW_IDX);
    CHECK(to_us(nan) == LIM);
    CHECK(to_us(1e300) == LIM);

    /* rounding, not truncation */
    CHECK(to_us(1000000003.0 - 1000000000.0) == 3000);
    CHECK(to_us((1000000.003 - 1000000.0) * 1000.0) == 3000);
    CHECK(to_us(0.000375) == 0);                /* 0.375 us, exact */
    CHECK(to_us(0.000625) == 1);                /* 0.625 us */
    CHECK(to_us(-1e306) == 0);                  /* x overflows to -inf */
    CHECK(to_us(1e306) == LIM);                 /* x overflows to +inf */
    CHECK(to_us(2.9996) == 3000);

    /* percentile walk */
    Hist *h = new Hist();
    h->reset();
    CHECK(h->count == 0);
    h->record_ms(3.3);
    CHECK(h->percentile_us(0.0) == 3300);
    CHECK(h->percentile_us(0.5) == 3300);
    CHECK(h->percentile_us(1.0) == 3300);
    h->reset();
    for (int ms = 1; ms <= 100; ms++)
        h->record_ms((double)ms);
    CHECK(h->count == 100);
    CHECK(h->sum_us == 5050000);
    CHECK(h->min_us == 1000 && h->max_us == 100000);
    CHECK(h->percentile_us(1.0) == 100000);
    CHECK(h->percentile_us(0.5) == lower_bound(index_us(50000) + 1));
    CHECK(h->percentile_us(0.9) == lower_bound(index_us(90000) + 1));
    CHECK(h->percentile_us(0.99) == 100000);  /* edge clamped to max */
    CHECK(h->percentile_us(0.01) == lower_bound(index_us(1000) + 1));
    CHECK(h->percentile_us(nan) == h->percentile_us(0.0));
    CHECK(h->percentile_us(7.0) == 100000);
    CHECK(h->cumulative_below(index_us(16384)) == 16);
    CHECK(h->cumulative_below(lathist::NBUCKETS + 5) == 100);

    /* overflow samples saturate and end the walk at max */
    h->record_ms(nan);
    CHECK(h->count == 101);
    CHECK(h->max_us == LIM);
    CHECK(h->percentile_us(1.0) == LIM);
    CHECK(h->percentile_us(0.5) == lower_bound(index_us(51000) + 1));

    /* merge of two halves == the whole */
    Hist *a = new Hist(), *b = new Hist(), *w = new Hist();
    a->reset(); b->reset(); w->reset();
    uint64_t x = 88172645463325252ULL;          /* xorshift64 */
    for (int i = 0; i < 4000; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        double ms = std::ldexp((double)(x >> 11), -53 + (int)(x % 37) - 10);
        w->record_ms(ms);
        (i % 2 ? a : b)->record_ms(ms);
    }
    a->merge(*b);
    for (int i = 0; i < lathist::NBUCKETS; i++)
        CHECK(a->counts[i] == w->counts[i]);
    CHECK(a->count == w->count && a->sum_us == w->sum_us);
    CHECK(a->min_us == w->min_us && a->max_us == w->max_us);
    CHECK(a->percentile_us(0.99) == w->percentile_us(0.99));
    b->reset();
    a->merge(*b);                               /* empty: no change */
    CHECK(a->count == w->count && a->min_us == w->min_us);
    b->merge(*w);                               /* into empty: copy */
    CHECK(b->count == w->count && b->min_us == w->min_us &&
          b->max_us == w->max_us);
    delete a; delete b; delete w; delete h;

    if (failures != 0) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("lathist ok");
    return 0;
}
