/* Fixed-layout log-linear latency histogram over integer microseconds.
 *
 * Pure arithmetic, no Python.h: speed.cpp wraps it as
 * _speed.LatencyHistogram and records into it from the claim handle;
 * tests/native/lathist_check.cpp exercises it stand-alone.  The pure
 * twin in cueball_amd/latency.py follows the same integer arithmetic,
 * so both agree exactly.
 *
 * Layout: values 0..15 us get one bucket each; above that every octave
 * [2^e, 2^(e+1)) is cut into 8 equal sub-buckets (a bucket is at most
 * 12.5 % wide).  272 regular buckets cover [0, 2^36) us; one overflow
 * bucket takes everything else (>= 2^36 us, nan, +-inf).  Overflow
 * samples saturate at 2^36 us in sum/min/max, so the integer state
 * stays well defined.
 */
#ifndef CUEBALL_LATHIST_H
#define CUEBALL_LATHIST_H

#include <cmath>
#include <cstdint>
#include <cstring>

namespace lathist {

enum {
    LINEAR = 16,          /* one bucket per us below this */
    SUB_BITS = 3,         /* 8 sub-buckets per octave */
    MAX_BITS = 36,        /* regular range is [0, 2^36) us */
    REGULAR = LINEAR + (MAX_BITS - 4) * 8,   /* 272 */
    OVERFLOW_IDX = REGULAR,
    NBUCKETS = REGULAR + 1                   /* 273 */
};

static const uint64_t LIMIT_US = (uint64_t)1 << MAX_BITS;

/* bucket of an in-range value (us < 2^36) */
static inline int
index_us(uint64_t us)
{
    if (us < LINEAR)
        return (int)us;
    if (us >= LIMIT_US)
        return OVERFLOW_IDX;
    int e = 63 - __builtin_clzll(us);        /* floor(log2(us)) >= 4 */
    return LINEAR + (e - 4) * 8 + (int)((us >> (e - SUB_BITS)) & 7);
}

/* inclusive lower edge of bucket idx; lower_bound(272) == 2^36 is the
 * exclusive upper edge of the last regular bucket */
static inline uint64_t
lower_bound(int idx)
{
    if (idx < LINEAR)
        return (uint64_t)idx;
    int k = idx - LINEAR;
    return (uint64_t)(8 + k % 8) << (k / 8 + 1);
}

/* ms (double) -> us, round to nearest; returns LIMIT_US for anything
 * that belongs in the overflow bucket */
static inline uint64_t
to_us(double ms)
{
    if (!std::isfinite(ms))
        return LIMIT_US;
    double x = ms * 1000.0;
    if (x <= 0.0)
        return 0;
    if (!(x < (double)LIMIT_US))
        return LIMIT_US;
    uint64_t us = (uint64_t)std::llround(x);
    return us >= LIMIT_US ? LIMIT_US : us;
}

struct Hist {
    uint64_t counts[NBUCKETS];
    uint64_t count;
    uint64_t sum_us;
    uint64_t min_us;
    uint64_t max_us;

    void reset()
    {
        std::memset(counts, 0, sizeof(counts));
        count = 0;
        sum_us = 0;
        min_us = 0;
        max_us = 0;
    }

    inline void record_us(uint64_t us)
    {
        if (us > LIMIT_US)
            us = LIMIT_US;
        counts[index_us(us)]++;
        if (count == 0 || us < min_us)
            min_us = us;
        if (us > max_us)
            max_us = us;
        count++;
        sum_us += us;
    }

    inline void record_ms(double ms) { record_us(to_us(ms)); }

    void merge(const Hist &o)
    {
        if (o.count == 0)
            return;
        for (int i = 0; i < NBUCKETS; i++)
            counts[i] += o.counts[i];
        if (count == 0 || o.min_us < min_us)
            min_us = o.min_us;
        if (o.max_us > max_us)
            max_us = o.max_us;
        count += o.count;
        sum_us += o.sum_us;
    }

    /* nearest-rank percentile in us: the exclusive upper edge of the
     * first bucket whose cumulative count reaches ceil(q*count),
     * clamped to the largest sample.  Caller checks count != 0. */
    uint64_t percentile_us(double q) const
    {
        if (!(q > 0.0))
            q = 0.0;
        if (q > 1.0)
            q = 1.0;
        uint64_t rank = (uint64_t)std::ceil(q * (double)count);
        if (rank < 1)
            rank = 1;
        if (rank > count)
            rank = count;
        uint64_t cum = 0;
        for (int i = 0; i < REGULAR; i++) {
            cum += counts[i];
            if (cum >= rank) {
                uint64_t up = lower_bound(i + 1);
                return up < max_us ? up : max_us;
            }
        }
        return max_us;
    }

    /* samples with rounded us value < lower_bound(idx) */
    uint64_t cumulative_below(int idx) const
    {
        uint64_t cum = 0;
        for (int i = 0; i < idx && i < NBUCKETS; i++)
            cum += counts[i];
        return cum;
    }
};

}  /* namespace lathist */

#endif  /* CUEBALL_LATHIST_H */
