// set_order.h -- the CPython set model's rules, once: in which order set(range(m)).difference(used_cols) iterates
// (tracker.py:193,216 registers new tracks in that order).  Ints hash to themselves; table sizes, linear probing
// (LINEAR_PROBES = 9) and perturbation (PERTURB_SHIFT = 5) as in Objects/setobject.c of CPython 3.7-3.12.
// Host and device: track.hip's three drivers (k_link, k_frame, k_batch) parallelise the insertions each in its own way and
// call the step and the rules here; the serial model below is what cpython_unused_order runs on one thread, and what
// tests/set_order_check.cc runs on the host against the interpreter.
// (The shapes below are chosen by what the kernels compile to -- references and not values for the probe's state, a
// functor with the fields of the lambda it replaced, a loop and not the functor in the serial insertion: each alternative
// compiled k_frame, k_batch or k_link to a different listing.  scripts/listing_diff.py shows it.)
#pragma once
#include "hd.h"

// set_copy_and_difference: with few claimed columns the result is a copy of set(range(m)) with keys removed, which
// iterates ascending -- no table to model
YSMR_HD_FORCE bool set_order_is_ascending(int m, int n_used) { return (m >> 2) > n_used; }

// The probe sequence of a key (setobject.c set_insert_clean), from i = key & mask with perturb = key: the slots i .. i + 9
// while that run stays inside the table (else i alone), then the perturbed jump to the next i.
YSMR_HD_FORCE int set_probe_run(const unsigned &i, const unsigned &mask) { return (i + 9u <= mask) ? 9 : 0; }
YSMR_HD_FORCE void set_probe_jump(unsigned &i, unsigned long long &perturb, const unsigned &mask)
{
    perturb >>= 5;
    i = (unsigned)(((unsigned long long)i * 5ull + 1ull + perturb) & mask);
}
// ... as one step of a walk that is at slot i + j (the parallel drivers: a lane keeps its place between rounds), on the
// caller's variables
struct SetProbeStep {
    unsigned &i;
    const unsigned &mask;
    int &j;
    unsigned long long &perturb;
    YSMR_HD_FORCE void operator()() const
    {
        const int probes = set_probe_run(i, mask);
        if (j < probes) ++j;
        else { set_probe_jump(i, perturb, mask); j = 0; }
    }
};

// The growth rule: after an add the table grows once fill * 5 >= mask * 3, i.e. at this fill ...
YSMR_HD_FORCE int set_growth_fill(unsigned mask) { return (int)((3u * mask + 4u) / 5u); }
// ... to the next power of two above four times the fill (twice, above 50 000 keys)
YSMR_HD_FORCE unsigned set_grown_size(int fill)
{
    const unsigned minused = (unsigned)fill > 50000u ? (unsigned)fill * 2u : (unsigned)fill * 4u;
    unsigned newsize = 8;
    while (newsize <= minused) newsize <<= 1;
    return newsize;
}

// ---- the serial model, on the caller's tables (entries < 0: empty) ----------------------------------------------------
YSMR_HD inline void set_insert_clean(int *table, unsigned mask, int key)
{
    unsigned long long perturb = (unsigned long long)key;
    unsigned i = (unsigned)key & mask;
    while (true) {
        int probes = set_probe_run(i, mask);
        for (int j = 0; j <= probes; ++j)
            if (table[i + j] < 0) { table[i + j] = key; return; }
        set_probe_jump(i, perturb, mask);
    }
}

// The order of the ascending list `unused` (the n_unused columns of 0 .. m - 1 that the n_used claims left) into `out`;
// `table` and `other` hold table_cap entries each.  Returns the number of keys, or -1 when the model's table would outgrow
// table_cap.  The insertions are order-dependent: one thread.
YSMR_HD inline int set_unused_order(const int *unused, int m, int n_used, int n_unused, int *out, int *table, int *other,
                                    int table_cap)
{
    if (set_order_is_ascending(m, n_used)) {
        for (int k = 0; k < n_unused; ++k) out[k] = unused[k];
        return n_unused;
    }
    unsigned mask = 7;
    int fill = 0;
    for (int i = 0; i < 8; ++i) table[i] = -1;
    for (int k = 0; k < n_unused; ++k) {
        set_insert_clean(table, mask, unused[k]);  // no equal keys, no dummies: add == insert_clean
        ++fill;
        if (fill >= set_growth_fill(mask)) {
            const unsigned newsize = set_grown_size(fill);
            if ((int)newsize > table_cap) return -1;
            for (unsigned i = 0; i < newsize; ++i) other[i] = -1;
            for (unsigned i = 0; i <= mask; ++i)
                if (table[i] >= 0) set_insert_clean(other, newsize - 1, table[i]);
            int *tmp = table; table = other; other = tmp;
            mask = newsize - 1;
        }
    }
    int count = 0;
    for (unsigned i = 0; i <= mask; ++i)
        if (table[i] >= 0) out[count++] = table[i];
    return count;
}
