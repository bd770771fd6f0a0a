// rate_walk.hpp - opj_tcd_makelayer's greedy walk over the coding passes of one code-block, the thresholds at which a
// walk is "the" walk, and the per-code-block table of all of them (j2k_rate.hip: k_rate_tables builds it once per
// analysed frame, k_rate looks its layers up in it).  Compiles for the device and for the host: the CPU test
// tests/rate_walk_host_check.cpp runs these very functions.
//
// `Tab` is a view of one frame's pass tables:
//   int passes(int b)            coding passes of code-block b
//   int base_of(int b)           where its entries start
//   int rate(int base, int p)    bytes up to and including pass p
//   double dist(int base, int p) distortion decrease up to and including pass p
#pragma once
#include <cfloat>

#if defined(__HIPCC__)
#define EBCC_RW_HD __host__ __device__
#else
#define EBCC_RW_HD
#endif

namespace ebcc {

// opj_tcd_makelayer's greedy walk over the passes of code-block b: passes taken (count returned, bit mask in m0 / m1)
// `from` > 0: the walk is taken up at pass `from` with passes [0, from) decided already - their mask in m0 / m1 on entry,
// the last pass taken among them `n_in` (count, 0: none) - see the tail of k_rate's bisection
template <class Tab>
EBCC_RW_HD inline int walk_block(const Tab &pt, int b, double thresh, unsigned long long &m0, unsigned long long &m1, int from = 0,
                                 int n_in = 0)
{
    if (from == 0) m0 = m1 = 0;
    const int tp = pt.passes(b);
    const int base = pt.base_of(b);
    int n = n_in;
    if (thresh < 0) return tp;
    int rbase = 0;                                                   // rate / distortion of the last pass taken
    double dbase = 0;
    if (n_in > 0) { rbase = pt.rate(base, n_in - 1); dbase = pt.dist(base, n_in - 1); }
    for (int p = from; p < tp; p++) {
        const int rp = pt.rate(base, p);
        const double dp = pt.dist(base, p);
        unsigned int dr;
        double dd;
        if (n == 0) { dr = (unsigned int) rp; dd = dp; }
        else { dr = (unsigned int) (rp - rbase); dd = dp - dbase; }
        // OpenJPEG's test is  thresh - fl(dd / dr) < DBL_EPSILON.  The outcome is already certain whenever dd and
        // thresh * dr differ by more than rounding can bridge (1e-11 relative, against 2^-52 per operation); only the
        // narrow band in between is divided.  (The reject shortcut also needs DBL_EPSILON to be negligible next to
        // thresh.)
        bool take;
        if (!dr) take = dd != 0;
        else {
            const double tdr = thresh * (double) dr;
            if (dd >= tdr * 1.00000000001) take = true;
            else if (thresh >= 1e-4 && dd <= tdr * 0.99999999999) take = false;
            else take = thresh - (dd / dr) < DBL_EPSILON;
        }
        if (take) {
            n = p + 1; rbase = rp; dbase = dp;
            if (p < 64) m0 |= 1ull << p; else m1 |= 1ull << (p - 64);
        }
    }
    return n;
}

// The thresholds at which a given greedy walk IS the walk: a pass with slope s = fl(dd / dr) is taken iff fl(thresh - s) <
// DBL_EPSILON, which holds up to a limit T(s) and fails from it on (the difference is monotone in thresh).  So the walk
// that takes exactly the passes of (m0, m1) from pass `from` on (the passes below it are given: last one taken n_in) is
// the walk at thresh iff A <= thresh < B, with B the smallest limit of a pass it takes and A the largest limit of a pass
// it leaves - two numbers per walk instead of a walk per threshold.
EBCC_RW_HD inline double next_up(double x)       // the next double above a finite x
{
    if (x == 0.0) { const long long one = 1; double r; __builtin_memcpy(&r, &one, 8); return r; }
    long long u;
    __builtin_memcpy(&u, &x, 8);
    u += x > 0.0 ? 1 : -1;
    double r;
    __builtin_memcpy(&r, &u, 8);
    return r;
}
EBCC_RW_HD inline double next_down(double x) { return -next_up(-x); }
EBCC_RW_HD inline double take_limit(double s)
{
    double t = s + DBL_EPSILON;                                        // close to the limit; settle on it exactly
    for (int k = 0; k < 8 && (t - s) < DBL_EPSILON; k++) t = next_up(t);
    for (int k = 0; k < 8; k++) { const double d = next_down(t); if ((d - s) < DBL_EPSILON) break; t = d; }
    return t;
}
// [tlo, thi]: the bracket the thresholds to come lie in.  A pass whose slope is clearly outside it (by 1e-9 relative; only
// used when the bracket is far above DBL_EPSILON) either does not constrain them at all or rules the walk out for all of
// them - its exact limit is not needed, nor the division that gives its slope.  tlo = 0: the exact interval.
template <class Tab>
EBCC_RW_HD inline void walk_interval(const Tab &pt, int b, unsigned long long m0, unsigned long long m1, int from, int n_in, double tlo,
                                     double thi, double &A, double &B)
{
    const int tp = pt.passes(b);
    const int base = pt.base_of(b);
    int n = n_in, rbase = 0;
    double dbase = 0;
    if (n_in > 0) { rbase = pt.rate(base, n_in - 1); dbase = pt.dist(base, n_in - 1); }
    A = -DBL_MAX; B = DBL_MAX;
    const bool coarse = tlo >= 1e-4;
    for (int p = from; p < tp; p++) {
        const int rp = pt.rate(base, p);
        const double dp = pt.dist(base, p);
        const unsigned int dr = n == 0 ? (unsigned int) rp : (unsigned int) (rp - rbase);
        const double dd = n == 0 ? dp : dp - dbase;
        const bool taken = p < 64 ? (m0 >> p) & 1ull : (m1 >> (p - 64)) & 1ull;
        if (dr) {
            const double fdr = (double) dr;
            if (coarse && dd > thi * fdr * 1.000000001) {                // limit above every threshold to come
                if (!taken) A = DBL_MAX;
            } else if (coarse && dd < tlo * fdr * 0.999999999) {         // limit below every threshold to come
                if (taken) B = -DBL_MAX;
            } else {
                const double lim = take_limit(dd / fdr);
                if (taken) B = lim < B ? lim : B; else A = lim > A ? lim : A;
            }
        } else if (taken != (dd != 0)) { A = DBL_MAX; B = -DBL_MAX; }    // (cannot happen for a walk that was walked: never matches)
        if (taken) { n = p + 1; rbase = rp; dbase = dp; }
    }
}

// ------------------------------------------------------------------------------------------------
// Walk table of a code-block.  Over the threshold axis the walk is piecewise constant: there are limits
// A_0 > A_1 > ... such that the walk at t is walk i exactly when A_i <= t < A_(i-1) (A_(-1) = +inf).  The table keeps
// the limits and, per walk, what a layer needs of it: its number of passes.  It depends on the code-block's pass
// tables alone, so it is built once and every rate allocation of the frame - every search, every probe - reads it.
// ------------------------------------------------------------------------------------------------

// walk_block at `thresh` (passes taken: the count returned, their mask in m0 / m1) and, in the same pass over the
// code-block, the lower end A of that walk's exact interval - walk_interval's A with tlo = 0: the largest limit of a pass
// the walk leaves (-DBL_MAX: it leaves none that a lower threshold would take) - with `first`, the first pass that has it.
// `known` > 0: the outcomes of passes [0, known) are given in m0 / m1 and not tested.
// Only the largest limit is wanted, so the pass left with the largest slope so far is carried as a fraction and compared
// by cross-multiplication: a pass clearly below it (by 1e-9 relative, which covers the roundings of both slopes and the
// DBL_EPSILON of take_limit as long as the largest slope is 1e-4 or more) is passed over, one clearly above it takes its
// place, and only what is too close to tell, or too small, is divided on the spot.  One division per walk instead of one
// per pass - and that one by all lanes of a wave together.
template <class Tab>
EBCC_RW_HD inline int walk_and_limit(const Tab &pt, int b, double thresh, unsigned long long &m0, unsigned long long &m1, int known,
                                     double &A, int &first)
{
    const int tp = pt.passes(b);
    const int base = pt.base_of(b);
    int n = 0, rbase = 0;
    double dbase = 0;
    double bd = 0, br = 0;                                           // the largest slope of a pass left, bd / br (br == 0: none yet)
    first = -1;
    if (known == 0) m0 = m1 = 0;
    for (int p = 0; p < tp; p++) {
        const int rp = pt.rate(base, p);
        const double dp = pt.dist(base, p);
        unsigned int dr;
        double dd;
        if (n == 0) { dr = (unsigned int) rp; dd = dp; }
        else { dr = (unsigned int) (rp - rbase); dd = dp - dbase; }
        bool take;
        if (p < known) take = p < 64 ? (m0 >> p) & 1ull : (m1 >> (p - 64)) & 1ull;
        else if (!dr) take = dd != 0;                                // (walk_block's test)
        else {
            const double tdr = thresh * (double) dr;
            if (dd >= tdr * 1.00000000001) take = true;
            else if (thresh >= 1e-4 && dd <= tdr * 0.99999999999) take = false;
            else take = thresh - (dd / dr) < DBL_EPSILON;
        }
        if (take) {
            n = p + 1; rbase = rp; dbase = dp;
            if (p < 64) m0 |= 1ull << p; else m1 |= 1ull << (p - 64);
            continue;
        }
        if (!dr) continue;                                           // (left whatever the threshold)
        const double fdr = (double) dr;
        if (br == 0) { bd = dd; br = fdr; first = p; continue; }
        if (bd >= 1e-4 * br) {
            const double l = dd * br, r = bd * fdr;
            if (l < r * 0.999999999) continue;
            if (l > r * 1.000000001) { bd = dd; br = fdr; first = p; continue; }
        }
        if (take_limit(dd / fdr) > take_limit(bd / br)) { bd = dd; br = fdr; first = p; }
    }
    A = br != 0 ? take_limit(bd / br) : -DBL_MAX;
    return n;
}

// Fills lim[] / np[] (at most max_n entries; a code-block of tp passes has at most tp + 1 walks) and returns the number
// written: the walk above every slope, then the walk just below each walk's lower end.  The table then answers every
// threshold >= lim[count - 1]; it ends at a limit <= 0, below which no bisection goes, or early - at max_n, or where a
// limit does not lie below the threshold it was made for - and then the thresholds below its end are left to
// walk_block (walk_table_find returns -1 for them).
// From one walk to the next, at next_down(A): the passes before `first` that were left have limits below A and stay left,
// the ones taken have limits above it and stay taken, what they are measured against has not changed, and `first`
// itself is taken now - so the test starts behind it (and does not land in the band that has to be divided at every
// step: the threshold is a hair below that very pass's limit).
template <class Tab>
EBCC_RW_HD inline int walk_table_build(const Tab &pt, int b, double *lim, unsigned char *np, int max_n)
{
    double t = DBL_MAX;                                              // above every slope
    int count = 0, known = 0;
    unsigned long long m0 = 0, m1 = 0;
    while (count < max_n) {
        double A;
        int first;
        const int n = walk_and_limit(pt, b, t, m0, m1, known, A, first);
        if (!(A <= t)) break;
        lim[count] = A; np[count] = (unsigned char) n;
        count++;
        if (A <= 0) break;                                           // (-DBL_MAX: the walk leaves no pass)
        t = next_down(A);
        m0 = first >= 64 ? m0 : m0 & ((1ull << first) - 1ull);
        m1 = first > 64 ? m1 & ((1ull << (first - 64)) - 1ull) : 0ull;
        if (first < 64) m0 |= 1ull << first; else m1 |= 1ull << (first - 64);
        known = first + 1;
    }
    return count;
}

// The walk of threshold t >= 0: the first entry with lim <= t, looked for in [a, z] - a: an entry known to be at or
// above t's, z: one known to be at or below it (0 and count - 1 when nothing is known).  -1: t is below the table.
EBCC_RW_HD inline int walk_table_find(const double *lim, int a, int z, double t)
{
    if (z < a) return -1;
    while (a < z) {
        const int m = (a + z) >> 1;
        if (lim[m] <= t) z = m; else a = m + 1;
    }
    return lim[a] <= t ? a : -1;
}

}  // namespace ebcc
