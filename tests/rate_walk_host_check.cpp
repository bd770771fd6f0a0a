// CPU check of ebcc_amd/csrc/rate_walk.hpp - the very functions k_rate_tables and k_rate compile for gfx950 - built for
// the host (tests/test_rate_walk_host.py).  For hand-made and random pass tables:
//   1. the walk table's answer equals walk_block's (pass count and pass masks) at random thresholds, at every limit and
//      at the doubles next to it, with the whole table searched and with a bracket;
//   2. a code-block of tp passes never has more than tp + 1 walks, its table ends at a limit <= 0, and every entry's limit
//      is the lower end of its walk's exact interval (walk_interval), whose upper end is the entry before;
//   3. walk_block's form with the 1e-11 accept / reject bands equals the plain  thresh - dd / dr < DBL_EPSILON  form.
// usage: rate_walk_host_check [random tables]; prints "<n> failures".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../ebcc_amd/csrc/rate_walk.hpp"

using namespace ebcc;

struct Tab {
    std::vector<int> r;
    std::vector<double> d;
    int passes(int) const { return (int) r.size(); }
    int base_of(int) const { return 0; }
    int rate(int base, int p) const { return r[(size_t) (base + p)]; }
    double dist(int base, int p) const { return d[(size_t) (base + p)]; }
};

// opj_tcd_makelayer's test as OpenJPEG writes it
static int walk_plain(const Tab &t, double thresh, unsigned long long &m0, unsigned long long &m1)
{
    m0 = m1 = 0;
    const int tp = t.passes(0);
    if (thresh < 0) return tp;
    int n = 0;
    for (int p = 0; p < tp; p++) {
        unsigned int dr;
        double dd;
        if (n == 0) { dr = (unsigned int) t.r[(size_t) p]; dd = t.d[(size_t) p]; }
        else { dr = (unsigned int) (t.r[(size_t) p] - t.r[(size_t) n - 1]); dd = t.d[(size_t) p] - t.d[(size_t) n - 1]; }
        bool take;
        if (!dr) take = dd != 0;
        else take = thresh - (dd / dr) < DBL_EPSILON;
        if (take) {
            n = p + 1;
            if (p < 64) m0 |= 1ull << p; else m1 |= 1ull << (p - 64);
        }
    }
    return n;
}

static long failures = 0, thresholds = 0, tables = 0, walks = 0;
static void fail(const char *what, const Tab &t, double x)
{
    if (++failures <= 20) fprintf(stderr, "FAIL %s: %d passes, threshold %.17g\n", what, t.passes(0), x);
}

static void check_table(const Tab &t, std::mt19937_64 &rng)
{
    const int tp = t.passes(0);
    tables++;
    // (room for more walks than there can be, to count them)
    std::vector<double> lim((size_t) (2 * tp + 8));
    std::vector<unsigned char> np(lim.size());
    const int count = walk_table_build(t, 0, lim.data(), np.data(), (int) lim.size());
    walks += count;
    if (count < 1 || count > tp + 1) { fail("walk count", t, (double) count); return; }
    if (!(lim[(size_t) count - 1] <= 0)) fail("table ends above zero", t, lim[(size_t) count - 1]);
    for (int i = 1; i < count; i++) if (!(lim[(size_t) i] < lim[(size_t) i - 1])) fail("limits not falling", t, lim[(size_t) i]);
    // the walk of every entry, taken at its limit
    std::vector<unsigned long long> w0((size_t) count), w1((size_t) count);
    for (int i = 0; i < count; i++) {
        const double at = lim[(size_t) i] > 0 ? lim[(size_t) i] : 0.0;
        const int n = walk_block(t, 0, at, w0[(size_t) i], w1[(size_t) i]);
        if (n != np[(size_t) i]) fail("entry's passes", t, at);
        // its exact interval (walk_interval without a bracket): the table's limit, and up to the entry before
        double A, B;
        walk_interval(t, 0, w0[(size_t) i], w1[(size_t) i], 0, 0, 0.0, 0.0, A, B);
        if (A != lim[(size_t) i]) fail("lower limit != walk_interval's", t, at);
        if (B != (i > 0 ? lim[(size_t) i - 1] : DBL_MAX)) fail("intervals not contiguous", t, at);
    }
    auto check = [&](double x) {
        if (!(x >= 0) || !std::isfinite(x)) return;
        thresholds++;
        unsigned long long m0, m1, q0, q1;
        const int n = walk_block(t, 0, x, m0, m1);
        const int k = walk_table_find(lim.data(), 0, count - 1, x);
        if (k < 0) { if (lim[(size_t) count - 1] <= 0) fail("not found", t, x); return; }
        if (np[(size_t) k] != n || w0[(size_t) k] != m0 || w1[(size_t) k] != m1) fail("lookup != walk", t, x);
        if (k > 0 && !(x < lim[(size_t) k - 1])) fail("entry above", t, x);
        // bracketed search: from the entries of a threshold above and one below
        const double up = x * (1.0 + (double) (rng() % 1000) / 500.0) + 1e-300, dn = x * ((double) (rng() % 1000) / 1000.0);
        const int a = walk_table_find(lim.data(), 0, count - 1, up), z = walk_table_find(lim.data(), 0, count - 1, dn);
        if (a >= 0 && z >= 0 && walk_table_find(lim.data(), a, z, x) != k) fail("bracketed lookup", t, x);
        // plain form
        const int pn = walk_plain(t, x, q0, q1);
        if (pn != n || q0 != m0 || q1 != m1) fail("fast form != plain form", t, x);
    };
    double smin = DBL_MAX, smax = 0;
    for (int i = 0; i < count; i++) {
        const double A = lim[(size_t) i];
        if (A == -DBL_MAX) continue;
        check(A); check(next_up(A)); check(next_down(A));
        if (A > 0) { smin = A < smin ? A : smin; smax = A > smax ? A : smax; }
    }
    check(0.0); check(DBL_MAX); check(1e-300); check(DBL_EPSILON); check(1e-4); check(next_down(1e-4));
    if (smax > 0) {
        std::uniform_real_distribution<double> u(std::log(smin) - 2.0, std::log(smax) + 2.0);
        for (int i = 0; i < 64; i++) check(std::exp(u(rng)));
        // and close to the limits, where the 1e-11 bands of the fast form end
        for (int i = 0; i < count; i++)
            if (lim[(size_t) i] > 0)
                for (int k = 0; k < 4; k++) check(lim[(size_t) i] * (1.0 + ((double) (rng() % 2001) - 1000.0) * 2e-14));
    }
}

int main(int argc, char **argv)
{
    const int n_random = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937_64 rng(20240611);
    // hand-made tables
    {
        Tab t{{7}, {123.5}};                                           // one pass
        check_table(t, rng);
        Tab z{{0}, {5.0}};                                             // one pass of no bytes
        check_table(z, rng);
        Tab e{{}, {}};                                                 // no pass
        check_table(e, rng);
    }
    {
        Tab t;                                                         // all rate steps zero
        for (int p = 0; p < 12; p++) { t.r.push_back(9); t.d.push_back(100.0 + (p % 3 ? p : 0)); }
        check_table(t, rng);
        Tab u;
        for (int p = 0; p < 12; p++) { u.r.push_back(0); u.d.push_back(p % 2 ? 3.0 : 0.0); }
        check_table(u, rng);
    }
    {
        Tab t;                                                         // equal slopes in a row
        for (int p = 0; p < 30; p++) { t.r.push_back(4 * (p + 1)); t.d.push_back(10.0 * (p + 1)); }
        check_table(t, rng);
        Tab u;                                                         // ... in runs, rising and falling
        int r = 0; double d = 0;
        for (int p = 0; p < 40; p++) { r += 3; d += (p / 5) % 2 ? 6.0 : 1.5; u.r.push_back(r); u.d.push_back(d); }
        check_table(u, rng);
    }
    {
        Tab t;                                                         // slopes below 1e-4: the reject shortcut is off
        int r = 0; double d = 0;
        for (int p = 0; p < 25; p++) { r += 1 + p % 4; d += 1e-5 / (1 + p % 7); t.r.push_back(r); t.d.push_back(d); }
        check_table(t, rng);
        Tab u;                                                         // ... and around DBL_EPSILON
        r = 0; d = 0;
        for (int p = 0; p < 25; p++) { r += 1 + p % 3; d += DBL_EPSILON * (0.25 + p % 5); u.r.push_back(r); u.d.push_back(d); }
        check_table(u, rng);
    }
    {
        Tab t;                                                         // more than 64 passes: the m1 half of the mask
        int r = 0; double d = 0;
        for (int p = 0; p < 100; p++) { r += 1 + (p * 7) % 11; d += 1000.0 / (1 + (p * 5) % 13) * (p % 9 == 0 ? 0.0 : 1.0); t.r.push_back(r); t.d.push_back(d); }
        check_table(t, rng);
    }
    // random tables: 1..100 passes, slopes over 12 decades, zero rate steps, zero distortion steps, integer-valued distortions
    for (int k = 0; k < n_random; k++) {
        Tab t;
        const int tp = 1 + (int) (rng() % 100);
        const bool integral = rng() % 4 == 0;
        const double scale = std::pow(10.0, (double) (rng() % 13) - 6.0);
        int r = 0; double d = 0;
        for (int p = 0; p < tp; p++) {
            if (rng() % 8 != 0) r += 1 + (int) (rng() % (rng() % 3 ? 40 : 2000));
            if (r > 16000) r = 16000;
            if (rng() % 10 != 0) {
                double step = scale * std::pow(10.0, (double) (rng() % 6000) / 1000.0 - 3.0);
                if (integral) step = std::floor(step * 16.0) + (double) (rng() % 3);
                d += step;
            }
            t.r.push_back(r); t.d.push_back(d);
        }
        check_table(t, rng);
    }
    printf("%ld tables, %ld walks, %ld thresholds: %ld failures\n", tables, walks, thresholds, failures);
    return failures ? 1 : 0;
}
