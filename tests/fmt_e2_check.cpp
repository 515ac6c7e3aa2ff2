// checks gnumap_amd/csrc/gm_fmt_dev.h on the host: gm_put_e2_hd must write what printf("%.2e") writes on its domain (+0.0 and
// 2^-200 <= v < 2^200), always 8 characters, and nothing (length 0) outside it.  The values the ninth .gmp column prints are 0, 1
// and 1 - P, multiples of 2^-53; the function is checked on its whole domain all the same.
#include "gm_fmt_dev.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
int main() {
    std::mt19937_64 rng(29);
    char a[64], b[64]; long bad = 0, n = 0, outside = 0;
    const double lo_edge = std::ldexp(1.0, -200), hi_edge = std::ldexp(1.0, 200);
    auto in_domain = [&](double v) { return (v == 0 && !std::signbit(v)) || (v >= lo_edge && v < hi_edge); };
    auto chk = [&](double v) {
        memset(a, 0x7f, sizeof a);
        char* e = gm_put_e2_hd(a, v); ++n;
        if (!in_domain(v)) {
            ++outside;
            if (e != a || a[0] != 0x7f) { if (bad < 10) printf("OUTSIDE %.17g: length %ld or a byte written\n", v, (long)(e - a)); ++bad; }
            return;
        }
        if (e - a != 8 || a[8] != 0x7f) { if (bad < 10) printf("LENGTH %.17g: %ld\n", v, (long)(e - a)); ++bad; return; }
        *e = 0; snprintf(b, sizeof b, "%.2e", v);
        if (strcmp(a, b)) { if (bad < 10) printf("MISMATCH %.17g: %s vs %s\n", v, a, b); ++bad; }
    };
    auto around = [&](double v) { chk(v); chk(std::nextafter(v, 0)); chk(std::nextafter(v, INFINITY)); };
    // log-uniform over the domain: a random mantissa under every exponent
    for (long i = 0; i < 2000000; ++i) chk(std::ldexp(1.0 + (double)(rng() >> 12) / 4503599627370496.0, (int)(rng() % 400) - 200));
    // multiples of 2^-53: what 1 - P can be
    for (long k = 1; k <= 1000000; ++k) chk(std::ldexp((double)k, -53));
    for (long i = 0; i < 1000000; ++i) chk(std::ldexp((double)(rng() >> 11), -53));
    for (long i = 0; i < 500000; ++i) chk(1.0 - std::ldexp((double)(rng() >> (11 + rng() % 50)), -53));
    // every decimal tie candidate d.dd5e+-XX (the double next to it) and its two neighbours in ulps; 9.995 carries among them
    for (int e = -60; e <= 59; ++e)
        for (int d = 1000; d <= 9999; ++d) {
            char t[24]; snprintf(t, sizeof t, "%d.%03de%d", d / 1000, d % 1000, e);
            if (d % 10 == 5) around(strtod(t, nullptr));
        }
    for (int e = -60; e <= 59; ++e) {
        char t[24];
        snprintf(t, sizeof t, "9.995e%d", e); around(strtod(t, nullptr));
        snprintf(t, sizeof t, "9.994999e%d", e); around(strtod(t, nullptr));
        snprintf(t, sizeof t, "9.9949999999999999e%d", e); around(strtod(t, nullptr));
        snprintf(t, sizeof t, "9.99e%d", e); around(strtod(t, nullptr));
    }
    // exactly representable ties: d.dd5 with a short binary fraction (x.125, x.375, ...) under dyadic scalings, and 2^-k
    for (int k = 0; k <= 200; ++k) { around(std::ldexp(1.0, -k)); if (k < 200) around(std::ldexp(1.0, k)); }
    for (int i = 1; i < 80; ++i) { around(i * 0.125); around(i * 0.0625 + 1.0); around(i * 0.125 * 1000.0); }
    for (double v : { 1.125, 1.375, 1.625, 1.875, 2.125, 9.875, 9.625, 1.005, 1.015, 1.025, 1.035, 1.045, 112.5, 137.5, 1125.0, 11250.0, 0.5, 0.25, 0.125, 0.0625 }) around(v);
    for (long i = 0; i < 300000; ++i) {                      // (3 digits + 0.5) * 2^k: an exact binary number; a decimal tie where the power of ten divides out
        const double x = (double)(100 + rng() % 900) + 0.5;
        chk(x); chk(x * 1e3); chk(x * 1e9); chk(x * 1e15); chk(x * 1e-2); chk(std::ldexp(x, (int)(rng() % 300) - 150));
        chk((double)((1000 + rng() % 9000) * 10 + 5) * 1e6); chk((double)((100 + rng() % 900) * 10 + 5) * 1e18);
    }
    // powers of ten from 1e-60 to 1e60 with their neighbours
    for (int e = -60; e <= 60; ++e) {
        char t[16]; snprintf(t, sizeof t, "1e%d", e);
        const double p = strtod(t, nullptr);
        around(p); chk(p * 9.995); chk(p * 9.994999); chk(p * 9.995001); chk(p * 1.005); chk(p * 1.5); chk(p * 2.015);
    }
    const double fixed[] = { 0.0, 1.0, 0.001, 0.05, 0.999, 0.9995, 0.99949999999999994, 1e-16, 1.1102230246251565e-16, 2.220446049250313e-16, 5e-17 };
    for (double v : fixed) chk(v);
    // the two edges of the domain, in and out
    chk(lo_edge); chk(std::nextafter(lo_edge, 0)); chk(std::nextafter(lo_edge, 1)); chk(std::nextafter(hi_edge, 0)); chk(hi_edge); chk(std::nextafter(hi_edge, INFINITY));
    // outside: negative, -0.0, nan, inf, denormals, the far ends; random bit patterns over all doubles
    const double out[] = { -0.0, -1.0, -0.001, -lo_edge, -hi_edge, NAN, -NAN, INFINITY, -INFINITY, 5e-324, 2.2250738585072014e-308, 1e-300, 1e300, 1e-61, 1e61, 1.7e308 };
    for (double v : out) chk(v);
    for (long i = 0; i < 1000000; ++i) { uint64_t u = rng(); double d; memcpy(&d, &u, 8); chk(d); }
    for (long i = 0; i < 500000; ++i) chk(-std::ldexp(1.0 + (double)(rng() >> 12) / 4503599627370496.0, (int)(rng() % 400) - 200));
    printf("%ld values (%ld outside the domain), %ld mismatches\n", n, outside, bad);
    return bad != 0 || outside < 1000;
}
