// checks gnumap_amd/csrc/gm_fmt_dev.h on the host: gm_put_g6_hd must write what printf("%g") writes on its domain (0, -0, inf, nan and
// 2^-200 <= |v| < 2^200) and nothing (length 0) outside it.  The value families of fmt_g6_check.cpp, plus the ones the exponent form
// and the wide range add.
#include "gm_fmt_dev.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
int main() {
    std::mt19937_64 rng(11);
    char a[64], b[64]; long bad = 0, n = 0, outside = 0;
    const double lo_edge = std::ldexp(1.0, -200), hi_edge = std::ldexp(1.0, 200);
    auto in_domain = [&](double v) { const double av = std::fabs(v); return v == 0 || std::isinf(v) || std::isnan(v) || (av >= lo_edge && av < hi_edge); };
    auto chk = [&](double v) {
        memset(a, 0x7f, sizeof a);
        char* e = gm_put_g6_hd(a, v); ++n;
        if (!in_domain(v)) { ++outside; if (e != a) { if (bad < 10) printf("OUTSIDE %.17g: length %ld, not 0\n", v, (long)(e - a)); ++bad; } return; }
        *e = 0; snprintf(b, sizeof b, "%g", v);
        if (strcmp(a, b)) { if (bad < 10) printf("MISMATCH %.17g: %s vs %s\n", v, a, b); ++bad; }
    };
    for (long i = 0; i < 1500000; ++i) {                     // fmt_g6_check.cpp's first family
        const double u = (double)(rng() >> 11) / 9007199254740992.0;
        const int dec = (int)(rng() % 13) - 5;
        const float f = (float)(u * std::pow(10.0, dec));
        chk((double)f); chk(-(double)f); chk((double)f * (1.0 / 0.37)); chk(u * std::pow(10.0, dec));
    }
    for (int e = -6; e <= 7; ++e)
        for (int k = -3; k <= 3; ++k) {
            const double p = std::pow(10.0, e);
            chk(std::nextafter(p, k < 0 ? 0 : 1e300)); chk(p); chk(p * (1 + k * 1e-7)); chk(p * 9.999995); chk(p * 9.9999949); chk(p * 1.5); chk(p * 1.000005); chk(p * 2.000015);
        }
    for (long i = 0; i < 500000; ++i) {                      // exact halves of the sixth digit, and short binary fractions
        const double x = (double)(100000 + rng() % 900000) + 0.5; const int dec = (int)(rng() % 10) - 9;
        chk(x * std::pow(10.0, dec)); chk(std::ldexp((double)(rng() % (1 << 24)), -(int)(rng() % 30)));
    }
    const double fixed[] = { 0.0, -0.0, 1.0, 0.5, 999999.5, 999999.4999, 0.0001, 0.00009999995, 1e6, 123456.5, 1234565e-1, 0.1, 100000, INFINITY, -INFINITY, NAN, -NAN,
                             5e-324, 1e-5, 1e300, 2.5e-7, 8.40759e-05, -1e-300, 2.2250738585072014e-308 };
    for (double v : fixed) chk(v);
    // every power of ten from 1e-60 to 1e60 and both neighbours, with the ties and near-ties of the sixth digit around them
    for (int e = -60; e <= 60; ++e) {
        char t[16]; snprintf(t, sizeof t, "1e%d", e);
        const double p = strtod(t, nullptr);
        chk(p); chk(std::nextafter(p, 0)); chk(std::nextafter(p, 1e300)); chk(-p);
        chk(p * 9.999995); chk(p * 9.9999949); chk(p * 9.9999951); chk(p * 1.000005); chk(p * 2.000015); chk(p * 1.5);
    }
    // the two edges of the domain and a value just outside each
    chk(lo_edge); chk(-lo_edge); chk(std::nextafter(lo_edge, 0)); chk(std::nextafter(hi_edge, 0)); chk(hi_edge); chk(-hi_edge); chk(std::nextafter(lo_edge, 1));
    // exact sixth-digit ties in exponent form: (6 digits + 0.5) * 2^k is exact in binary, so the scaled value is an exact tie whenever
    // the power of ten divides out; dyadic scalings keep the half exactly representable
    for (long i = 0; i < 300000; ++i) {
        const double x = (double)(100000 + rng() % 900000) + 0.5;
        chk(x * 1e-11); chk(x * 1e7); chk(x * 1e9); chk(std::ldexp(x, (int)(rng() % 300) - 150));
        chk((double)(1000000 + 2 * (rng() % 4500000) + 1) * 0.5 * 1e10);      // an odd integer / 2 * 10^10 is an integer below 2^53: exact, and a tie when it has seven digits
        const uint64_t six = 100000 + rng() % 900000;
        chk((double)(six * 10 + 5) * 1e6); chk((double)(six * 10 + 5) * 1e12); chk((double)(six * 10 + 5) * 1e15);
    }
    // floats widened to double across the whole float exponent range, denormals included; times 1/0.25 and 1/1.0 (the reference's adjust values)
    for (long i = 0; i < 2000000; ++i) {
        uint32_t u = (uint32_t)rng(); float f; memcpy(&f, &u, 4);
        const double d = (double)f;
        chk(d); chk(d * (1.0 / 0.25f)); chk(d * (1.0 / 1.0f));
    }
    for (uint32_t ex = 0; ex < 255; ++ex)                    // every float exponent: the smallest, the largest and a middle mantissa
        for (uint32_t mant : { 0u, 1u, 0x400000u, 0x7FFFFFu, 0x2AAAAAu }) {
            uint32_t u = (ex << 23) | mant; float f; memcpy(&f, &u, 4);
            chk((double)f); chk(-(double)f); chk((double)f * 4.0);
        }
    for (uint32_t mant = 1; mant < 200000; mant += 7) { float f; memcpy(&f, &mant, 4); chk((double)f); }     // float denormals
    // random doubles over the whole double range: in-domain ones must match, the others must give length 0
    for (long i = 0; i < 1000000; ++i) { uint64_t u = rng(); double d; memcpy(&d, &u, 8); chk(d); }
    for (long i = 0; i < 1000000; ++i) chk(std::ldexp(1.0 + (double)(rng() >> 12) / 4503599627370496.0, (int)(rng() % 420) - 210));
    printf("%ld values (%ld outside the domain), %ld mismatches\n", n, outside, bad);
    return bad != 0 || outside < 1000;
}
