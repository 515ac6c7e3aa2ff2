// gm_fmt_dev.h — exact printf("%g") and printf("%.2e") that compile for the host and for the device: the XA / XP columns of a SAM row
// (src/Driver.cpp:2196-2205) written by k_out_text_sizes (gm_output.hip), and the p-value of --snp's ninth .gmp column
// (PrintSNPCall src/GenomeBwt.cpp:1011-1090) written by k_track_rows (gm_tracktext.hip).  No library calls, no division of wide integers.
// Also gm_comp_char, the complement of a base as a reverse-strand row prints it (gm_output.hip, gm_bam.hip).
//
// Domain of gm_put_g6_hd: 0, -0, inf, nan and every double with 2^-200 <= |v| < 2^200 (every float, denormals included, times any
// sensible 1 / adjust); of gm_put_e2_hd: +0.0 and 2^-200 <= v < 2^200 (a p-value).  Outside it they write nothing and return their
// argument: a caller sees length 0 and refuses the record (or hands the slab to the host) instead of printing a wrong digit.
//
// Scheme, for D significant digits (6 and 3): v = m * 2^e2 with a 53-bit m.  For a decimal exponent E, N = floor(v / 10^(E-D+1)) is
// estimated in double (one rounding of v, one of the power: off by one at most), then pinned with 256-bit integers:
// A / B = v / 10^(E-D+1) with A, B products of m, a power of five (table) and a power of two (shift), N B <= A < (N+1) B.
// 10^(D-1) <= N < 10^D says that E was right; the remainder A - N B against B / 2 gives round-half-even on the exact binary value, as
// printf rounds.  Largest integer that occurs: m * 5^68 < 2^211.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GM_FMT_HD __host__ __device__
#else
#define GM_FMT_HD
#endif

// reverse_comp's table (SequenceOperations.h:56-96): a<->t, c<->g in both cases, '-' stays, everything else 'n'.  The bases of a
// reverse-strand row, as text (k_out_text_rows, gm_output.hip) and as BAM nibbles (k_bam_rows, gm_bam.hip)
GM_FMT_HD static inline char gm_comp_char(char c) {
    const char lo = (char)(c | 0x20);
    const char up = (char)(c == lo ? 0 : 0x20);            // subtracted again for an upper-case letter
    switch (lo) {
        case 'a': return (char)('t' - up); case 't': return (char)('a' - up);
        case 'c': return (char)('g' - up); case 'g': return (char)('c' - up);
        default: return c == '-' ? '-' : 'n';
    }
}

// The BAM nibble of a base, "=ACMGRSVTWYHKDBN" in either case; anything else is N (15).  One function for the SEQ nibbles of a
// record (k_bam_rows, gm_bam.hip) and for the comparison behind NM / MD (gm_md_walk, gm_mdtag_dev.h): the two cannot drift apart
GM_FMT_HD static inline uint32_t gm_bam_nibble(char c) {
    switch (c & ~0x20) {
        case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
        case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
        default: return c == '=' ? 0u : 15u;
    }
}

struct gm_u256 { uint64_t w0, w1, w2, w3; };             // little endian; named words, never indexed (no scratch on the device)

GM_FMT_HD static inline uint64_t gm_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// a * m; the callers' products stay below 2^256
GM_FMT_HD static inline gm_u256 gm_u256_mul64(gm_u256 a, uint64_t m) {
    gm_u256 r; uint64_t lo, c;
    r.w0 = a.w0 * m; c = gm_mulhi64(a.w0, m);
    lo = a.w1 * m; r.w1 = lo + c; c = gm_mulhi64(a.w1, m) + (r.w1 < lo ? 1u : 0u);
    lo = a.w2 * m; r.w2 = lo + c; c = gm_mulhi64(a.w2, m) + (r.w2 < lo ? 1u : 0u);
    r.w3 = a.w3 * m + c;
    return r;
}

GM_FMT_HD static inline gm_u256 gm_u256_shl(gm_u256 a, unsigned s) {            // s < 256
    const unsigned bs = s & 63u, ws = s >> 6;
    if (bs) {
        a.w3 = (a.w3 << bs) | (a.w2 >> (64u - bs)); a.w2 = (a.w2 << bs) | (a.w1 >> (64u - bs));
        a.w1 = (a.w1 << bs) | (a.w0 >> (64u - bs)); a.w0 <<= bs;
    }
    if (ws & 1u) { a.w3 = a.w2; a.w2 = a.w1; a.w1 = a.w0; a.w0 = 0; }
    if (ws & 2u) { a.w3 = a.w1; a.w2 = a.w0; a.w1 = 0; a.w0 = 0; }
    return a;
}

GM_FMT_HD static inline int gm_u256_cmp(const gm_u256& a, const gm_u256& b) {
    if (a.w3 != b.w3) return a.w3 < b.w3 ? -1 : 1;
    if (a.w2 != b.w2) return a.w2 < b.w2 ? -1 : 1;
    if (a.w1 != b.w1) return a.w1 < b.w1 ? -1 : 1;
    if (a.w0 != b.w0) return a.w0 < b.w0 ? -1 : 1;
    return 0;
}

GM_FMT_HD static inline gm_u256 gm_u256_sub(gm_u256 a, const gm_u256& b) {      // a >= b
    uint64_t br, t;
    t = a.w0 - b.w0; br = a.w0 < b.w0; a.w0 = t;
    t = a.w1 - b.w1 - br; br = (a.w1 < b.w1) || (a.w1 == b.w1 && br); a.w1 = t;
    t = a.w2 - b.w2 - br; br = (a.w2 < b.w2) || (a.w2 == b.w2 && br); a.w2 = t;
    a.w3 = a.w3 - b.w3 - br;
    return a;
}

// exactly `count` decimal digits of v (zero padded on the left)
GM_FMT_HD static inline char* gm_put_digits(char* w, uint32_t v, int count) {
    for (int i = count - 1; i >= 0; --i) { w[i] = (char)('0' + v % 10u); v /= 10u; }
    return w + count;
}

// the D leading decimal digits (D = 6: "%g", D = 3: "%.2e") of av = m * 2^e2, 2^-200 <= av < 2^200 with the biased exponent be:
// 10^(D-1) <= N < 10^D, its first digit at 10^E, rounded half-even on the exact binary value.  false: refused (the estimate was not
// within a few units, or a product would leave 256 bits); the callers then write nothing.
template <int D> GM_FMT_HD static inline bool gm_fmt_digits_hd(double av, int be, uint64_t m, int e2, uint32_t& N_out, int& E_out) {
    static_assert(D == 6 || D == 3, "the bounds below are worked out for these two");
    static const uint64_t t5[69][3] = {
        { 0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x0000000000000005ull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x0000000000000019ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x000000000000007dull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x0000000000000271ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x0000000000000c35ull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x0000000000003d09ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x000000000001312dull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x000000000005f5e1ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x00000000001dcd65ull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x00000000009502f9ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x0000000002e90eddull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x000000000e8d4a51ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x0000000048c27395ull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x000000016bcc41e9ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x000000071afd498dull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x0000002386f26fc1ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x000000b1a2bc2ec5ull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x000003782dace9d9ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x00001158e460913dull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x000056bc75e2d631ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x0001b1ae4d6e2ef5ull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x000878678326eac9ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x002a5a058fc295edull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x00d3c21bcecceda1ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x0422ca8b0a00a425ull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x14adf4b7320334b9ull, 0x0000000000000000ull, 0x0000000000000000ull }, { 0x6765c793fa10079dull, 0x0000000000000000ull, 0x0000000000000000ull },
        { 0x04fce5e3e2502611ull, 0x0000000000000002ull, 0x0000000000000000ull }, { 0x18f07d736b90be55ull, 0x000000000000000aull, 0x0000000000000000ull },
        { 0x7cb2734119d3b7a9ull, 0x0000000000000032ull, 0x0000000000000000ull }, { 0x6f7c40458122964dull, 0x00000000000000fcull, 0x0000000000000000ull },
        { 0x2d6d415b85acef81ull, 0x00000000000004eeull, 0x0000000000000000ull }, { 0xe32246c99c60ad85ull, 0x00000000000018a6ull, 0x0000000000000000ull },
        { 0x6fab61f00de36399ull, 0x0000000000007b42ull, 0x0000000000000000ull }, { 0x2e58e9b04570f1fdull, 0x000000000002684cull, 0x0000000000000000ull },
        { 0xe7bc90715b34b9f1ull, 0x00000000000c097cull, 0x0000000000000000ull }, { 0x86aed236c807a1b5ull, 0x00000000003c2f70ull, 0x0000000000000000ull },
        { 0xa16a1b11e8262889ull, 0x00000000012ced32ull, 0x0000000000000000ull }, { 0x2712875988becaadull, 0x0000000005e0a1fdull, 0x0000000000000000ull },
        { 0xc35ca4bfabb9f561ull, 0x000000001d6329f1ull, 0x0000000000000000ull }, { 0xd0cf37be5aa1cae5ull, 0x0000000092efd1b8ull, 0x0000000000000000ull },
        { 0x140c16b7c528f679ull, 0x00000002deaf189cull, 0x0000000000000000ull }, { 0x643c7196d9ccd05dull, 0x0000000e596b7b0cull, 0x0000000000000000ull },
        { 0xf52e37f2410011d1ull, 0x00000047bf19673dull, 0x0000000000000000ull }, { 0xc9e717bb45005915ull, 0x00000166bb7f0435ull, 0x0000000000000000ull },
        { 0xf18376a85901bd69ull, 0x00000701a97b150cull, 0x0000000000000000ull }, { 0xb7915149bd08b30dull, 0x000023084f676940ull, 0x0000000000000000ull },
        { 0x95d69670b12b7f41ull, 0x0000af298d050e43ull, 0x0000000000000000ull }, { 0xed30f03375d97c45ull, 0x00036bcfc1194751ull, 0x0000000000000000ull },
        { 0xa1f4b1014d3f6d59ull, 0x00111b0ec57e6499ull, 0x0000000000000000ull }, { 0x29c77506823d22bdull, 0x00558749db77f700ull, 0x0000000000000000ull },
        { 0xd0e549208b31adb1ull, 0x01aba4714957d300ull, 0x0000000000000000ull }, { 0x147a6da2b7f86475ull, 0x085a36366eb71f04ull, 0x0000000000000000ull },
        { 0x6664242d97d9f649ull, 0x29c30f1029939b14ull, 0x0000000000000000ull }, { 0xfff4b4e3f741cf6dull, 0xd0cf4b50cfe20765ull, 0x0000000000000000ull },
        { 0xffc78873d4490d21ull, 0x140c78940f6a24fdull, 0x0000000000000004ull }, { 0xfee5aa43256d41a5ull, 0x643e5ae44d12b8f5ull, 0x0000000000000014ull },
        { 0xfa7c534fbb224839ull, 0xf537c675815d9ccdull, 0x0000000000000065ull }, { 0xe46da08ea7ab691dull, 0xca16e04b86d41005ull, 0x00000000000001fdull },
        { 0x762422c946590d91ull, 0xf2726179a224501dull, 0x00000000000009f4ull }, { 0x4eb4adee5fbd43d5ull, 0xbc3be7602ab59093ull, 0x00000000000031c8ull },
        { 0x898765a7deb25329ull, 0xad2b84e0d58bd2e0ull, 0x000000000000f8ebull }, { 0xafa4fc47597b9fcdull, 0x61d998642bbb1e62ull, 0x000000000004dc9aull },
        { 0x6e38ed64bf6a1f01ull, 0xe93ff9f4daa797edull, 0x0000000000184f03ull }, { 0x271ca2f7bd129b05ull, 0x8e3fe1c84545f7a3ull, 0x0000000000798b13ull },
        { 0xc38f2ed6b15d0719ull, 0xc73f68e95a5dd62full, 0x00000000025fb761ull }, { 0xd1cbea3176d1237dull, 0xe43d0c8ec3d52eeeull, 0x000000000bde94e8ull },
        { 0x18fb92f75215b171ull, 0x75313ec9d329eaaaull, 0x000000003b58e88cull },
    };
    static const double p10[69] = {
        1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9,
        1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19,
        1e20, 1e21, 1e22, 1e23, 1e24, 1e25, 1e26, 1e27, 1e28, 1e29,
        1e30, 1e31, 1e32, 1e33, 1e34, 1e35, 1e36, 1e37, 1e38, 1e39,
        1e40, 1e41, 1e42, 1e43, 1e44, 1e45, 1e46, 1e47, 1e48, 1e49,
        1e50, 1e51, 1e52, 1e53, 1e54, 1e55, 1e56, 1e57, 1e58, 1e59,
        1e60, 1e61, 1e62, 1e63, 1e64, 1e65, 1e66, 1e67, 1e68,
    };
    int E = ((be - 1023) * 1233) >> 12;                      // floor(log10 |v|) to within two: N below says which way it is off
    constexpr uint64_t lo = D == 6 ? 100000ull : 100ull, hi = lo * 10ull;
    constexpr double xlo = D == 6 ? 1e3 : 1.0, xhi = D == 6 ? 1e9 : 1e6;     // E off by two either way still lands inside
    uint32_t N = 0;
    bool found = false;
    for (int tries = 0; tries < 5 && !found; ++tries) {
        const int j = E - (D - 1), aj = j < 0 ? -j : j;
        if (aj > 68) return false;
        // the estimate first: xlo <= x < xhi also says that nothing below leaves 256 bits (A 2^s < 2^30 B, B 2^-s <= A)
        const double x = j < 0 ? av * p10[aj] : av / p10[aj];
        if (!(x < xhi)) { ++E; continue; }
        if (!(x >= xlo)) { --E; continue; }
        gm_u256 P5; P5.w0 = t5[aj][0]; P5.w1 = t5[aj][1]; P5.w2 = t5[aj][2]; P5.w3 = 0;
        gm_u256 A, B;
        if (j < 0) { A = gm_u256_mul64(P5, m); B.w0 = 1; B.w1 = B.w2 = B.w3 = 0; }
        else { A.w0 = m; A.w1 = A.w2 = A.w3 = 0; B = P5; }
        const int s = e2 - j;                                // v / 10^j = A / B * 2^s
        if (s > 250 || s < -250) return false;
        if (s >= 0) A = gm_u256_shl(A, (unsigned)s); else B = gm_u256_shl(B, (unsigned)-s);
        uint64_t n = (uint64_t)x;
        gm_u256 NB = gm_u256_mul64(B, n);
        for (int k = 0; k < 4 && gm_u256_cmp(NB, A) > 0; ++k) { --n; NB = gm_u256_sub(NB, B); }
        if (gm_u256_cmp(NB, A) > 0) return false;
        gm_u256 R = gm_u256_sub(A, NB);
        for (int k = 0; k < 4 && gm_u256_cmp(R, B) >= 0; ++k) { ++n; R = gm_u256_sub(R, B); }
        if (gm_u256_cmp(R, B) >= 0) return false;            // the estimate was not within a few units: refuse, never guess
        if (n < lo) { --E; continue; }
        if (n >= hi) { ++E; continue; }
        const int c = gm_u256_cmp(gm_u256_shl(R, 1), B);     // remainder against one half
        if (c > 0 || (c == 0 && (n & 1ull))) ++n;
        if (n == hi) { n = lo; ++E; }                        // the rounding carried into one digit more
        N = (uint32_t)n;
        found = true;
    }
    N_out = N; E_out = E;
    return found;
}

// "%g" of v; returns the end of the text, or w itself (nothing written) outside the domain
GM_FMT_HD static inline char* gm_put_g6_hd(char* w, double v) {
    char* const w0 = w;
    uint64_t bits;
    __builtin_memcpy(&bits, &v, 8);
    const bool neg = (bits >> 63) != 0;
    const int be = (int)((bits >> 52) & 0x7FFu);
    const uint64_t frac = bits & ((1ull << 52) - 1);
    if (be == 0x7FF) {                                       // glibc: inf, -inf, nan, -nan
        if (neg) *w++ = '-';
        if (frac) { *w++ = 'n'; *w++ = 'a'; *w++ = 'n'; } else { *w++ = 'i'; *w++ = 'n'; *w++ = 'f'; }
        return w;
    }
    if (be == 0 && frac == 0) { if (neg) *w++ = '-'; *w++ = '0'; return w; }
    if (be < 1023 - 200 || be >= 1023 + 200) return w0;      // outside 2^-200 <= |v| < 2^200 (denormal doubles included)
    const uint64_t m = frac | (1ull << 52);
    const int e2 = be - 1075;                                // |v| = m * 2^e2
    const uint64_t abits = bits & ~(1ull << 63);
    double av;
    __builtin_memcpy(&av, &abits, 8);
    uint32_t N; int E;
    if (!gm_fmt_digits_hd<6>(av, be, m, e2, N, E)) return w0;
    int nd = 6;
    while (nd > 1 && N % 10u == 0) { N /= 10u; --nd; }       // trailing zeros go (no '#' flag); N now has nd digits, the first at 10^E
    if (neg) *w++ = '-';
    if (E < -4 || E >= 6) {                                  // exponent form: d[.ddddd]e[+-]XX, two exponent digits at least
        uint32_t top = 1;
        for (int i = 1; i < nd; ++i) top *= 10u;
        *w++ = (char)('0' + N / top);
        if (nd > 1) { *w++ = '.'; w = gm_put_digits(w, N % top, nd - 1); }
        *w++ = 'e';
        int ae = E;
        if (E < 0) { *w++ = '-'; ae = -E; } else *w++ = '+';
        w = gm_put_digits(w, (uint32_t)ae, ae >= 100 ? 3 : 2);
    } else if (E >= 0) {
        const int ip = E + 1;                                // digits before the point
        if (nd <= ip) { w = gm_put_digits(w, N, nd); for (int i = nd; i < ip; ++i) *w++ = '0'; }
        else {
            uint32_t low = 1;
            for (int i = ip; i < nd; ++i) low *= 10u;
            w = gm_put_digits(w, N / low, ip);
            *w++ = '.';
            w = gm_put_digits(w, N % low, nd - ip);
        }
    } else {
        *w++ = '0'; *w++ = '.';
        for (int i = -1; i > E; --i) *w++ = '0';
        w = gm_put_digits(w, N, nd);
    }
    return w;
}

// "%.2e" of v, always the 8 characters d.dde[+-]dd; returns the end of the text, or w itself (nothing written) outside the domain:
// +0.0 and positive doubles with 2^-200 <= v < 2^200 (decimal exponents -61 .. 60).  The p-value of --snp's ninth column.
GM_FMT_HD static inline char* gm_put_e2_hd(char* w, double v) {
    uint64_t bits;
    __builtin_memcpy(&bits, &v, 8);
    uint32_t N = 0; int E = 0;                               // +0.0: 0.00e+00
    if (bits) {
        const int be = (int)((bits >> 52) & 0x7FFu);
        if ((bits >> 63) || be < 1023 - 200 || be >= 1023 + 200) return w;       // negative, -0.0, nan, inf, denormal, out of range
        if (!gm_fmt_digits_hd<3>(v, be, (bits & ((1ull << 52) - 1)) | (1ull << 52), be - 1075, N, E)) return w;
    }
    const uint32_t ae = (uint32_t)(E < 0 ? -E : E);          // <= 61
    w[0] = (char)('0' + N / 100u); w[1] = '.'; w[2] = (char)('0' + N / 10u % 10u); w[3] = (char)('0' + N % 10u);
    w[4] = 'e'; w[5] = E < 0 ? '-' : '+'; w[6] = (char)('0' + ae / 10u); w[7] = (char)('0' + ae % 10u);
    return w + 8;
}
