// CPU harness for the settlement of chain_segment (abr_exact_jump.h), in both of its forms (SettleKind: by remainder, by
// three candidates): runs chains segment by segment next to the naive loop and reports the first case in which
//   1  the chain's value, addition count or hit flag differs from the naive loop's,
//   2  a segment with an unspoiled estimate jumped less (or more) than the longest legal jump, counted with naive additions.
// Built two ways by tests/test_chain_settle_cpu.py: as a shared library (helpers.native_harness), and with
// -DCHAIN_SETTLE_MAIN as a stand-alone program that reads the same cases from a file (the sanitizer build).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
static int64_t g_overshoot = 0;
#define ABR_BRACKET_HOOK(ok) (g_overshoot += (ok) ? 0 : 1)
#include "abr_exact_jump.h"

using namespace abrx;

template <int STOP>
static bool naive(double &x, double c, double thr, int32_t n, int32_t &a) {
    a = 0;
    while (a < n) {
        x = x + c;
        a++;
        if (stop_hit<STOP>(x, thr)) return true;
    }
    return false;
}

// chain_segment's own conditions for jumping at all, restated: a segment that may not jump has m = 0 by definition.
// This is a copy of the code under test, not an independent derivation: the longest-jump check guards the trip COUNT of
// segments that do jump; a wrong condition copied into both would only show where it changes a result, in the comparison
// with the naive loop.
template <int STOP>
static bool can_jump(const ChainState &cs, double c, int32_t n) {
    const int e = expo(cs.x);
    if (!(e > 54 && e < 2046) || n <= 0) return false;
    const double ac = (STOP == STOP_GE) ? c : -c;
    const double base = pow2_biased(e);
    const double dm = (base + ac) - base;
    const double rem = ac - dm;
    const bool tie = ((rem < 0.0) ? -rem : rem) == base * 0x1p-53;
    return expo(ac) < e && (!tie || cs.eb == e);
}

// The longest legal jump of a segment that starts at x with a budget of n additions: naive additions whose results stay
// inside the binade (going down: above its bottom) and on the near side of the stop, at most n - 1 of them.
template <int STOP>
static int32_t longest_jump(double x, double c, double thr, int32_t n) {
    const int e = expo(x);
    const double base = pow2_biased(e);
    int32_t m = 0;
    while (m < n - 1) {
        const double y = x + c;
        bool inside;
        if (STOP == STOP_GE) inside = y < thr && y < base + base;
        else if (STOP == STOP_LE) inside = y > thr && y > base;
        else inside = y >= thr && y > base;
        if (!inside) break;
        x = y; m++;
    }
    return m;
}

template <int STOP, int BIAS, int FORM>
static int check_one(double x0, double c, double thr, int32_t n, double &x_out, int32_t &a_out, bool &hit_out,
                     int64_t &segments) {
    ChainState cs;
    cs.x = x0; cs.eb = -1;
    int32_t a = 0;
    bool hit = false;
    while (a < n && !hit) {
        const int32_t left = n - a, budget = left < kJumpCap ? left : kJumpCap;
        const ChainState before = cs;
        const bool can = can_jump<STOP>(cs, c, budget);
        const int32_t did = chain_segment<STOP, BIAS, FORM>(cs, c, thr, left, hit);
        segments++;
        if (did < 1 || did > budget) return 2;
        if (BIAS == 0) {
            const int32_t want = can ? longest_jump<STOP>(before.x, c, thr, budget) : 0;
            if (did - 1 != want) return 2;
        }
        a += did;
    }
    // ... and the public entry point against the naive loop
    double xc = x0, xn = x0;
    int32_t ac = 0, an = 0;
    const bool hc = chain<STOP, BIAS, FORM>(xc, c, thr, n, ac);
    const bool hn = naive<STOP>(xn, c, thr, n, an);
    uint64_t bc, bn, bs;
    memcpy(&bc, &xc, 8); memcpy(&bn, &xn, 8); memcpy(&bs, &cs.x, 8);
    x_out = xc; a_out = ac; hit_out = hc;
    if (bc != bn || ac != an || hc != hn) return 1;
    if (bs != bn || a != an || hit != hn) return 1;
    return 0;
}

template <int STOP, int BIAS, int FORM>
static int64_t run(const double *x0, const double *c, const double *thr, const int32_t *n, int64_t cases,
                   double *x_out, int32_t *a_out, uint8_t *hit_out, int64_t *stats) {
    for (int64_t i = 0; i < cases; i++) {
        bool h = false;
        const int why = check_one<STOP, BIAS, FORM>(x0[i], c[i], thr[i], n[i], x_out[i], a_out[i], h, stats[0]);
        hit_out[i] = h;
        if (why) { stats[1] = why; return i; }
    }
    return -1;
}

extern "C" {
// kind: 0 >=, 1 <=, 2 <; bias: 0, +4, -4; form: SettleKind.  Returns the first failing case or -1; stats[0] += segments run, stats[1] = why
// (see the top of the file), stats[2] = estimates the settlement had to repair in this call.  -2: bad arguments.
int64_t settle_check(int32_t kind, int32_t bias, int32_t form, const double *x0, const double *c, const double *thr, const int32_t *n,
                     int64_t cases, double *x_out, int32_t *a_out, uint8_t *hit_out, int64_t *stats) {
    int64_t r = -2;
    g_overshoot = 0;
#define ABR_CASE(K, B) \
    if (kind == (K) && bias == (B)) \
        r = form == SETTLE_REMAINDER    ? run<(K), (B), SETTLE_REMAINDER>(x0, c, thr, n, cases, x_out, a_out, hit_out, stats) \
            : form == SETTLE_CANDIDATES ? run<(K), (B), SETTLE_CANDIDATES>(x0, c, thr, n, cases, x_out, a_out, hit_out, stats) \
                                        : -2;
    ABR_CASE(0, 0) ABR_CASE(0, 4) ABR_CASE(0, -4)
    ABR_CASE(1, 0) ABR_CASE(1, 4) ABR_CASE(1, -4)
    ABR_CASE(2, 0) ABR_CASE(2, 4) ABR_CASE(2, -4)
#undef ABR_CASE
    stats[2] = g_overshoot;
    return r;
}
int32_t settle_jump_cap() { return kJumpCap; }
}

#ifdef CHAIN_SETTLE_MAIN
// File: int64 blocks; per block int32 kind, int32 bias, int32 form, int32 0, int64 cases, then x0[], c[], thr[] (float64) and n[] (int32).
// Prints "ok <cases> <segments>" and exits 0 when every block passes.
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t blocks = 0, total = 0, stats[3] = {0, 0, 0};
    if (fread(&blocks, 8, 1, f) != 1) return 2;
    for (int64_t b = 0; b < blocks; b++) {
        int32_t kb[4];
        int64_t cases = 0;
        if (fread(kb, 4, 4, f) != 4 || fread(&cases, 8, 1, f) != 1 || cases < 0) return 2;
        const size_t N = (size_t)cases;
        double *x0 = (double *)malloc(8 * N + 8), *c = (double *)malloc(8 * N + 8), *thr = (double *)malloc(8 * N + 8);
        double *xo = (double *)malloc(8 * N + 8);
        int32_t *n = (int32_t *)malloc(4 * N + 4), *ao = (int32_t *)malloc(4 * N + 4);
        uint8_t *ho = (uint8_t *)malloc(N + 1);
        if (fread(x0, 8, N, f) != N || fread(c, 8, N, f) != N || fread(thr, 8, N, f) != N || fread(n, 4, N, f) != N) return 2;
        const int64_t bad = settle_check(kb[0], kb[1], kb[2], x0, c, thr, n, cases, xo, ao, ho, stats);
        if (bad != -1) {
            printf("block %lld (kind %d bias %d form %d): case %lld fails, why %lld\n", (long long)b, kb[0], kb[1], kb[2], (long long)bad,
                   (long long)stats[1]);
            return 1;
        }
        total += cases;
        free(x0); free(c); free(thr); free(xo); free(n); free(ao); free(ho);
    }
    fclose(f);
    printf("ok %lld %lld\n", (long long)total, (long long)stats[0]);
    return 0;
}
#endif
