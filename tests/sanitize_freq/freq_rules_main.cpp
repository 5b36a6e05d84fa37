// The rules of meth-freq (csrc/abea_freq_rules.h) compiled for the host and held against the C library: "%.3lf" of every
// m / c with m <= c <= 2048, strtod of "%.2lf" for every k / 1024 with |k| <= 16384 and for a million seeded float pairs, "%d",
// the line length, the CG step on buffers of exactly the record's size.  Built with ASan + UBSan (Makefile); prints the counts
// and exits 0, or names the first mismatch and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../genomicsbench_amd/csrc/abea_freq_rules.h"

namespace R = gbx::abea_freq_rules;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || R::bits_of(a) == R::bits_of(b); }

static int check_llr(double x, const char *what)
{
    char text[512];
    snprintf(text, sizeof text, "%.2lf", x);
    const double want = strtod(text, nullptr), got = R::llr_as_printed(x);
    if (same(want, got)) return 0;
    fprintf(stderr, "%s: %.17g prints %s reads %.17g, the rule gives %.17g\n", what, x, text, want, got);
    return 1;
}

int main()
{
    long n_freq = 0, n_llr = 0, n_dec = 0;
    // "%.3lf"
    for (int c = 1; c <= 2048; ++c)
        for (int m = 0; m <= c; ++m, ++n_freq) {
            char want[32], got[8] = {0};
            snprintf(want, sizeof want, "%.3lf", (double)m / c);
            R::freq_put(got, R::freq_milli(m, c));
            if (strlen(want) != R::FREQ_LEN || memcmp(want, got, R::FREQ_LEN)) { fprintf(stderr, "%d / %d: %s, the rule gives %s\n", m, c, want, got); return 1; }
        }
    const int big[][2] = {{1, 2147483647}, {2147483646, 2147483647}, {1073741823, 2147483647}, {2147483647, 2147483647}, {1, 2001}, {1001, 2002000}};
    for (const auto &p : big) {
        char want[32], got[8] = {0};
        snprintf(want, sizeof want, "%.3lf", (double)p[0] / p[1]);
        R::freq_put(got, R::freq_milli(p[0], p[1]));
        if (memcmp(want, got, R::FREQ_LEN)) { fprintf(stderr, "%d / %d: %s, the rule gives %s\n", p[0], p[1], want, got); return 1; }
    }
    // the two-decimal rule
    for (int k = -16384; k <= 16384; ++k, ++n_llr)
        if (check_llr((double)k / 1024.0, "k / 1024")) return 1;
    const double edges[] = {0.0, -0.0, 0.005, -0.005, 0.015, 0.004999999999999999, 1e-320, -1e-320, 4.9e-324, 2.4951171875, -2.4951171875, 2.494140625, 2.125,
                            2.375, 70368744177663.99, 70368744177664.0, -70368744177664.0, 70368744177664.02, 35184372088831.996, 4503599627370495.5,
                            4503599627370496.0, 1e300, -1e300, 1.7976931348623157e308, INFINITY, -INFINITY, NAN, -NAN, 0.125, 0.375, 1e15 + 0.125, 1234567.005};
    for (double x : edges) { if (check_llr(x, "edge")) return 1; ++n_llr; }
    for (int i = 0; i < 1000000; ++i, ++n_llr) {
        float a, b;
        if (i & 1) {                                              // any two floats
            const uint32_t ua = (uint32_t)rnd(), ub = (uint32_t)rnd();
            memcpy(&a, &ua, 4); memcpy(&b, &ub, 4);
        } else {                                                  // two scores a few units apart, on a grid that meets the ties
            a = -(float)(rnd() % 4000000) / 1024.0f;
            b = a + ((float)(rnd() % 16384) - 8192.0f) / 1024.0f;
        }
        if (check_llr((double)a - (double)b, "float pair")) return 1;
    }
    // "%d" and the line
    std::vector<long long> ints = {0, 1, 9, 10, 99, 100, 999999999, 1000000000, 2147483647, -1, -9, -10, -2147483647 - 1LL};
    for (int i = 0; i < 10000; ++i) ints.push_back((long long)(int32_t)rnd());
    for (long long v : ints) {
        char want[32], got[32] = {0};
        const int n = snprintf(want, sizeof want, "%d", (int)v);
        ++n_dec;
        if (R::dec_len(v) != n || R::dec_put(got, v) != n || memcmp(want, got, (size_t)n)) { fprintf(stderr, "%%d of %lld: %s, the rule gives %s\n", v, want, got); return 1; }
    }
    {
        char line[256];
        const int n = snprintf(line, sizeof line, "\t%d\t%d\t%d\t%d\t%d\t%.3lf\t%s\n", 2147483647, 0, 12, 2000, 9, 9.0 / 2000, "split-group");
        if (R::line_tail_len(2147483647, 0, 12, 2000, 9, -1) != n || R::line_tail_len(2147483647, 0, 12, 2000, 9, 7) != n - 4) { fprintf(stderr, "line length\n"); return 1; }
    }
    // the CG step never reads past the record: heap buffers of exactly its size
    const char *seqs[] = {"", "C", "G", "CG", "CGCG", "AAC", "GAA", "AACGAACG", "cgCg", "CCGG"};
    const int want_cg[] = {0, 0, 0, 1, 2, 0, 0, 2, 0, 1};
    for (size_t k = 0; k < sizeof seqs / sizeof *seqs; ++k) {
        const size_t len = strlen(seqs[k]);
        char *buf = (char *)malloc(len ? len : 1);
        memcpy(buf, seqs[k], len);
        int n = 0;
        for (long long i = -1; i <= (long long)len; ++i) n += R::cg_at(buf, (long long)len, i) ? 1 : 0;
        free(buf);
        if (n != want_cg[k]) { fprintf(stderr, "CG step on \"%s\": %d\n", seqs[k], n); return 1; }
    }
    // the call and the key order
    if (R::called(2.49, 2.5) || !R::called(2.5, 2.5) || !R::called(-2.5, 2.5) || !R::called(NAN, 2.5) || !R::called(0.0, 0.0) || R::methylated(NAN) ||
        R::methylated(-0.0) || !R::methylated(0.01) || !R::splits(1, 2) || R::splits(1, 1) || R::splits(0, 5)) { fprintf(stderr, "the call\n"); return 1; }
    if (R::key_cmp(0, 5, 5, 1, 0, 0) >= 0 || R::key_cmp(1, 5, 9, 1, 5, 7) <= 0 || R::key_cmp(2, 2147483647, 0, 2, 0, 2147483647) <= 0 || R::key_cmp(3, 4, 5, 3, 4, 5) != 0) {
        fprintf(stderr, "the key order\n");
        return 1;
    }
    if (R::site_byte('c') != 'C' || R::site_byte('n') != 'A' || R::site_byte('Y') != 'C' || R::site_byte('k') != 'G') { fprintf(stderr, "the site byte\n"); return 1; }
    printf("ok freq %ld llr %ld dec %ld\n", n_freq, n_llr, n_dec);
    return 0;
}
