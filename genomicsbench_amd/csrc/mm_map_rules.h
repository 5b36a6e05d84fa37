// mm_map_rules.h — minimap2 behind the chain scores: chain ends, backtrack, chain order, regions (mm_gen_regs), parents
// (mm_set_parent), selection (mm_select_sub), mapq (mm_set_mapq) and the PAF line, for one read.  One text for the device
// (mm_map_kernels.hip: a wavefront per read) and for a plain C++ build on the host (shims/mm_map_cpu_twin.cpp, one thread), which
// the CPU tests hold against the restatement tests/mm_map_ref.py.
//
// A function takes a team T: lane() of size() lanes work on the read, sync() is a barrier that also makes the team's stores
// visible to it, atomic_min / atomic_add act on an int in memory and return what was there.  On the host the team is one lane.
// Every sync() is reached by all lanes: the loops around them run on values every lane reads alike.
//
// Backtrack without the sequential walk: walking the keys in rank order, a walk marks upwards until it meets a mark, so in the
// end an anchor belongs to the lowest rank whose start lies in its subtree of the parent forest.  Every key walks at once and
// lowers own[] with atomic_min, leaving where a lower rank has been (that rank marks everything above, or stops at a lower one
// still).  Key k's chain is then its start and the anchors above it that it owns; the anchor it stops at gives the score rule.
#pragma once
#include <cstdint>
#include <cmath>
#include "mm_machine.h"
#include "../../include/gbx.h"

namespace gbx {

struct MmSolo {                                    // the host's team
    int lane() const { return 0; }
    int size() const { return 1; }
    void sync() const {}
    int atomic_min(int32_t *p, int32_t v) const { const int32_t o = *p; if (v < o) *p = v; return o; }
    int atomic_add(int32_t *p, int32_t v) const { const int32_t o = *p; *p = o + v; return o; }
};

struct MmZ { uint64_t x, y; };

// one read's input: n anchors with chain's score f, parent p (local, -1: none; chain leaves p[i] < i, anything else counts as
// none) and peak v
struct MmMapRead {
    int32_t n;
    const uint64_t *ax, *ay;
    const int32_t *f, *p, *v;
    int32_t qlen, rep_len;
    uint32_t hash;
};
// n entries each, the read's own
struct MmChainWork {
    int32_t *own, *top, *perm;
    uint64_t *key, *urank;
    int32_t *n_keys;                               // one int
};

GBX_MM_HD inline int32_t mm_map_par(const int32_t *p, int32_t i)
{
    const int32_t j = p[i];
    return j >= 0 && j < i ? j : -1;
}

// ascending by less(); any n, the bitonic network with the tail taken as +infinity.  less() must be a total order.
template <class T, class E, class Less>
GBX_MM_HD inline void mm_team_sort(const T &t, E *a, int32_t n, const Less &less)
{
    for (int64_t k = 2; (k >> 1) < n; k <<= 1) {
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t i = t.lane(); i < n; i += t.size()) {
                const int64_t l = j == (k >> 1) ? (i ^ (k - 1)) : (i ^ j);
                if (l > i && l < n && less(a[l], a[i])) { const E e = a[i]; a[i] = a[l]; a[l] = e; }
            }
            t.sync();
        }
    }
}

struct MmKeyDesc { GBX_MM_HD bool operator()(uint64_t a, uint64_t b) const { return a > b; } };
struct MmByFirstX {
    const uint64_t *ax; const int32_t *top;
    GBX_MM_HD bool operator()(int32_t a, int32_t b) const
    {
        const uint64_t xa = ax[top[a]], xb = ax[top[b]];
        return xa != xb ? xa < xb : a < b;
    }
};
struct MmZDesc { GBX_MM_HD bool operator()(const MmZ &a, const MmZ &b) const { return a.x != b.x ? a.x > b.x : a.y > b.y; } };

// Steps 1-3: chain ends, backtrack, chain order.  -> the chains' keys u_out[*n_chains] (score << 32 | anchors) in order and
// their anchors cax, cay [*n_chained], concatenated.  All outputs are the read's own, n entries.
template <class T>
GBX_MM_HD inline void mm_map_chains(const T &t, const MmMapRead &r, const gbx_mm_map_params &P, const MmChainWork &w, uint64_t *u_out,
                                    uint64_t *cax, uint64_t *cay, int32_t *n_chains, int32_t *n_chained)
{
    const int32_t n = r.n, NONE = 0x7fffffff;
    for (int32_t i = t.lane(); i < n; i += t.size()) w.own[i] = NONE;
    if (t.lane() == 0) { *w.n_keys = 0; *n_chains = 0; *n_chained = 0; }
    t.sync();
    for (int32_t i = t.lane(); i < n; i += t.size()) {
        const int32_t j = mm_map_par(r.p, i);
        if (j >= 0) w.own[j] = 0;                                     // has a child
    }
    t.sync();
    for (int32_t i = t.lane(); i < n; i += t.size()) {
        if (w.own[i] != NONE || r.v[i] < P.min_chain_score) continue;
        int32_t j = i;
        while (j >= 0 && r.f[j] < r.v[j]) j = mm_map_par(r.p, j);
        if (j < 0) j = i;
        w.key[t.atomic_add(w.n_keys, 1)] = (uint64_t)(uint32_t)r.f[j] << 32 | (uint32_t)j;
    }
    t.sync();
    const int32_t nk = *w.n_keys;
    for (int32_t i = t.lane(); i < n; i += t.size()) w.own[i] = NONE;
    t.sync();
    mm_team_sort(t, w.key, nk, MmKeyDesc());
    for (int32_t k = t.lane(); k < nk; k += t.size()) {
        int32_t j = (int32_t)(uint32_t)w.key[k];
        while (j >= 0) {
            if (t.atomic_min(&w.own[j], k) < k) break;
            j = mm_map_par(r.p, j);
        }
    }
    t.sync();
    for (int32_t k = t.lane(); k < nk; k += t.size()) {
        const int32_t start = (int32_t)(uint32_t)w.key[k], s = (int32_t)(w.key[k] >> 32);
        int32_t c = 1, last = start, j = mm_map_par(r.p, start);
        while (j >= 0 && w.own[j] == k) { ++c; last = j; j = mm_map_par(r.p, j); }
        const int32_t sc = j < 0 ? s : s - r.f[j];
        const bool keep = c >= P.min_cnt && (j < 0 || sc >= P.min_chain_score);
        w.urank[k] = keep ? (uint64_t)(uint32_t)sc << 32 | (uint32_t)c : 0;
        w.top[k] = last;
    }
    t.sync();
    if (t.lane() == 0) {
        int32_t m = 0;
        for (int32_t k = 0; k < nk; ++k)
            if (w.urank[k]) w.perm[m++] = k;
        *n_chains = m;
    }
    t.sync();
    const int32_t m = *n_chains;
    mm_team_sort(t, w.perm, m, MmByFirstX{r.ax, w.top});
    if (t.lane() == 0) {
        int32_t pos = 0;
        for (int32_t i = 0; i < m; ++i) {
            const int32_t k = w.perm[i];
            u_out[i] = w.urank[k];
            w.top[k] = pos;                                           // from here on: where the chain's anchors go
            pos += (int32_t)(uint32_t)w.urank[k];
        }
        *n_chained = pos;
    }
    t.sync();
    for (int32_t i = t.lane(); i < m; i += t.size()) {
        const int32_t k = w.perm[i], c = (int32_t)(uint32_t)w.urank[k], pos = w.top[k];
        int32_t j = (int32_t)(uint32_t)w.key[k];
        for (int32_t step = 0; step < c && j >= 0; ++step) {
            cax[pos + c - 1 - step] = r.ax[j];
            cay[pos + c - 1 - step] = r.ay[j];
            j = mm_map_par(r.p, j);
        }
    }
    t.sync();
}

// L(n): the double logarithm rounded once to float
GBX_MM_HD inline float mm_map_logf(int32_t n) { return (float)log((double)n); }

// Steps 4-7 on a read's nch chains u (step-3 order) and chained anchors a: -> regs[*n_regs], *n_regs <= nch.  z, w: nch entries.
template <class T>
GBX_MM_HD inline void mm_map_regs(const T &t, const MmMapRead &r, int32_t read, const gbx_mm_map_params &P, int32_t nch, const uint64_t *u,
                                  const uint64_t *ax, const uint64_t *ay, MmZ *z, int32_t *w, gbx_mm_reg *regs, int32_t *n_regs)
{
    const uint64_t ALL = ~0ull;
    if (t.lane() == 0) {
        int64_t k = 0;
        for (int32_t i = 0; i < nch; ++i) {
            const uint32_t c = (uint32_t)u[i];
            const uint32_t h = (uint32_t)mm_hash64((mm_hash64(ax[k], ALL) + mm_hash64(ay[k], ALL)) ^ (uint64_t)r.hash, ALL);
            z[i].x = u[i] ^ (uint64_t)h;
            z[i].y = (uint64_t)k << 32 | c;
            k += c;
        }
    }
    t.sync();
    mm_team_sort(t, z, nch, MmZDesc());
    for (int32_t i = t.lane(); i < nch; i += t.size()) {
        gbx_mm_reg g;
        g.id = i; g.parent = -1; g.score = (int32_t)(z[i].x >> 32); g.hash = (uint32_t)z[i].x;
        g.cnt = (int32_t)(uint32_t)z[i].y; g.as = (int32_t)(z[i].y >> 32);
        g.subsc = g.n_sub = g.mapq = 0; g.read = read;
        const uint64_t *x = ax + g.as, *y = ay + g.as;
        const int32_t last = g.cnt - 1, sp = (int32_t)(y[0] >> 32 & 0xff);
        g.rev = (int32_t)(x[0] >> 63); g.rid = (int32_t)(x[0] << 1 >> 33);
        const int32_t rs = (int32_t)(uint32_t)x[0] + 1 - sp;
        g.rs = rs > 0 ? rs : 0; g.re = (int32_t)(uint32_t)x[last] + 1;
        const int32_t q0 = (int32_t)(uint32_t)y[0] + 1 - sp, q1 = (int32_t)(uint32_t)y[last] + 1;
        if (g.rev) { g.qs = r.qlen - q1; g.qe = r.qlen - q0; } else { g.qs = q0; g.qe = q1; }
        int32_t mlen = sp, blen = sp;
        for (int32_t m = 1; m <= last; ++m) {
            const int32_t span = (int32_t)(y[m] >> 32 & 0xff);
            const int32_t tl = (int32_t)(uint32_t)x[m] - (int32_t)(uint32_t)x[m - 1], ql = (int32_t)(uint32_t)y[m] - (int32_t)(uint32_t)y[m - 1];
            blen += tl > ql ? tl : ql;
            mlen += tl > span && ql > span ? span : tl < ql ? tl : ql;
        }
        g.mlen = mlen; g.blen = blen;
        regs[i] = g;
    }
    t.sync();
    if (t.lane() == 0) {
        int32_t n = nch;
        // ---- parents
        int32_t np = 0;
        if (n > 0) { w[0] = 0; regs[0].parent = 0; np = 1; }
        for (int32_t i = 1; i < n; ++i) {
            gbx_mm_reg &ri = regs[i];
            const int32_t si = ri.qs, ei = ri.qe;
            int32_t uncov = 0, xx = si;
            bool any = false;
            for (int64_t lastc = -1;;) {                              // the clipped intersections in ascending order, one a round
                int64_t best = INT64_MAX;
                for (int32_t j = 0; j < np; ++j) {
                    const gbx_mm_reg &rp = regs[w[j]];
                    int32_t sj = rp.qs, ej = rp.qe;
                    if (ej <= si || sj >= ei) continue;
                    any = true;
                    if (sj < si) sj = si;
                    if (ej > ei) ej = ei;
                    const int64_t c = (int64_t)sj << 32 | (int64_t)ej;
                    if (c > lastc && c < best) best = c;
                }
                if (best == INT64_MAX) break;
                const int32_t cs = (int32_t)(best >> 32), ce = (int32_t)(best & 0xffffffff);
                if (cs > xx) uncov += cs - xx;
                if (ce > xx) xx = ce;
                lastc = best;
            }
            if (any && ei > xx) uncov += ei - xx;
            int32_t j = 0;
            for (; j < np; ++j) {
                gbx_mm_reg &rp = regs[w[j]];
                const int32_t sj = rp.qs, ej = rp.qe;
                if (ej <= si || sj >= ei) continue;
                const int32_t li = ei - si, lj = ej - sj, mn = lj < li ? lj : li, mx = lj > li ? lj : li;
                const int32_t ol = (ei < ej ? ei : ej) - (si > sj ? si : sj);
                if ((float)ol / (float)mn - (float)uncov / (float)mx > P.mask_level) {
                    ri.parent = w[j];
                    if (ri.score > rp.subsc) rp.subsc = ri.score;
                    if (ri.cnt >= rp.cnt) ++rp.n_sub;
                    break;
                }
            }
            if (j == np) { w[np++] = i; ri.parent = i; ri.n_sub = 0; }
        }
        // ---- selection; w: old id -> new id
        if (P.pri_ratio > 0.0f && n > 0) {
            int32_t k = 0, n2 = 0;
            for (int32_t i = 0; i < n; ++i) {
                const gbx_mm_reg g = regs[i];
                bool keep = g.parent == i;
                if (!keep) {
                    const gbx_mm_reg &rp = regs[w[g.parent]];         // the parent where it already stands
                    if (((float)g.score >= (float)rp.score * P.pri_ratio || g.score + P.min_diff >= rp.score) && n2 < P.best_n &&
                        !(g.qs == rp.qs && g.qe == rp.qe && g.rid == rp.rid && g.rs == rp.rs && g.re == rp.re)) {
                        keep = true;
                        ++n2;
                    }
                }
                if (keep) {
                    w[i] = k;
                    regs[k] = g;
                    regs[k].id = k;
                    regs[k].parent = w[g.parent];
                    ++k;
                }
            }
            n = k;
        }
        // ---- mapq
        int64_t sum_sc = 0;
        for (int32_t i = 0; i < n; ++i)
            if (regs[i].parent == regs[i].id) sum_sc += regs[i].score;
        const float uniq_ratio = (float)sum_sc / (float)(sum_sc + r.rep_len);
        for (int32_t i = 0; i < n; ++i) {
            gbx_mm_reg &g = regs[i];
            if (g.parent != g.id) { g.mapq = 0; continue; }
            const float pen_s1 = (g.score > 100 ? 1.0f : 0.01f * (float)g.score) * uniq_ratio;
            const float pen_c = g.cnt > 10 ? 1.0f : 0.1f * (float)g.cnt;
            const float pen_cm = pen_s1 < pen_c ? pen_s1 : pen_c;
            const int32_t sub = g.subsc > P.min_chain_score ? g.subsc : P.min_chain_score;
            const float x = (float)sub / (float)g.score;
            int32_t q = (int32_t)(pen_cm * 40.0f * (1.0f - x) * mm_map_logf(g.score));
            q -= (int32_t)(4.343f * mm_map_logf(g.n_sub + 1) + .499f);
            g.mapq = q < 0 ? 0 : q > 60 ? 60 : q;
        }
        *n_regs = n;
    }
    t.sync();
}

// ---- PAF: the line of one region at out[at ..), written below cap only (out may be null: the length alone) -> its length
struct MmPafOut {
    uint8_t *out; int64_t at, cap, n;
    GBX_MM_HD void ch(uint8_t c) { if (out && at + n < cap) out[at + n] = c; ++n; }
    GBX_MM_HD void str(const char *s) { while (*s) ch((uint8_t)*s++); }
    GBX_MM_HD void bytes(const uint8_t *s, int64_t len) { for (int64_t i = 0; i < len; ++i) ch(s[i]); }
    GBX_MM_HD void num(int64_t v)
    {
        char d[24];
        int nd = 0;
        uint64_t a = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
        if (v < 0) ch('-');
        do { d[nd++] = (char)('0' + a % 10); a /= 10; } while (a);
        while (nd) ch((uint8_t)d[--nd]);
    }
};

GBX_MM_HD inline int64_t mm_paf_line(uint8_t *out, int64_t at, int64_t cap, const gbx_mm_reg &g, const uint8_t *qname, int64_t qname_len, int32_t qlen,
                                     const uint8_t *tname, int64_t tname_len, int32_t tlen, int32_t rep_len)
{
    MmPafOut o{out, at, cap, 0};
    o.bytes(qname, qname_len); o.ch('\t'); o.num(qlen); o.ch('\t'); o.num(g.qs); o.ch('\t'); o.num(g.qe); o.ch('\t');
    o.ch(g.rev ? '-' : '+'); o.ch('\t');
    if (tname) o.bytes(tname, tname_len); else o.ch('*');
    o.ch('\t'); o.num(tlen); o.ch('\t'); o.num(g.rs); o.ch('\t'); o.num(g.re); o.ch('\t');
    o.num(g.mlen); o.ch('\t'); o.num(g.blen); o.ch('\t'); o.num(g.mapq);
    o.str(g.parent == g.id ? "\ttp:A:P" : "\ttp:A:S");
    o.str("\tcm:i:"); o.num(g.cnt);
    o.str("\ts1:i:"); o.num(g.score);
    if (g.parent == g.id) { o.str("\ts2:i:"); o.num(g.subsc); }
    o.str("\trl:i:"); o.num(rep_len);
    o.ch('\n');
    return o.n;
}

// the driver's per-read hash: X31(name) ^ (W(qlen) + W(11))
GBX_MM_HD inline uint32_t mm_map_wang(uint32_t key)
{
    key += ~(key << 15); key ^= key >> 10; key += key << 3; key ^= key >> 6; key += ~(key << 11); key ^= key >> 16;
    return key;
}
GBX_MM_HD inline uint32_t mm_map_read_hash(const uint8_t *name, int64_t len, int32_t qlen)
{
    uint32_t h = len > 0 ? name[0] : 0;
    for (int64_t i = 1; i < len; ++i) h = (h << 5) - h + name[i];
    return h ^ (mm_map_wang((uint32_t)qlen) + mm_map_wang(11u));
}

}  // namespace gbx
