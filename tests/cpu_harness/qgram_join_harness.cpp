// qgram_join_harness.cpp -- host build of what strsim_qgram_join.h shares with k_qgram_join_lane (strsim_qgram_join_kernels.h), for
// tests/test_qgram_join_cpu.py: g++ compiles the same headers.
//   qj_bound_check   for every pair of lengths 0 .. 32: the library's qgram_score over EVERY admissible (I, na, nb) -- multiset:
//                    I in 0 .. min(gq, gc) at na = gq, nb = gc; set: 1 <= na <= gq, 1 <= nb <= gc, I <= min(na, nb) -- against
//                    qgram_join_ub: no tuple above the bound, and the bound attained.
//   qj_need_mask     the library's need mask of a call, for the comparison with qgram_join_ub >= cutoff made directly.
//   qj_score_check   the uniform-text scoring call (qgram_join_pair, with qgram_join_first for the candidate's first occurrences and
//                    the query's distinct grams, as the kernels call them) against brute force over std::map, for every pair of
//                    lengths 0 .. 32 over one alphabet, in the 7-plane form and, where bits 5 and 6 of all bytes agree, the
//                    5-plane form.
//   qj_replay        join_replay_host of join_sweep_host.h under k_qgram_join_lane's own part: the lanes' words of the need mask
//                    and the lengths whose bit is set, a pair yielding the f64 of the scoring call over real strings, the brute
//                    force as what it must end with.
// Built as a shared library; with -DQGRAM_JOIN_HARNESS_MAIN it is a stand-alone program that runs every case (the form that is run
// under the address and undefined-behaviour sanitizers).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "join_sweep_host.h"
#include "strsim_qgram_join.h"

using namespace strsim;

// ---- the bound and the mask ----

extern "C" double qj_ub(int kind, uint32_t q, int set, uint32_t lq, uint32_t lc) { return qgram_join_ub(kind, q, set != 0, lq, lc); }

// 0, or how many length pairs have a tuple above the bound or none that attains it.
extern "C" uint32_t qj_bound_check(int kind, uint32_t q, int set)
{
    uint32_t bad = 0;
    for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq)
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
            const double ub = qgram_join_ub(kind, q, set != 0, lq, lc);
            const uint32_t gq = qgram_count(lq, q), gc = qgram_count(lc, q);
            bool above = false, attained = false;
            auto see = [&](double v) {
                if (!(v <= ub)) above = true; // (a NaN would count too)
                if (v == ub) attained = true;
            };
            if (gq == 0u || gc == 0u) {
                // a side without a gram: no formula.  Equal strings, which only equal lengths allow, are 1.0; unequal ones 0.0
                if (lq == lc) see(qgram_score(kind, 0u, gq, gc, true));
                if (lq != lc || lq > 0u) see(qgram_score(kind, 0u, gq, gc, false));
            } else if (set) {
                for (uint32_t na = 1; na <= gq; ++na)
                    for (uint32_t nb = 1; nb <= gc; ++nb)
                        for (uint32_t i = 0; i <= std::min(na, nb); ++i) see(qgram_score(kind, i, na, nb, false));
            } else {
                for (uint32_t i = 0; i <= std::min(gq, gc); ++i) see(qgram_score(kind, i, gq, gc, false));
            }
            if (above || !attained) ++bad;
        }
    return bad;
}

// The library's need mask of a call into out[33]; returns whether any bit is set.
extern "C" int qj_need_mask(int kind, uint32_t q, int set, double cutoff, uint64_t *out)
{
    MatchJoinNeed need;
    const bool any = qgram_join_need_mask(kind, q, set != 0, cutoff, need);
    memcpy(out, need.w, sizeof need.w);
    return any ? 1 : 0;
}

// The cutoffs of the suite: -inf, 0, 0.5, 0.8, 1.0, 1.5, and ub(kind, 2, multiset, 7, 9) with its two f64 neighbours.
extern "C" uint32_t qj_cutoffs(int kind, double *out)
{
    const double e = qgram_join_ub(kind, 2u, false, 7, 9), inf = std::numeric_limits<double>::infinity();
    const double cuts[9] = {-inf, 0.0, 0.5, 0.8, 1.0, 1.5, nextafter(e, 0.0), e, nextafter(e, 2.0)};
    memcpy(out, cuts, sizeof cuts);
    return 9u;
}

// ---- the scoring call ----

// A string of the lane class as k_match_pack leaves it: eight words, the length and the class bits of bits 5 / 6.
struct Packed {
    uint32_t w[8], len, cls, P[7], P5[5];
};

static Packed pack(const std::string &s)
{
    Packed p{};
    uint32_t any = 0u, all = 0xFFu;
    p.len = (uint32_t)s.size();
    for (uint32_t b = 0; b < p.len; ++b) {
        const uint32_t c = (uint8_t)s[b];
        any |= c;
        all &= c;
        p.w[b >> 2] |= c << (8u * (b & 3u));
    }
    p.cls = p.len ? ((any & 0x20u) ? 1u : 0u) | ((all & 0x20u) ? 0u : 2u) | ((any & 0x40u) ? 4u : 0u) | ((all & 0x40u) ? 0u : 8u) : 0u;
    build_planes<7>(p.w, p.P);
    for (int b = 0; b < 5; ++b) p.P5[b] = p.P[b];
    return p;
}

static bool five_planes(uint32_t cls) { return (cls & 3u) != 3u && (cls & 12u) != 12u; } // match_five_planes

// qgram_ref.score with std::map: the grams of both strings counted, then the library's epilogue.
static double brute(int kind, uint32_t q, bool set, const std::string &a, const std::string &b)
{
    std::map<std::string, std::pair<uint32_t, uint32_t>> cnt;
    uint32_t ga = 0, gb = 0;
    for (size_t i = 0; i + q <= a.size(); ++i, ++ga) ++cnt[a.substr(i, q)].first;
    for (size_t i = 0; i + q <= b.size(); ++i, ++gb) ++cnt[b.substr(i, q)].second;
    uint32_t isect = 0, na = set ? 0u : ga, nb = set ? 0u : gb;
    for (const auto &kv : cnt) {
        const uint32_t ca = kv.second.first, cb = kv.second.second;
        if (set) {
            isect += ca && cb ? 1u : 0u;
            na += ca ? 1u : 0u;
            nb += cb ? 1u : 0u;
        } else {
            isect += std::min(ca, cb);
        }
    }
    return qgram_score(kind, isect, na, nb, a == b);
}

// The score of (query, candidate) as k_qgram_join_lane forms it; wave_cls: the class bits of the wave's live queries.
template <int Q>
static double kernel_score(int kind, bool set, const Packed &qp, const Packed &cp, uint32_t wave_cls, int force_planes)
{
    // (tmax: any uniform bound at or above the length)
    const uint32_t first_c = set ? qgram_join_first<Q>(cp.w, cp.P, cp.len, 32u) : 0u;
    const uint32_t nbq = set ? popc32(qgram_join_first<Q>(qp.w, qp.P, qp.len, qp.len)) : 0u;
    const bool five = force_planes ? force_planes == 5 : five_planes(wave_cls | cp.cls);
    if (set) {
        return five ? qgram_join_pair<5, Q, true>(kind, cp.w, cp.len, first_c, qp.P5, qp.w[0], qp.len, nbq)
                    : qgram_join_pair<7, Q, true>(kind, cp.w, cp.len, first_c, qp.P, qp.w[0], qp.len, nbq);
    }
    return five ? qgram_join_pair<5, Q, false>(kind, cp.w, cp.len, first_c, qp.P5, qp.w[0], qp.len, nbq)
                : qgram_join_pair<7, Q, false>(kind, cp.w, cp.len, first_c, qp.P, qp.w[0], qp.len, nbq);
}

static double kernel_score_q(uint32_t q, int kind, bool set, const Packed &qp, const Packed &cp, uint32_t wave_cls, int force_planes)
{
    return q == 1u ? kernel_score<1>(kind, set, qp, cp, wave_cls, force_planes)
                   : q == 2u ? kernel_score<2>(kind, set, qp, cp, wave_cls, force_planes) : kernel_score<3>(kind, set, qp, cp, wave_cls, force_planes);
}

static std::string random_string(Rng &g, const std::string &alphabet, uint32_t len)
{
    std::string s(len, '\0');
    for (auto &c : s) c = alphabet[g.below((uint32_t)alphabet.size())];
    return s;
}

// alphabets: 0 "a", 1 "ab", 2 "abcdefgh", 3 all 128 ASCII bytes, 4 {NUL, a}
static std::string alphabet_of(int which)
{
    switch (which) {
    case 0: return "a";
    case 1: return "ab";
    case 2: return "abcdefgh";
    case 3: { std::string s; for (int c = 0; c < 128; ++c) s.push_back((char)c); return s; }
    default: return std::string("\0a", 2);
    }
}

// Every pair of lengths 0 .. 32 over one alphabet, `reps` random pairs each (one of them a near duplicate), all four kinds; the
// count of scores that differ from brute force in any bit.  stats[0] = pairs scored, stats[1] = of them in the 5-plane form.
extern "C" uint32_t qj_score_check(uint64_t seed, int alphabet, uint32_t q, int set, uint32_t reps, uint64_t *stats)
{
    Rng g{seed * 0x9E3779B97F4A7C15ull + 77u + (uint64_t)alphabet};
    const std::string alpha = alphabet_of(alphabet);
    uint32_t bad = 0;
    stats[0] = stats[1] = 0;
    for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq)
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc)
            for (uint32_t r = 0; r < reps; ++r) {
                const std::string a = random_string(g, alpha, lq);
                std::string b = random_string(g, alpha, lc);
                if (r == 0) { // a near duplicate: the query's bytes, one of them changed
                    for (uint32_t x = 0; x < std::min(lq, lc); ++x) b[x] = a[x];
                    if (lc && g.below(2)) b[g.below(lc)] = alpha[g.below((uint32_t)alpha.size())];
                }
                const Packed qp = pack(a), cp = pack(b);
                const bool can5 = five_planes(qp.cls | cp.cls);
                for (int kind = 0; kind < 4; ++kind) {
                    const double want = brute(kind, q, set != 0, a, b);
                    for (int planes = 5; planes <= 7; planes += 2) {
                        if (planes == 5 && !can5) continue;
                        const double got = kernel_score_q(q, kind, set != 0, qp, cp, qp.cls, planes);
                        ++stats[0];
                        stats[1] += planes == 5;
                        if (memcmp(&got, &want, 8)) ++bad;
                    }
                }
            }
    return bad;
}

// One pair, for the known answers of the Python side.
extern "C" double qj_score(int kind, uint32_t q, int set, const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb)
{
    const Packed qp = pack(std::string((const char *)a, la)), cp = pack(std::string((const char *)b, lb));
    return kernel_score_q(q, kind, set != 0, qp, cp, qp.cls, 0);
}

// ---- the replay ----

// What k_qgram_join_lane adds to the shared sweep, over real strings.
struct QgramCase {
    int kind;
    uint32_t q;
    bool set;
    const std::vector<Packed> &Q, &Cs;
    const std::vector<double> &want; // brute force, [i * nc + j]
    uint32_t wave_cls;
    double cutoff;
    MatchJoinNeed need;
    bool nothing;
    uint64_t allowed, seen;
    uint64_t *stats;

    double expected(uint32_t i, uint32_t j) const { return want[(size_t)i * Cs.size() + j]; }

    void lengths(JoinWave &W, bool fill, uint32_t split)
    {
        std::vector<uint64_t> mine(W.nq, 0);
        uint64_t wave = 0;
        for (uint32_t l = 0; l < MATCH_JOIN_LENGTHS; ++l) {
            const uint64_t w = need.w[l];
            bool any = false;
            for (uint32_t i = 0; i < W.nq; ++i)
                if (Q[i].len == l) { mine[i] = w; any = true; }
            if (any) wave |= w;
        }
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
            if (!((wave >> lc) & 1ull)) continue;
            seen |= 1ull << lc;
            join_slice_host(
                W, fill, split, lc, [&](uint32_t i) { return ((mine[i] >> lc) & 1ull) != 0ull; }, [&](uint32_t) { return MatchJoinRule{cutoff}; },
                [&](uint32_t i, uint32_t j) { return kernel_score_q(q, kind, set, Q[i], Cs[j], wave_cls, 0); });
        }
    }

    int after(const JoinWave &W, bool fill)
    {
        const uint64_t visited = seen;
        seen = 0;
        if (!fill) stats[2] = visited;
        if (visited != allowed) return 13; // exactly the lengths whose bit is set in some live lane's word
        if (fill) return 0;
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) // (and a clear bit is a true statement)
            for (uint32_t i = 0; i < W.nq; ++i)
                if (!match_join_needs(need, Q[i].len, lc) && qgram_join_ub(kind, q, set, Q[i].len, lc) >= cutoff) return 14;
        return 0;
    }
};

// nq <= 64 queries and nc candidates of random lengths 0 .. maxlen over "abc", a third of the candidates near duplicates of a query.
// stats[0] = candidates visited by one sweep, stats[1] = hits, stats[2] = the lengths the count sweep visited (bits).  0, or the
// number of the first check that failed.
extern "C" int qj_replay(uint64_t seed, int kind, uint32_t q, int set, uint32_t nq, uint32_t nc, uint32_t maxlen, double cutoff, int upper,
                         uint32_t splits, int undersize, uint32_t shift, uint64_t *stats)
{
    Rng g{seed * 2654435761ull + 12345u + (uint64_t)kind * 977u + q * 31u + (set ? 7u : 0u)};
    const std::string alpha = "abc";
    std::vector<std::string> qs(nq), cs(nc);
    for (auto &s : qs) s = random_string(g, alpha, g.below(maxlen + 1));
    for (auto &s : cs) {
        s = random_string(g, alpha, g.below(maxlen + 1));
        if (nq && g.below(3) == 0u) {
            s = qs[g.below(nq)];
            if (!s.empty() && g.below(2)) s[g.below((uint32_t)s.size())] = alpha[g.below(3)];
            if (g.below(3) == 0u && s.size() < maxlen) s.push_back(alpha[g.below(3)]);
        }
    }
    std::vector<Packed> Q, Cs;
    std::vector<uint32_t> clen;
    uint32_t wave_cls = 0;
    for (auto &s : qs) { Q.push_back(pack(s)); wave_cls |= Q.back().cls; }
    for (auto &s : cs) { Cs.push_back(pack(s)); clen.push_back((uint32_t)s.size()); }
    std::vector<double> want((size_t)nq * nc);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < nc; ++j) want[(size_t)i * nc + j] = brute(kind, q, set != 0, qs[i], cs[j]);
    stats[2] = 0;
    QgramCase C{kind, q, set != 0, Q, Cs, want, wave_cls, cutoff, {}, false, 0, 0, stats};
    C.nothing = !qgram_join_need_mask(kind, q, set != 0, cutoff, C.need);
    for (uint32_t i = 0; i < nq; ++i) C.allowed |= C.need.w[Q[i].len];
    return join_replay_host(C, nq, clen, upper != 0, splits, undersize, shift, stats);
}

// Every case of the sweep; the count of failures.
extern "C" uint32_t qj_replay_all(void)
{
    uint32_t failed = 0;
    uint64_t stats[3];
    double cuts[9];
    for (int kind = 0; kind < 4; ++kind) {
        const uint32_t ncuts = qj_cutoffs(kind, cuts);
        for (uint32_t q = 1; q <= 3; ++q)
            for (int set = 0; set < 2; ++set)
                for (uint32_t c = 0; c < ncuts; ++c)
                    for (int upper = 0; upper < 2; ++upper)
                        for (uint32_t splits = 1; splits <= 3; ++splits) {
                            const uint32_t shift = (splits + c) % 3u; // hit-map groups of 1, 2 and 4 positions
                            const int under = (int)((c + q + (uint32_t)upper) & 1u);
                            const uint64_t seed = splits;
                            const uint32_t nq = seed == 1 ? 1u : seed == 2 ? 64u : 23u;
                            const uint32_t nc = 40u + (uint32_t)seed * 17u;
                            if (qj_replay(seed + 100 * c, kind, q, set, nq, nc, seed == 3 ? 6u : 32u, cuts[c], upper, splits, under, shift, stats)) ++failed;
                        }
    }
    return failed;
}

#ifdef QGRAM_JOIN_HARNESS_MAIN
int main()
{
    uint32_t bounds = 0, masks = 0, scores = 0;
    double cuts[9];
    uint64_t stats[3];
    for (int kind = 0; kind < 4; ++kind)
        for (uint32_t q = 1; q <= 3; ++q)
            for (int set = 0; set < 2; ++set) {
                bounds += qj_bound_check(kind, q, set);
                const uint32_t ncuts = qj_cutoffs(kind, cuts);
                for (uint32_t c = 0; c < ncuts; ++c) {
                    uint64_t w[MATCH_JOIN_LENGTHS];
                    qj_need_mask(kind, q, set, cuts[c], w);
                    for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq)
                        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc)
                            masks += (((w[lq] >> lc) & 1ull) != 0ull) != (qgram_join_ub(kind, q, set != 0, lq, lc) >= cuts[c]);
                }
            }
    for (int alphabet = 0; alphabet < 5; ++alphabet)
        for (uint32_t q = 1; q <= 3; ++q)
            for (int set = 0; set < 2; ++set) scores += qj_score_check(1, alphabet, q, set, 2, stats);
    const uint32_t failed = qj_replay_all();
    printf("qgram_join harness: %u length pairs off their bound, %u mask bits differ, %u scores differ, %u replays failed\n", bounds, masks, scores,
           failed);
    return bounds || masks || scores || failed ? 1 : 0;
}
#endif
