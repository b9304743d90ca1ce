// distance_join_harness.cpp -- host build of what strsim_distance_join.h shares with k_distance_join_lane
// (strsim_distance_join_kernels.h), for tests/test_distance_join_cpu.py: g++ compiles the same headers.
//   dj_facts_check   exhaustively over every ordered pair of strings over an alphabet up to a length: the three facts of the
//                    Damerau-Levenshtein filter (dl <= osa; osa <= 2 -> dl == osa; osa <= 2 dl) with full-matrix DPs of its own,
//                    the uniform-text cores against those DPs, and for k = 0 .. 4 and unbounded the decision of the sweep (the OSA
//                    core, distance_join_undecided, dl_lane_core) against the full-matrix distance: the same hits, and on a hit
//                    the same d.
//   dj_need_mask     the library's need mask of a call, for the comparison with | lq - lc | <= k made directly.
//   dj_replay        join_replay_host of join_sweep_host.h under k_distance_join_lane's own part: the lanes' words of the need
//                    mask and the lengths whose bit is set, a pair yielding the distance of the kind's scoring call over real
//                    strings, -(double) of the brute-force distance as what it must end with.
// Built as a shared library; with -DDISTANCE_JOIN_HARNESS_MAIN it is a stand-alone program that runs every case (the form that is
// run under the address and undefined-behaviour sanitizers).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "join_sweep_host.h"
#include "strsim_distance_join.h"

using namespace strsim;

static const uint32_t KS[6] = {0u, 1u, 2u, 3u, 4u, DIST_UNBOUNDED};

// ---- full-matrix references ----

static uint32_t ref_lev(const std::string &a, const std::string &b, bool transpose)
{
    const size_t n = a.size(), m = b.size();
    std::vector<std::vector<uint32_t>> D(n + 1, std::vector<uint32_t>(m + 1));
    for (size_t i = 0; i <= n; ++i) D[i][0] = (uint32_t)i;
    for (size_t j = 0; j <= m; ++j) D[0][j] = (uint32_t)j;
    for (size_t i = 1; i <= n; ++i)
        for (size_t j = 1; j <= m; ++j) {
            uint32_t v = std::min({D[i - 1][j - 1] + (a[i - 1] != b[j - 1] ? 1u : 0u), D[i - 1][j] + 1u, D[i][j - 1] + 1u});
            if (transpose && i > 1 && j > 1 && a[i - 1] == b[j - 2] && a[i - 2] == b[j - 1]) v = std::min(v, D[i - 2][j - 2] + 1u);
            D[i][j] = v;
        }
    return D[n][m];
}

// Lowrance and Wagner, the whole matrix with the table of last rows
static uint32_t ref_dl(const std::string &a, const std::string &b)
{
    const size_t n = a.size(), m = b.size();
    const uint32_t big = (uint32_t)(n + m);
    std::vector<std::vector<uint32_t>> H(n + 2, std::vector<uint32_t>(m + 2, big));
    for (size_t i = 0; i <= n; ++i) H[i + 1][1] = (uint32_t)i;
    for (size_t j = 0; j <= m; ++j) H[1][j + 1] = (uint32_t)j;
    std::map<char, size_t> last_row;
    for (size_t i = 1; i <= n; ++i) {
        size_t last_col = 0;
        for (size_t j = 1; j <= m; ++j) {
            const size_t k = last_row.count(b[j - 1]) ? last_row[b[j - 1]] : 0, l = last_col;
            uint32_t cost = 1;
            if (a[i - 1] == b[j - 1]) { cost = 0; last_col = j; }
            H[i + 1][j + 1] = std::min({H[i][j] + cost, H[i + 1][j] + 1u, H[i][j + 1] + 1u, H[k][l] + (uint32_t)((i - k - 1) + 1 + (j - l - 1))});
        }
        last_row[a[i - 1]] = i;
    }
    return H[n + 1][m + 1];
}

static uint32_t ref_distance(int kind, const std::string &a, const std::string &b)
{
    return kind == EDIT_DAMERAU ? ref_dl(a, b) : ref_lev(a, b, kind == EDIT_OSA);
}

// ---- the scoring calls as the kernel makes them ----

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

// d of (query, candidate) as k_distance_join_lane<kind> forms it under the cutoff k; the column records of the cell DP are col
// (DL_LANE_MAX words between two guard words, checked by the caller).
static uint32_t kernel_distance(int kind, uint32_t k, const Packed &qp, const Packed &cp, bool five, uint32_t *col)
{
    if (kind == EDIT_LEVENSHTEIN)
        return five ? nearest_lev_uniform_text<5>(cp.w, cp.len, qp.P5, qp.len) : nearest_lev_uniform_text<7>(cp.w, cp.len, qp.P, qp.len);
    const uint32_t o = five ? nearest_osa_uniform_text<5>(cp.w, cp.len, qp.P5, qp.len) : nearest_osa_uniform_text<7>(cp.w, cp.len, qp.P, qp.len);
    if (kind == EDIT_OSA) return o;
    return distance_join_damerau_pair(o, k, qp.w, qp.len, cp.w, cp.len, col, 1u);
}

// stats: [0] ordered pairs, [1] violations of a fact, [2] pairs with dl < osa, [3] pairs undecided at k = 2 (| lq - lc | <= 2 and
// 3 <= osa <= 4), [4] decisions that differ from the full-matrix distance, [5] cores that differ from their DP, [6] cell DPs run.
extern "C" uint32_t dj_facts_check(uint32_t alphabet, uint32_t maxlen, uint64_t *stats)
{
    std::vector<std::string> all{""};
    for (size_t from = 0, len = 1; len <= maxlen; ++len) {
        const size_t to = all.size();
        for (size_t x = from; x < to; ++x)
            for (uint32_t c = 0; c < alphabet; ++c) all.push_back(all[x] + (char)('a' + c));
        from = to;
    }
    std::vector<Packed> P;
    for (auto &s : all) P.push_back(pack(s));
    for (int x = 0; x < 7; ++x) stats[x] = 0;
    const uint32_t GUARD = 0xC0FFEE11u;
    std::vector<uint32_t> col(DL_LANE_MAX + 2);
    for (size_t i = 0; i < all.size(); ++i)
        for (size_t j = 0; j < all.size(); ++j) {
            const std::string &a = all[i], &b = all[j];
            const uint32_t lev = ref_lev(a, b, false), o = ref_lev(a, b, true), dl = ref_dl(a, b);
            ++stats[0];
            if (!(dl <= o)) ++stats[1];
            if (o <= 2u && dl != o) ++stats[1];
            if (!(o <= lev && lev <= 2u * dl)) ++stats[1];
            if (dl < o) ++stats[2];
            if (distance_join_needs(P[i].len, P[j].len, 2u) && distance_join_undecided(o, 2u)) ++stats[3];
            const bool can5 = five_planes(P[i].cls | P[j].cls);
            for (int five = 0; five <= (can5 ? 1 : 0); ++five) {
                if (kernel_distance(EDIT_LEVENSHTEIN, 0u, P[i], P[j], five != 0, nullptr) != lev) ++stats[5];
                if (kernel_distance(EDIT_OSA, 0u, P[i], P[j], five != 0, nullptr) != o) ++stats[5];
            }
            for (uint32_t k : KS) {
                std::fill(col.begin(), col.end(), GUARD);
                const uint32_t d = kernel_distance(EDIT_DAMERAU, k, P[i], P[j], can5, col.data() + 1);
                if (col.front() != GUARD || col.back() != GUARD) ++stats[4];
                if (col[1] != GUARD) ++stats[6];
                const bool hit = distance_join_hit(d, k, false, 0u, 0u);
                if (hit != (dl <= k) || (hit && d != dl)) ++stats[4];
                if (k <= 1u && col[1] != GUARD) ++stats[4]; // at k <= 1 nothing is ever undecided
            }
        }
    return (uint32_t)(stats[1] + stats[4] + stats[5]);
}

// The library's need mask of a call into out[33].
extern "C" void dj_need_mask(uint32_t k, uint64_t *out)
{
    MatchJoinNeed need;
    distance_join_need_mask(k, need);
    memcpy(out, need.w, sizeof need.w);
}

extern "C" double dj_cutoff(uint32_t k) { return distance_join_cutoff(k); }

// 0, or the mask bits of the call at k that differ from | lq - lc | <= k.
extern "C" uint32_t dj_need_check(uint32_t k)
{
    uint64_t w[MATCH_JOIN_LENGTHS];
    dj_need_mask(k, w);
    uint32_t bad = 0;
    for (uint32_t lq = 0; lq < MATCH_JOIN_LENGTHS; ++lq) {
        if (w[lq] >> MATCH_JOIN_LENGTHS) ++bad;
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
            const uint64_t diff = lq > lc ? lq - lc : lc - lq;
            bad += (((w[lq] >> lc) & 1ull) != 0ull) != (diff <= (uint64_t)k);
        }
    }
    return bad;
}

// One pair, for the known answers of the Python side.
extern "C" uint32_t dj_distance(int kind, uint32_t k, const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb)
{
    const Packed qp = pack(std::string((const char *)a, la)), cp = pack(std::string((const char *)b, lb));
    uint32_t col[DL_LANE_MAX];
    return kernel_distance(kind, k, qp, cp, five_planes(qp.cls | cp.cls), col);
}

// ---- the replay ----

static std::string random_string(Rng &g, const std::string &alphabet, uint32_t len)
{
    std::string s(len, '\0');
    for (auto &c : s) c = alphabet[g.below((uint32_t)alphabet.size())];
    return s;
}

// What k_distance_join_lane adds to the shared sweep, over real strings.
struct DistanceCase {
    int kind;
    uint32_t k;
    const std::vector<Packed> &Q, &Cs;
    const std::vector<uint32_t> &want; // brute force, [i * nc + j]
    uint32_t wave_cls;
    double cutoff;
    MatchJoinNeed need;
    bool nothing;
    uint64_t allowed, seen;
    uint64_t *stats;

    double expected(uint32_t i, uint32_t j) const { return -(double)want[(size_t)i * Cs.size() + j]; }

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
        uint32_t col[DL_LANE_MAX];
        for (uint32_t lc = 0; lc < MATCH_JOIN_LENGTHS; ++lc) {
            if (!((wave >> lc) & 1ull)) continue;
            seen |= 1ull << lc;
            join_slice_host(
                W, fill, split, lc, [&](uint32_t i) { return ((mine[i] >> lc) & 1ull) != 0ull; }, [&](uint32_t) { return DistanceJoinRule{k}; },
                [&](uint32_t i, uint32_t j) { return kernel_distance(kind, k, Q[i], Cs[j], five_planes(wave_cls | Cs[j].cls), col); });
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
                if (!match_join_needs(need, Q[i].len, lc) && (Q[i].len > lc ? Q[i].len - lc : lc - Q[i].len) <= k) return 14;
        return 0;
    }
};

// nq <= 64 queries and nc candidates of random lengths 0 .. maxlen over "abc", a third of the candidates edited copies of a query
// (a substitution, a swap of two neighbours, an appended byte).  stats[0] = candidates visited by one sweep, stats[1] = hits,
// stats[2] = the lengths the count sweep visited (bits).  0, or the number of the first check that failed.
extern "C" int dj_replay(uint64_t seed, int kind, uint32_t k, uint32_t nq, uint32_t nc, uint32_t maxlen, int upper, uint32_t splits, int undersize,
                         uint32_t shift, uint64_t *stats)
{
    Rng g{seed * 2654435761ull + 4321u + (uint64_t)kind * 977u + (uint64_t)(k & 255u) * 31u};
    const std::string alpha = "abc";
    std::vector<std::string> qs(nq), cs(nc);
    for (auto &s : qs) s = random_string(g, alpha, g.below(maxlen + 1));
    for (auto &s : cs) {
        s = random_string(g, alpha, g.below(maxlen + 1));
        if (nq && g.below(3) == 0u) {
            s = qs[g.below(nq)];
            if (!s.empty() && g.below(2)) s[g.below((uint32_t)s.size())] = alpha[g.below(3)];
            for (uint32_t t = g.below(3); t > 0u && s.size() >= 2; --t) {
                const uint32_t at = g.below((uint32_t)s.size() - 1u);
                std::swap(s[at], s[at + 1]);
            }
            if (g.below(3) == 0u && s.size() < maxlen) s.insert(s.begin() + g.below((uint32_t)s.size() + 1u), alpha[g.below(3)]);
        }
    }
    std::vector<Packed> Q, Cs;
    std::vector<uint32_t> clen;
    uint32_t wave_cls = 0;
    for (auto &s : qs) { Q.push_back(pack(s)); wave_cls |= Q.back().cls; }
    for (auto &s : cs) { Cs.push_back(pack(s)); clen.push_back((uint32_t)s.size()); }
    std::vector<uint32_t> want((size_t)nq * nc);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < nc; ++j) want[(size_t)i * nc + j] = ref_distance(kind, qs[i], cs[j]);
    stats[2] = 0;
    DistanceCase C{kind, k, Q, Cs, want, wave_cls, distance_join_cutoff(k), {}, false, 0, 0, stats};
    distance_join_need_mask(k, C.need);
    for (uint32_t i = 0; i < nq; ++i) C.allowed |= C.need.w[Q[i].len];
    return join_replay_host(C, nq, clen, upper != 0, splits, undersize, shift, stats);
}

// Every case of the sweep; the count of failures.
extern "C" uint32_t dj_replay_all(void)
{
    uint32_t failed = 0;
    uint64_t stats[3];
    for (int kind = 0; kind < 3; ++kind)
        for (uint32_t c = 0; c < 6; ++c)
            for (int upper = 0; upper < 2; ++upper)
                for (uint32_t splits = 1; splits <= 3; ++splits) {
                    const uint32_t shift = (splits + c) % 3u; // hit-map groups of 1, 2 and 4 positions
                    const int under = (int)((c + (uint32_t)kind + (uint32_t)upper) & 1u);
                    const uint64_t seed = splits;
                    const uint32_t nq = seed == 1 ? 1u : seed == 2 ? 64u : 23u;
                    const uint32_t nc = 40u + (uint32_t)seed * 17u;
                    if (dj_replay(seed + 100 * c, kind, KS[c], nq, nc, seed == 3 ? 6u : 32u, upper, splits, under, shift, stats)) ++failed;
                }
    return failed;
}

#ifdef DISTANCE_JOIN_HARNESS_MAIN
int main()
{
    uint64_t s3[7], s2[7];
    const uint32_t bad3 = dj_facts_check(3, 5, s3), bad2 = dj_facts_check(2, 7, s2);
    uint32_t masks = 0;
    for (uint32_t k : KS) masks += dj_need_check(k);
    masks += dj_need_check(31u) + dj_need_check(32u) + dj_need_check(33u) + dj_need_check(0xFFFFFFFEu);
    const uint32_t failed = dj_replay_all();
    printf("distance_join harness: %llu ordered pairs, %llu fact violations, %llu decisions differ, %llu cores differ, %llu pairs with dl < osa, "
           "%llu undecided at k = 2, %u mask bits differ, %u replays failed\n",
           (unsigned long long)(s3[0] + s2[0]), (unsigned long long)(s3[1] + s2[1]), (unsigned long long)(s3[4] + s2[4]),
           (unsigned long long)(s3[5] + s2[5]), (unsigned long long)(s3[2] + s2[2]), (unsigned long long)(s3[3] + s2[3]), masks, failed);
    return bad3 || bad2 || masks || failed ? 1 : 0;
}
#endif
