// damerau_harness.cpp -- host replay of the Damerau-Levenshtein kernels' shared code (strsim_damerau.h): the lane core
// (dl_lane_core, as k_dl_lane runs it: zero-padded 32-byte windows, the packed column records at a stride, loop bounds beyond the
// lane's own strings) and the strip walk of k_dl_wave (dl_strip_step over 64 emulated lanes, with the shift between the lanes, the
// two 64-column stages and the boundary row kept in place), each against the full-matrix DP.
//
// Built by tests/test_damerau_cpu.py as a shared library (g++ -shared), and with -DDAMERAU_HARNESS_MAIN as a stand-alone program
// that runs a sweep of both and exits non-zero on a mismatch -- the form the sanitizers are run on.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "strsim_damerau.h"

using namespace strsim;

namespace {

// Lowrance and Wagner, the whole matrix
uint32_t brute(const uint32_t *a, uint32_t la, const uint32_t *b, uint32_t lb)
{
    const uint32_t W = lb + 2, big = la + lb;
    std::vector<uint32_t> H((size_t)(la + 2) * W, big);
    for (uint32_t i = 0; i <= la; ++i) H[(size_t)(i + 1) * W + 1] = i;
    for (uint32_t j = 0; j <= lb; ++j) H[(size_t)W + j + 1] = j;
    std::map<uint32_t, uint32_t> last_row;
    for (uint32_t i = 1; i <= la; ++i) {
        uint32_t last_col = 0;
        for (uint32_t j = 1; j <= lb; ++j) {
            const auto f = last_row.find(b[j - 1]);
            const uint32_t k = f == last_row.end() ? 0u : f->second, l = last_col;
            uint32_t cost = 1;
            if (a[i - 1] == b[j - 1]) { cost = 0; last_col = j; }
            const uint32_t v = std::min(std::min(H[(size_t)i * W + j] + cost, H[(size_t)(i + 1) * W + j] + 1u),
                                        std::min(H[(size_t)i * W + j + 1] + 1u, H[(size_t)k * W + l] + (i - k - 1) + 1u + (j - l - 1)));
            H[(size_t)(i + 1) * W + j + 1] = v;
        }
        last_row[a[i - 1]] = i;
    }
    return H[(size_t)(la + 1) * W + lb + 1];
}

void window(const uint8_t *s, uint32_t len, uint32_t (&w)[8])
{
    uint8_t buf[32] = {};
    memcpy(buf, s, len);
    memcpy(w, buf, 32);
}

// k_dl_lane's pair: lit = 0 the longer string gives the rows, 1 / 2 the literal (a / b) gives the columns.  pslack / tslack: how
// far the wave's loop bounds lie beyond this lane's strings.  stride: the lane count of the record array.
uint32_t lane(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb, int lit, uint32_t pslack, uint32_t tslack, uint32_t stride)
{
    const bool a_is_pat = lit == 1 ? false : (lit == 2 ? true : la >= lb);
    const uint8_t *p = a_is_pat ? a : b, *t = a_is_pat ? b : a;
    const uint32_t lp = a_is_pat ? la : lb, lt = a_is_pat ? lb : la;
    uint32_t wp[8], wt[8];
    window(p, lp, wp);
    window(t, lt, wt);
    const uint32_t pmax = std::min(lp + pslack, DL_LANE_MAX), tmax = std::min(lt + tslack, DL_LANE_MAX);
    std::vector<uint32_t> col((size_t)DL_LANE_MAX * stride, 0xDEADBEEFu);
    const uint32_t d = dl_lane_core(wp, lp, pmax, wt, lt, tmax, col.data() + (stride - 1u), stride);
    // the lane's records lie in its own slot of every column and nowhere else
    for (size_t x = 0; x < col.size(); ++x)
        if (x % stride != stride - 1u && col[x] != 0xDEADBEEFu) return 0xFFFFFFFFu;
    return d;
}

// k_dl_wave's pair: the string with more values gives the rows.  cap: the columns the "LDS" boundary row holds; beyond it the walk
// uses a second array, laid out as the scratch slot is (pitch = slot_words / DL_COL_WORDS).
uint32_t walk(const uint32_t *a, uint32_t ca, const uint32_t *b, uint32_t cb, uint32_t cap, uint32_t slot_cols)
{
    const bool a_rows = ca >= cb;
    const uint32_t *rv = a_rows ? a : b, *cv = a_rows ? b : a;
    const uint32_t m = a_rows ? ca : cb, n = a_rows ? cb : ca;
    if (n == 0u) return m;
    std::vector<uint32_t> lds((size_t)DL_COL_WORDS * cap, 0u), scratch((size_t)dl_wave_slot_words(slot_cols), 0u);
    uint32_t *vals = lds.data();
    uint64_t pitch = cap;
    if (n > cap) {
        if ((uint64_t)DL_COL_WORDS * n > scratch.size()) return 0xFFFFFFFFu;
        vals = scratch.data();
        pitch = scratch.size() / DL_COL_WORDS;
    }
    uint32_t *bnd = vals + pitch;
    for (uint32_t j = 0; j < n; ++j) vals[j] = cv[j];
    const uint32_t strips = dl_strips(m);
    uint32_t last[64] = {};
    for (uint32_t s = 0; s < strips; ++s) {
        const uint32_t rs = dl_strip_rows(m, s);
        const bool more = s + 1u < strips;
        DlRow rw[64];
        DlCol c[64];
        uint32_t s_in[DL_COL_WORDS * 64u] = {}, s_out[4u * 64u] = {};
        for (uint32_t r = 0; r < 64u; ++r) {
            rw[r] = dl_row_start(64u * s + r + 1u, r < rs ? rv[64u * s + r] : 0xFFFFFFFFu);
            c[r] = dl_col_start(0u, 0u);
        }
        const uint32_t steps = dl_strip_steps(n, rs);
        for (uint32_t t = 0; t < steps; ++t) {
            if ((t & 63u) == 0u) {
                for (uint32_t r = 0; r < 64u; ++r) {
                    const uint32_t idx = t + r;
                    DlCol bc = dl_col_start(idx + 1u, 0u);
                    if (idx < n) {
                        if (idx >= pitch) return 0xFFFFFFFEu;
                        bc.ch = vals[idx];
                        if (s != 0u) {
                            bc.p1 = bnd[idx];
                            bc.p2 = bnd[pitch + idx];
                            bc.fr = bnd[2u * pitch + idx];
                            bc.k = bnd[3u * pitch + idx];
                        }
                    }
                    s_in[r] = bc.p1; s_in[64u + r] = bc.p2; s_in[128u + r] = bc.fr; s_in[192u + r] = bc.k; s_in[256u + r] = bc.ch;
                }
            }
            for (uint32_t r = 63u; r >= 1u; --r) c[r] = c[r - 1u]; // the shift down
            const uint32_t x = t & 63u;
            c[0] = DlCol{s_in[x], s_in[64u + x], s_in[128u + x], s_in[192u + x], s_in[256u + x]};
            uint32_t j63 = 0u;
            for (uint32_t r = 0; r < 64u; ++r) {
                const uint32_t j = dl_strip_step(rw[r], c[r], r, t, rs, n);
                if (r == 63u) j63 = j;
            }
            if (more) {
                if (j63 != dl_strip_col(63u, t, rs, n)) return 0xFFFFFFFDu;
                if (j63 != 0u) {
                    const uint32_t y = (j63 - 1u) & 63u;
                    s_out[y] = c[63].p1; s_out[64u + y] = c[63].p2; s_out[128u + y] = c[63].fr; s_out[192u + y] = c[63].k;
                    if (y == 63u || j63 == n) {
                        for (uint32_t r = 0; r <= y; ++r) {
                            const uint32_t idx = (j63 - 1u) - y + r;
                            if (idx >= n) return 0xFFFFFFFCu;
                            bnd[idx] = s_out[r];
                            bnd[pitch + idx] = s_out[64u + r];
                            bnd[2u * pitch + idx] = s_out[128u + r];
                            bnd[3u * pitch + idx] = s_out[192u + r];
                        }
                    }
                }
            }
        }
        for (uint32_t r = 0; r < 64u; ++r) last[r] = rw[r].left;
    }
    return last[(m - 1u) & 63u];
}

} // namespace

extern "C" {

uint32_t dl_lane_max_c(void) { return DL_LANE_MAX; }
uint32_t dl_wave_lds_cols_c(void) { return DL_WAVE_LDS_COLS; }
uint32_t dl_wave_small_cols_c(void) { return DL_WAVE_SMALL_COLS; }
uint64_t dl_wave_slot_words_c(uint64_t n) { return dl_wave_slot_words(n); }

// -> d, or a value >= 0xFFFFFFF0 when the replay itself went wrong
uint32_t dl_lane_c(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb, int lit, uint32_t pslack, uint32_t tslack, uint32_t stride)
{
    if (la > DL_LANE_MAX || lb > DL_LANE_MAX || stride == 0u) return 0xFFFFFFFBu;
    return lane(a, la, b, lb, lit, pslack, tslack, stride);
}

uint32_t dl_walk_c(const uint32_t *a, uint32_t ca, const uint32_t *b, uint32_t cb, uint32_t cap, uint32_t slot_cols)
{
    return walk(a, ca, b, cb, cap, slot_cols);
}

uint32_t dl_brute_c(const uint32_t *a, uint32_t ca, const uint32_t *b, uint32_t cb) { return brute(a, ca, b, cb); }

// what k_dl_lane does with a row, and what both kernels write
uint32_t dl_lane_row_c(int live, uint32_t la, uint32_t lb, int ascii, uint32_t k) { return dl_lane_row(live != 0, la, lb, ascii != 0, k); }
uint32_t dl_result_u32_c(uint64_t d, uint64_t la, uint64_t lb, uint32_t k) { return dist_result<uint32_t>(d, la, lb, k); }
double dl_result_f64_c(uint64_t d, uint64_t la, uint64_t lb) { return dist_result<double>(d, la, lb, DIST_UNBOUNDED); }

} // extern "C"

#ifdef DAMERAU_HARNESS_MAIN
int main()
{
    uint64_t state = 0x9E3779B97F4A7C15ull, bad = 0, done = 0;
    auto rnd = [&](uint32_t n) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((state >> 33) % n);
    };
    // the lane core: every length pair over three letters
    for (uint32_t la = 0; la <= DL_LANE_MAX; ++la)
        for (uint32_t lb = 0; lb <= DL_LANE_MAX; ++lb) {
            uint8_t a[32], b[32];
            uint32_t va[32], vb[32];
            for (uint32_t i = 0; i < la; ++i) va[i] = a[i] = (uint8_t)('a' + rnd(3));
            for (uint32_t i = 0; i < lb; ++i) vb[i] = b[i] = (uint8_t)(i < la && rnd(4) ? a[i] : 'a' + rnd(3));
            const uint32_t want = brute(va, la, vb, lb);
            for (int lit = 0; lit < 3; ++lit) {
                bad += lane(a, la, b, lb, lit, rnd(4), rnd(4), 1u + rnd(5)) != want;
                ++done;
            }
        }
    // the strip walk around the strip and the stage boundaries, in "LDS" and in "scratch"
    const uint32_t sizes[] = {1, 2, 63, 64, 65, 127, 128, 129, 200};
    for (uint32_t m : sizes)
        for (uint32_t n : sizes) {
            std::vector<uint32_t> a(m), b(n);
            for (auto &v : a) v = 0x100u + rnd(3);
            for (uint32_t i = 0; i < n; ++i) b[i] = i < m && rnd(4) ? a[i] : 0x100u + rnd(3);
            const uint32_t want = brute(a.data(), m, b.data(), n);
            bad += walk(a.data(), m, b.data(), n, 256u, 0u) != want;
            bad += walk(a.data(), m, b.data(), n, 16u, 200u) != want;
            done += 2;
        }
    printf("damerau_harness: %llu checks, %llu mismatches\n", (unsigned long long)done, (unsigned long long)bad);
    return bad != 0;
}
#endif
