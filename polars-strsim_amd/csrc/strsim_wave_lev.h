// strsim_wave_lev.h -- Levenshtein behind the lane kernels: block-parallel Myers with DPP hand-off.  The block kernels of
// k_wave_pairs<LEVENSHTEIN> (BYTES batches: both strings ASCII, 64 pattern rows per lane, wave_lev_blocks64; SYMBOLS batches:
// anything else inside the BMP, 32 rows of 16-bit symbols per lane, wave_lev_blocks), the ASCII staging, and k_huge_pairs' row of
// any length in stripes (wave_lev_stripes, huge_levenshtein).
// Included by strsim_kernel_wave.h inside namespace strsim, behind the decode and the anti-diagonal fallback it uses and in front
// of the kernel that uses it.  Reference semantics: strsim.rs:125-160 (Levenshtein on `char`s).
#pragma once

// Levenshtein: a row with a string beyond WAVE_CAP BYTES still runs in k_wave_pairs' SYMBOLS batches when both strings
// have at most WAVE_CAP scalar values (e.g. 600 Cyrillic letters = 1 200 bytes); k_huge_pairs applies the same test
// and leaves such rows alone.
constexpr uint32_t LEV_SYMBOL_ROUTE_MAX_BYTES = 4u * WAVE_CAP;
__device__ __forceinline__ bool lev_fits_symbols(const uint8_t *__restrict__ pa, uint32_t la8, const uint8_t *__restrict__ pb,
                                                 uint32_t lb8)
{
    if (la8 > LEV_SYMBOL_ROUTE_MAX_BYTES || lb8 > LEV_SYMBOL_ROUTE_MAX_BYTES) return false;
    return wave_count_chars(pa, la8) <= (uint32_t)WAVE_CAP && wave_count_chars(pb, lb8) <= (uint32_t)WAVE_CAP;
}

// Levenshtein distance, block-based bit-parallel DP (Myers 1999 / Hyyro 2003, the published "advanced block" step), up to
// LEV_JOBS pairs per wave, each in its own run of lanes (sum of runs <= 64).  Within a job, lane k owns a block of rows of the
// SHORTER string (the pattern) as bit-planes in registers -- 64 bytes of an ASCII pair (two mask words, wave_lev_blocks64), 32
// scalar values of any other pair inside the BMP (one mask word, wave_lev_blocks) -- and the LONGER string (the text, staged in
// the wave's global arena) supplies the columns: that orientation needs the fewest lane-steps, blocks * (n + blocks - 1).
// Block k works on column t-k at step t and hands its bottom-row delta (+1/0/-1) to block k+1 through a one-lane DPP shift.
// The pattern is left-aligned to the top of its last block (window that ENDS at the end of the string), so every hand-off and
// the score row are the block's top bit.
__device__ __forceinline__ uint32_t bfe_u32(uint32_t w, uint32_t off, uint32_t width)
{
    return (uint32_t)__builtin_amdgcn_ubfe(w, off, width); // width 0 -> 0
}

// One pair of a batch.  Two kinds of batches: BYTES (both strings ASCII: the pattern is read straight from its column,
// the text is staged as bytes; wave_lev_blocks64, a lane per 64 pattern rows) and SYMBOLS (any UTF-8 inside the Basic
// Multilingual Plane: both strings are decoded by the wave and staged as 16-bit scalar values; wave_lev_blocks, a lane
// per 32 pattern rows).
struct BlockJob {
    uint32_t p0;      // BYTES: byte offset of the pattern (the SHORTER string) in its column
    uint32_t row;     // row of the frame
    uint16_t m, n;    // pattern / text length (bytes = scalar values for BYTES, scalar values for SYMBOLS)
    uint16_t txt;     // the staged text starts at unit 4 * txt of the batch's text arena (front pad included)
    uint8_t seg;      // first lane of the job's run of lanes: ceil(m / 64) (BYTES) or ceil(m / 32) (SYMBOLS)
    uint8_t in_a;     // BYTES: the pattern lives in column A
};

constexpr int LEV_TAB_WORDS = 2 * LUT_ENTRIES * 64; // LDS words of a wave's match tables: the split tables of strsim_lane_lut.h, one per mask word of a lane (6 KB)

struct BlockCols { // the two value columns (BYTES batches read their patterns from them)
    const uint8_t *valA, *valB;
    uint32_t totalA, totalB;
};

// SYMBOLS batches: 16-bit symbols, 32 pattern rows per lane.  Match masks: the masks of the low five bits of a symbol come
// from the split tables of strsim_lane_lut.h, built per lane in LDS when the batch starts (each lane writes and reads its
// own column only), and a step reads its mask instead of computing it; the higher bits are compared with bit-planes on top
// of that, as many as vary inside the batch: two for one script block (NP = 7), up to bit 10 or bit 15 for mixed scripts /
// CJK (NP = 11, 16): 22 + 2 * (NP - 5) VALU per step.
// (`cols` is not read here.  It stays in the signature because without it the compiler numbers the scalar spill slots of
// k_wave_pairs<0> differently: the device code is then no longer byte for byte what it was, profiles/wave_split_isa.txt.)
template <int NP>
__device__ __forceinline__ void wave_lev_blocks(const BlockJob *jobs, uint32_t njobs, uint32_t T, const BlockCols &cols, const uint8_t *arena,
                                                const uint16_t *pats, uint32_t *tab, double *__restrict__ out)
{
    static_assert(NP == 7 || NP == 11 || NP == 16, "five tabulated planes plus 2, 6 or 11 computed ones");
    const uint32_t lane = lane_id();
    uint32_t jdx = 0;
    for (uint32_t q = 1; q < njobs; ++q) jdx += lane >= (uint32_t)jobs[q].seg ? 1u : 0u;
    const uint32_t m = jobs[jdx].m, n = jobs[jdx].n;
    const uint32_t blk = lane - jobs[jdx].seg;
    const uint32_t B = (m + 31u) >> 5;
    const bool mine = blk < B; // lanes past the last job's run fall into it with blk >= B
    const uint32_t s = 32u * B - m; // fictitious shared-prefix rows at the bottom of block 0 (0..31)
    uint32_t P[NP];
    {
        // the 32 scalar values of this block were staged end-aligned (zeros in front of the string) at pats[lane * 32]
        uint32_t w[16];
        const uint4 *src = reinterpret_cast<const uint4 *>(pats + lane * 32u);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint4 v = mine ? src[d] : make_uint4(0u, 0u, 0u, 0u);
            w[4 * d] = v.x; w[4 * d + 1] = v.y; w[4 * d + 2] = v.z; w[4 * d + 3] = v.w;
        }
        build_planes_sym<NP>([&](int k) { return (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu; }, P);
    }
    const uint32_t valid = blk == 0u ? ~low_ones(s) : 0xFFFFFFFFu;
    uint32_t Pv = valid, Mv = ~valid;
    // Hand-off of a block's bottom row to the block above it in the job (the next lane): the -1 as a bit (it joins the match
    // mask at bit 0), the +1 as the block's whole Ph word -- the neighbour takes its top bit with the v_alignbit that shifts its
    // own Ph.  The first block of a job (and lane 0, which the DPP shift fills with 0) ORs the top bit in: the row above block 0
    // grows by one per column, whatever the last block of the job in front left in its word.
    const uint32_t first_top = blk == 0u ? 0x80000000u : 0u;
    const uint32_t pubw = blk + 1u == B ? 0u : 1u;  // field width of the published -1 bit (the LAST block of a job publishes 0)
    uint32_t houtP = 0u, houtN = 0u;
    // Column j = t - blk of the text at step t.  A staged text has TXT_PAD units in front and behind (never used as
    // columns: a block is idle for blk <= 31 steps before its own columns), so a lane just walks on: four columns
    // per four steps, fetched two trips ahead with one unaligned load; once past its text (the batch runs for the
    // longest job) the fetch position stops at the rear pad.
    typedef uint64_t u64_unaligned __attribute__((aligned(2)));
    const uint8_t *const col0 = arena + 4u * (uint32_t)jobs[jdx].txt + 2 * TXT_PAD;
    const uint32_t ncol = mine ? n : 0u;
    const int32_t jlast = (int32_t)n + TXT_PAD - 4; // last position a four-column fetch may start at
    int32_t j = -(int32_t)blk;
    auto fetch = [&](int32_t at) -> uint64_t { // four columns
        at = at < jlast ? at : jlast;
        return *reinterpret_cast<const u64_unaligned *>(col0 + 2 * at);
    };
    auto step = [&](uint32_t Eq0) {
        uint32_t hinP = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)houtP, 0x138 /* wave_shr:1 */, 0xF, 0xF, true) | first_top;
        asm volatile("" : "+v"(hinP)); // one v_or_b32_dpp (the compiler would move the OR behind the shift that uses it)
        const uint32_t hinN = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)houtN, 0x138, 0xF, 0xF, true);
        if ((uint32_t)j < ncol) {
            const uint32_t Xv = Eq0 | Mv;
            const uint32_t Eq = Eq0 | hinN;
            const uint32_t Xh = bitop3<0xBE>((Eq & Pv) + Pv, Pv, Eq); // (sum ^ Pv) | Eq
            const uint32_t Ph = bitop3<0xF1>(Mv, Xh, Pv);             // Mv | ~(Xh | Pv)
            const uint32_t Mh = Pv & Xh;
            houtP = Ph;
            houtN = bfe_u32(Mh, 31u, pubw);
            const uint32_t PhS = (uint32_t)__builtin_amdgcn_alignbit(Ph, hinP, 31), MhS = (Mh << 1) | hinN;
            Pv = bitop3<0xF1>(MhS, Xv, PhS);                          // MhS | ~(Xv | PhS)
            Mv = PhS & Xv;
        }
        ++j;
    };
    uint64_t w0 = fetch(j), w1 = fetch(j + 4);
    uint32_t t = 0;
    // the split tables of strsim_lane_lut.h (12 entries, 3 KB per wave): Eq(c) = L[c & 7] & M[(c >> 3) & 3]
    EqLut tl;
    tl.lane4 = lane * 4u;
    tl.krep = (STRSIM_LDS_ADDR(tab) >> 8) * 0x01010101u;
    {
        uint32_t P5[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) P5[k] = P[k];
        lut_build<5>(tl, P5, valid);
    }
    // column q (0..3) of the fetched word: its 32-bit half (the symbol starts at bit 16 * (q & 1) of it)
    auto half = [&](uint64_t w, int q) { return (uint32_t)(w >> (32 * (q >> 1))); };
    // mask of column q of w: the two table entries of its low five bits, then the higher planes
    auto high_planes = [&](uint32_t e, uint64_t w, int q) {
#pragma unroll
        for (int k = 5; k < NP; ++k) e = bitop3<0x90>(e, P[k], (uint32_t)__builtin_amdgcn_sbfe((int)half(w, q), 16 * (q & 1) + k, 1u));
        return e;
    };
    auto lookup = [&](const LutIndex &ix, int q) { // ix: the table coordinates of the bytes of half(w, q)
        return lut_read(tl, ix.l, 2 * (q & 1)) & lut_read(tl, ix.m, 2 * (q & 1));
    };
    auto trip = [&](uint64_t w) { // four steps on the four columns of w
        uint32_t e[4];
        const LutIndex ix0 = lut_index(tl, half(w, 0));
        const LutIndex ix1 = lut_index(tl, half(w, 2));
#pragma unroll
        for (int q = 0; q < 4; ++q) e[q] = lookup(q < 2 ? ix0 : ix1, q);
#pragma unroll
        for (int q = 0; q < 4; ++q) step(high_planes(e[q], w, q));
    };
    __builtin_amdgcn_s_setprio(0); // the step loop yields to waves that are staging their next batch (loads to issue)
    // three words in flight, refilled in turn (no register is copied, so no load is waited for before its turn)
    uint64_t w2 = fetch(j + 8);
    for (; t + 12u <= T; t += 12u) {
        trip(w0); w0 = fetch(j + 8);
        trip(w1); w1 = fetch(j + 8);
        trip(w2); w2 = fetch(j + 8);
    }
    if (t + 4u <= T) {
        trip(w0); t += 4u; w0 = w1; w1 = w2;
        if (t + 4u <= T) { trip(w0); t += 4u; w0 = w1; }
    }
    for (; t < T; ++t, w0 >>= 16) step(high_planes(lookup(lut_index(tl, (uint32_t)w0), 0), w0, 0));
    __builtin_amdgcn_s_setprio(1);
    // No running score: every block stops updating after its last column, so once all are done the column-n vertical
    // deltas are in Pv/Mv.  The row above block 0 sits at s + n (it starts at s because the s fictitious rows below it
    // start at -1 each), hence  D[m][n] = s + n + sum over the job's blocks of popc(Pv) - popc(Mv).
    int pre = mine ? (int)popc32(Pv) - (int)popc32(Mv) : 0; // -> inclusive prefix sum over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(pre, d);
        if (lane >= (uint32_t)d) pre += up;
    }
    // lane q finishes job q
    const uint32_t q = lane < njobs ? lane : 0u;
    const uint32_t qseg = jobs[q].seg, qm = jobs[q].m, qn = jobs[q].n;
    const uint32_t qB = (qm + 31u) >> 5;
    const int hi_sum = __shfl(pre, (int)(qseg + qB - 1u));
    const int lo_sum = __shfl(pre, (int)(qseg ? qseg - 1u : 0u));
    if (lane < njobs) {
        const int sum = hi_sum - (qseg ? lo_sum : 0);
        const uint32_t dist = (uint32_t)((int)(32u * qB - qm + qn) + sum);
        out[jobs[q].row] = epilogue_levenshtein(dist, qm, qn);
    }
}

// The block step for BYTES batches, with SIXTY-FOUR pattern rows per lane (two mask words): what a step spends per lane
// whatever the word holds -- the hand-off through DPP, its decoding and publishing, the column test, the table addresses --
// is paid once per 64 cells instead of once per 32 (about 12 of the 23 instructions of the one-word step; the two-word
// step is 30 + 3.5 for the table addresses and the text fetch: 0.7 of two one-word steps).  A job takes ceil(m / 64)
// lanes.  The match masks come from the split tables of strsim_lane_lut.h (L[c & 7] & M[(c >> 3) & 3], 12 entries per
// word).  Low words at tab (4 KB-aligned), high words 3 KB above; one address (a v_perm_b32) serves both.  Same recurrences,
// hand-off and distance formula as above.
template <int NP>
__device__ __forceinline__ void wave_lev_blocks64(const BlockJob *jobs, uint32_t njobs, uint32_t T, const BlockCols &cols,
                                                  const uint8_t *arena, uint32_t *tab, double *__restrict__ out)
{
    static_assert(NP == 5 || NP == 7, "ASCII: five tabulated planes plus 0 or 2 computed ones");
    const uint32_t lane = lane_id();
    uint32_t jdx = 0;
    for (uint32_t q = 1; q < njobs; ++q) jdx += lane >= (uint32_t)jobs[q].seg ? 1u : 0u;
    const uint32_t m = jobs[jdx].m, n = jobs[jdx].n;
    const uint32_t blk = lane - jobs[jdx].seg;
    const uint32_t B = (m + 63u) >> 6;
    const bool mine = blk < B;
    const uint32_t s = 64u * B - m; // fictitious shared-prefix rows at the bottom of block 0 (0..63)
    uint32_t Plo[NP], Phi[NP];
    {
        const bool in_a = jobs[jdx].in_a != 0;
        uint32_t w[16];
#pragma unroll
        for (int d = 0; d < 16; ++d) w[d] = 0u;
        if (mine)
            load_window_any<16>(in_a ? cols.valA : cols.valB, (int64_t)jobs[jdx].p0 + (int64_t)m - 64 * (int64_t)(B - blk),
                                in_a ? cols.totalA : cols.totalB, w);
        uint32_t h[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) h[d] = w[d];
        build_planes<NP>(h, Plo);
#pragma unroll
        for (int d = 0; d < 8; ++d) h[d] = w[8 + d];
        build_planes<NP>(h, Phi);
    }
    const uint64_t valid = blk == 0u ? ~((1ull << s) - 1ull) : ~0ull;
    uint64_t Pv = valid, Mv = ~valid;
    const uint32_t first = blk == 0u ? 1u : 0u;
    const uint32_t pubw = blk + 1u == B ? 0u : 1u;
    // Hand-off: the +1 and the -1 leaving a block's bottom row travel in two registers, so neither side packs or unpacks
    // anything.  The +1 is not even extracted: the neighbour fetches the block's whole top Ph word (one v_or_b32_dpp that also
    // sets the top bit for the first block of a job -- whatever the last block of the job in front of it left there) and
    // shifts its top bit into its own Ph with the v_alignbit that shifts Ph anyway.  The -1 is needed at bit 0 as well (it joins
    // the match mask), so it is published as a bit.
    uint32_t houtP = 0u, houtN = 0u;
    const uint32_t first_top = first << 31;
    typedef uint32_t u32_unaligned __attribute__((aligned(1)));
    const uint32_t txt0 = 4u * (uint32_t)jobs[jdx].txt + TXT_PAD; // this job's column 0 in the arena (uniform base + 32-bit offset)
    const uint32_t ncol = mine ? n : 0u;
    const uint32_t end = mine ? blk + n : 0u;   // first step at which this block has no column left
    const int32_t jlast = (int32_t)n + TXT_PAD - 4;
    uint32_t tt = 0u;                            // the step (uniform); this block's column is tt - blk
    const uint32_t fetch0 = txt0 - blk, fetch_last = txt0 + (uint32_t)jlast; // (blk <= 15 < TXT_PAD <= txt0)
    auto fetch = [&](uint32_t ahead) -> uint32_t { // columns tt + ahead - blk .. + 3 of this lane's text, not past its rear pad
        const uint32_t at = tt + ahead + fetch0;
        return *reinterpret_cast<const u32_unaligned *>(arena + (at < fetch_last ? at : fetch_last));
    };
    // the tables: this lane's column of the low-word table at tab, of the high-word table 3 KB above
    EqLut tl, th;
    tl.lane4 = th.lane4 = lane * 4u;
    tl.krep = (STRSIM_LDS_ADDR(tab) >> 8) * 0x01010101u;
    th.krep = ((STRSIM_LDS_ADDR(tab) >> 8) + (uint32_t)LUT_ENTRIES) * 0x01010101u;
    lut_build<NP>(tl, Plo, (uint32_t)valid);
    lut_build<NP>(th, Phi, (uint32_t)(valid >> 32));
    struct Col { uint32_t llo, lhi, mlo, mhi; };
    auto lookup = [&](const LutIndex &ix, uint32_t w, int q) {
        const uint32_t al = __builtin_amdgcn_perm(ix.l, tl.lane4, 0x0C0C0000u | ((4u + (uint32_t)q) << 8));
        const uint32_t am = __builtin_amdgcn_perm(ix.m, tl.lane4, 0x0C0C0000u | ((4u + (uint32_t)q) << 8));
        Col c;
#if defined(__HIP_DEVICE_COMPILE__)
        c.llo = lut_lds_read(al); c.lhi = lut_lds_read(al + (uint32_t)LUT_WAVE_BYTES);
        c.mlo = lut_lds_read(am); c.mhi = lut_lds_read(am + (uint32_t)LUT_WAVE_BYTES);
#else
        c.llo = c.lhi = al; c.mlo = c.mhi = am; // (host pass of hipcc: never run)
#endif
#pragma unroll
        for (int k = 5; k < NP; ++k) { // planes 5.. on top of M: m & ~(P_k ^ bit k of the column's byte)
            const uint32_t fill = bit_fill(w, 8 * q + k);
            c.mlo = bitop3<0x90>(c.mlo, Plo[k < NP ? k : 0], fill);
            c.mhi = bitop3<0x90>(c.mhi, Phi[k < NP ? k : 0], fill);
        }
        return c;
    };
    // RAMP: the first steps, while blocks are still starting (block k runs columns from step k on); after step 16 every
    // block has started and "has a column left" is one compare against the uniform step.
    auto step = [&](const Col &c, auto ramp) {
        uint32_t hinP = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)houtP, 0x138 /* wave_shr:1 */, 0xF, 0xF, true) | first_top;
        asm volatile("" : "+v"(hinP)); // keeps the OR next to the move (one v_or_b32_dpp) instead of behind the shift that uses it
        const uint32_t hinN = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)houtN, 0x138, 0xF, 0xF, true);
        const bool on = decltype(ramp)::value ? (tt - blk) < ncol : tt < end;
        if (on) {
            const uint32_t Pvl = (uint32_t)Pv, Pvh = (uint32_t)(Pv >> 32), Mvl = (uint32_t)Mv, Mvh = (uint32_t)(Mv >> 32);
            const uint32_t Xvl = bitop3<0xEA>(c.llo, c.mlo, Mvl), Xvh = bitop3<0xEA>(c.lhi, c.mhi, Mvh); // Eq0 | Mv
            const uint32_t Eql = bitop3<0xEA>(c.llo, c.mlo, hinN), Eqh = c.lhi & c.mhi;                    // Eq0 | hinN
            uint64_t masked = ((uint64_t)(Eqh & Pvh) << 32) | (Eql & Pvl);
            asm volatile("" : "+v"(masked)); // one 64-bit add on the register pair (left alone the compiler adds the halves apart: + 1)
            const uint64_t sum = masked + Pv;
            const uint32_t Xhl = bitop3<0xBE>((uint32_t)sum, Pvl, Eql), Xhh = bitop3<0xBE>((uint32_t)(sum >> 32), Pvh, Eqh);
            const uint32_t Phl = bitop3<0xF1>(Mvl, Xhl, Pvl), Phh = bitop3<0xF1>(Mvh, Xhh, Pvh);
            const uint32_t Mhl = Pvl & Xhl, Mhh = Pvh & Xhh;
            houtP = Phh;
            houtN = bfe_u32(Mhh, 31u, pubw);
            const uint32_t PhSl = (uint32_t)__builtin_amdgcn_alignbit(Phl, hinP, 31), PhSh = (uint32_t)__builtin_amdgcn_alignbit(Phh, Phl, 31);
            const uint32_t MhSl = (Mhl << 1) | hinN, MhSh = (uint32_t)__builtin_amdgcn_alignbit(Mhh, Mhl, 31);
            Pv = ((uint64_t)bitop3<0xF1>(MhSh, Xvh, PhSh) << 32) | bitop3<0xF1>(MhSl, Xvl, PhSl);
            Mv = ((uint64_t)(PhSh & Xvh) << 32) | (PhSl & Xvl);
        }
        ++tt;
    };
    uint32_t w0 = fetch(0u), w1 = fetch(4u);
    auto trip = [&](uint32_t w, auto ramp) { // four steps on the four columns of w
        const LutIndex ix = lut_index(tl, w);
        Col c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = lookup(ix, w, q);
#pragma unroll
        for (int q = 0; q < 4; ++q) step(c[q], ramp);
    };
    __builtin_amdgcn_s_setprio(0);
    uint32_t w2 = fetch(8u);
    // three words in flight, refilled in turn (before a trip, the word two trips ahead of it is the one fetched: + 8 columns)
    const std::true_type ramp_on{};
    const std::false_type ramp_off{};
    for (; tt < 24u && tt + 12u <= T;) {
        trip(w0, ramp_on); w0 = fetch(8u);
        trip(w1, ramp_on); w1 = fetch(8u);
        trip(w2, ramp_on); w2 = fetch(8u);
    }
    for (; tt + 12u <= T;) {
        trip(w0, ramp_off); w0 = fetch(8u);
        trip(w1, ramp_off); w1 = fetch(8u);
        trip(w2, ramp_off); w2 = fetch(8u);
    }
    if (tt + 4u <= T) {
        trip(w0, ramp_on); w0 = w1; w1 = w2;
        if (tt + 4u <= T) { trip(w0, ramp_on); w0 = w1; }
    }
    for (; tt < T; w0 >>= 8) step(lookup(lut_index(tl, w0), w0, 0), ramp_on);
    __builtin_amdgcn_s_setprio(1);
    int pre = mine ? (int)popc32((uint32_t)Pv) + (int)popc32((uint32_t)(Pv >> 32)) - (int)popc32((uint32_t)Mv) -
                         (int)popc32((uint32_t)(Mv >> 32))
                   : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(pre, d);
        if (lane >= (uint32_t)d) pre += up;
    }
    const uint32_t q = lane < njobs ? lane : 0u;
    const uint32_t qseg = jobs[q].seg, qm = jobs[q].m, qn = jobs[q].n;
    const uint32_t qB = (qm + 63u) >> 6;
    const int hi_sum = __shfl(pre, (int)(qseg + qB - 1u));
    const int lo_sum = __shfl(pre, (int)(qseg ? qseg - 1u : 0u));
    if (lane < njobs) {
        const int sum = hi_sum - (qseg ? lo_sum : 0);
        const uint32_t dist = (uint32_t)((int)(64u * qB - qm + qn) + sum);
        out[jobs[q].row] = epilogue_levenshtein(dist, qm, qn);
    }
}

// The same block step for ONE pair of any length (k_huge_pairs): both strings decoded to 32-bit scalar values in the
// global workspace, the pattern (the one with fewer values) cut into stripes of 64 blocks = 2048 rows that run one
// after the other over all the columns.  The bottom-row deltas of a stripe go through a byte array hb[column]
// (global, written by the stripe's last block 63 steps after block 0 of the same stripe consumed the entry the
// previous stripe left there); the distance is s + n + the vertical deltas of every block at its last column.
// txt[-TXT_PAD .. n + TXT_PAD) and hb[-TXT_PAD .. n + TXT_PAD) must be readable.  Scalar values <= 0xFFFF.
template <int NP>
__device__ __forceinline__ uint32_t wave_lev_stripes(const uint32_t *pat, uint32_t m, const uint32_t *txt, uint32_t n,
                                                     uint8_t *hb, uint32_t *tab)
{
    typedef uint32_t u32_unaligned __attribute__((aligned(1)));
    struct u32x4 { uint32_t v[4]; };
    const uint32_t lane = lane_id();
    const uint32_t Btot = (m + 31u) >> 5;
    const uint32_t s = 32u * Btot - m;
    int total = 0;
    uint32_t *const trow = tab + lane;
    const int32_t jlast = (int32_t)n + TXT_PAD - 4;
    for (uint32_t g0 = 0; g0 < Btot; g0 += 64u) {
        const uint32_t nb = Btot - g0 < 64u ? Btot - g0 : 64u;
        const bool mine = lane < nb;
        const uint32_t g = g0 + lane;
        const bool later = g0 != 0u;            // block 0 of this stripe is fed from hb[]
        const bool more = g0 + 64u < Btot;      // the last block of this stripe feeds hb[]
        uint32_t w[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const int64_t idx = (int64_t)g * 32 - (int64_t)s + k;
            w[k] = (mine && idx >= 0) ? pat[idx] : 0u;
        }
        uint32_t P[NP];
        build_planes_sym<NP>([&](int k) { return w[k] & 0xFFFFu; }, P);
        const uint32_t valid = g == 0u ? ~low_ones(s) : 0xFFFFFFFFu;
        uint32_t Pv = valid, Mv = ~valid;
        const uint32_t first = g == 0u ? 1u : 0u;
        const uint32_t pubw = g + 1u == Btot ? 0u : 1u;
        const uint32_t pubn = g + 1u == Btot ? 0u : 2u;
        uint32_t hout = 0u;
        {
            uint32_t P5[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) P5[k] = P[k];
#pragma unroll
            for (int code = 0; code < 32; ++code) trow[code * 64] = eq_mask<5>(P5, valid, (uint32_t)code, 0);
        }
        const uint32_t ncol = mine ? n : 0u;
        const bool feeder = more && lane + 1u == nb;
        int32_t j = -(int32_t)lane;
        auto clampj = [&](int32_t at) { return at < jlast ? at : jlast; };
        auto fetch_t = [&](int32_t at) { return *reinterpret_cast<const u32x4 *>(txt + clampj(at)); };
        auto fetch_h = [&](int32_t at) { return *reinterpret_cast<const u32_unaligned *>(hb + clampj(at)); };
        const uint32_t T = n + nb - 1u;
        auto trip = [&](const u32x4 &wt, uint32_t wh, uint32_t t) { // four steps on the four columns of wt
            uint32_t e[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) e[q] = trow[(wt.v[q] & 31u) * 64u];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t hin = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hout, 0x138 /* wave_shr:1 */, 0xF, 0xF, true);
                if (later && lane == 0u) hin = (wh >> (8 * q)) & 3u;
                if (t + (uint32_t)q < T && (uint32_t)j < ncol) {
                    uint32_t Eq0 = e[q];
#pragma unroll
                    for (int k = 5; k < NP; ++k) Eq0 = bitop3<0x90>(Eq0, P[k], bit_fill(wt.v[q], k));
                    const uint32_t hinP = (hin & 1u) | first, hinN = hin >> 1;
                    const uint32_t Xv = Eq0 | Mv;
                    const uint32_t Eq = Eq0 | hinN;
                    const uint32_t Xh = bitop3<0xBE>((Eq & Pv) + Pv, Pv, Eq);
                    const uint32_t Ph = bitop3<0xF1>(Mv, Xh, Pv);
                    const uint32_t Mh = Pv & Xh;
                    hout = bfe_u32(Ph, 31u, pubw) | ((Mh >> 30) & pubn);
                    const uint32_t PhS = (Ph << 1) | hinP, MhS = (Mh << 1) | hinN;
                    Pv = bitop3<0xF1>(MhS, Xv, PhS);
                    Mv = PhS & Xv;
                    if (feeder) hb[j] = (uint8_t)hout;
                }
                ++j;
            }
        };
        // two words in flight, refilled in turn one trip ahead of their use
        u32x4 ta = fetch_t(j), tb = fetch_t(j + 4);
        uint32_t ha = later ? fetch_h(j) : 0u, hc = later ? fetch_h(j + 4) : 0u; // only lane 0 uses them
        for (uint32_t t = 0; t < T; t += 8u) {
            trip(ta, ha, t);
            ta = fetch_t(j + 4);
            if (later) ha = fetch_h(j + 4);
            if (t + 4u < T) {
                trip(tb, hc, t + 4u);
                tb = fetch_t(j + 4);
                if (later) hc = fetch_h(j + 4);
            }
        }
        int v = mine ? (int)popc32(Pv) - (int)popc32(Mv) : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        total += v;
        __syncthreads(); // hb[] written by this stripe is read by the next one (same wave: the barrier's workgroup-scope fence orders its plain global stores before those loads)
    }
    return (uint32_t)((int)(s + n) + total);
}

// Copy the ASCII string p[0, len) into LDS bytes and/or just test it: returns true when every byte is < 0x80.
// or6/and6 accumulate, wave-uniformly, whether bits 5 and 6 are set in any / in every byte (plane-count choice).
// One pass over the two strings of a pair: are all their bytes ASCII, which of bits 5 / 6 vary over them (or6 / and6
// accumulate over the jobs of a batch), and the text copied to its arena slot `dst` (4-aligned).
__device__ __forceinline__ bool wave_ascii_stage(const uint8_t *__restrict__ pat, uint32_t mlen, const uint8_t *__restrict__ txt,
                                                 uint32_t nlen, uint8_t *dst, uint32_t &or6, uint32_t &and6)
{
    // Four bytes per lane and trip (a string of 1 024 bytes: 4 trips; both strings in the same trip, so their loads are in
    // flight together), OR / AND of the bytes kept per lane and reduced over the wave once at the end.  Until late in round 3:
    // a pass per string, a byte per lane and five ballots per trip -- a tenth of k_wave_pairs<levenshtein>'s instructions on
    // cfg5 and, one row after the other, a latency chain per row (207 -> 241 M pairs/s).  Staged, the last dword of a text
    // reaches up to 3 bytes into its rear pad.
    typedef uint32_t u32_unaligned __attribute__((aligned(1)));
    const uint32_t lane = lane_id();
    uint32_t o = 0u, a = 0xFFFFFFFFu;
    auto dword = [&](const uint8_t *p, uint32_t len, uint32_t i) {
        const uint32_t rem = len - i;
        uint32_t w;
        if (rem >= 4u) {
            w = *reinterpret_cast<const u32_unaligned *>(p + i);
        } else { // the string's last one to three bytes, one by one: nothing is read behind a string
            w = p[i];
            if (rem > 1u) w |= (uint32_t)p[i + 1u] << 8;
            if (rem > 2u) w |= (uint32_t)p[i + 2u] << 16;
        }
        const uint32_t keep = rem >= 4u ? 0xFFFFFFFFu : ((1u << (8u * rem)) - 1u);
        o |= w & keep;
        a &= w | ~keep;
        return w;
    };
    const uint32_t longest = mlen > nlen ? mlen : nlen;
    for (uint32_t c0 = 0; c0 < longest; c0 += 256u) {
        const uint32_t i = c0 + 4u * lane;
        if (i < nlen) *reinterpret_cast<uint32_t *>(dst + i) = dword(txt, nlen, i);
        if (i < mlen) (void)dword(pat, mlen, i);
    }
    if (__ballot((o & 0x20202020u) != 0u) != 0ull) or6 |= 0x20u;
    if (__ballot((o & 0x40404040u) != 0u) != 0ull) or6 |= 0x40u;
    if (__ballot((a & 0x20202020u) != 0x20202020u) != 0ull) and6 &= ~0x20u;
    if (__ballot((a & 0x40404040u) != 0x40404040u) != 0ull) and6 &= ~0x40u;
    return __ballot((o & 0x80808080u) != 0u) == 0ull;
}

// Levenshtein similarity of one pair of any length (k_huge_pairs): decode, then the striped block kernel with as many
// bit-planes as the pair's scalar values need; values beyond the BMP fall back to the anti-diagonal DP.
__device__ __forceinline__ double huge_levenshtein(const uint8_t *__restrict__ pa, uint32_t la8, const uint8_t *__restrict__ pb,
                                                   uint32_t lb8, uint32_t *sA, uint32_t *sB, uint32_t *aux, uint32_t *tab)
{
    const uint32_t lane = lane_id();
    if (la8 == 0u && lb8 == 0u) return 1.0;
    if (la8 == 0u || lb8 == 0u) return 0.0;
    bool nonascii = false;
    __syncthreads();
    const uint32_t la = wave_decode(pa, la8, sA, nonascii);
    const uint32_t lb = wave_decode(pb, lb8, sB, nonascii);
    uint32_t o = 0u, a_ = 0xFFFFFFFFu;
    for (uint32_t i = lane; i < la; i += 64u) { o |= sA[i]; a_ &= sA[i]; }
    for (uint32_t i = lane; i < lb; i += 64u) { o |= sB[i]; a_ &= sB[i]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        o |= (uint32_t)__shfl_xor((int)o, d);
        a_ &= (uint32_t)__shfl_xor((int)a_, d);
    }
    o = uniform(o);
    const uint32_t vary = uniform(o ^ a_);
    uint32_t dist;
    if (o > 0xFFFFu) {
        dist = wave_levenshtein(sA, la, sB, lb, aux);
    } else {
        const bool a_pat = la <= lb;
        const uint32_t *pat = a_pat ? sA : sB, *txt = a_pat ? sB : sA;
        const uint32_t m = a_pat ? la : lb, n = a_pat ? lb : la;
        uint8_t *hb = reinterpret_cast<uint8_t *>(aux) + 64;
        if (vary >> 11) dist = wave_lev_stripes<16>(pat, m, txt, n, hb, tab);
        else if (vary >> 7) dist = wave_lev_stripes<11>(pat, m, txt, n, hb, tab);
        else dist = wave_lev_stripes<7>(pat, m, txt, n, hb, tab);
    }
    return epilogue_levenshtein(dist, la, lb);
}
